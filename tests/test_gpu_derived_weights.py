"""Every derived form of a weight (conv_ops._cached) after every weight writer, on the GPU: the FORMS x WRITERS matrix of
tests/derived_cases.py at the layer level -- after a write the call equals, bit for bit, the same call on fresh Parameters and stays
within the route's bound of a float64 reference from the current weights -- and at the model level: the generator's forward after
fused, plain, validated and graph-replayed updates equals the forward of a fresh generator loaded from the current weights."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import derived_cases as dc  # noqa: E402

import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import _native, conv_ops, synthetic, validation  # noqa: E402
from video_frame_inpainting_amd.environments import create_eval_environment, create_training_environment  # noqa: E402
from video_frame_inpainting_amd.options import TrainOptions  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(autouse=True)
def _fp32_convs():
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False


# ---------------------------------------------------------------------------------------------------------------- forms x writers

_INPUTS, _FIRST_REF = {}, {}      # per form: the inputs, and the reference of the initial weights (the same in every pair of the form)


def _setup(form):
    if form.name not in _INPUTS:
        _INPUTS[form.name] = form.inputs()
    module = form.module(DEV)
    if form.name not in _FIRST_REF:
        _FIRST_REF[form.name] = form.ref(module, _INPUTS[form.name])
    return module, _INPUTS[form.name], dc.to_device(_INPUTS[form.name], DEV)


def _assert_within_bound(form, got, ref, label):
    """check (b): every output within bound x max |ref| of the float64 reference from the current weights"""
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        scale, err = dc.max_abs(r), dc.max_abs(g.detach().double().cpu() - r)
        print('%s, %s, output %d: max |gpu - fp64| = %.3g = %.3g of max |fp64| (bound %.0e)' % (form.name, label, i, err, err / scale, form.bound))
        assert scale > 0 and err <= form.bound * scale, (form.name, label, i, err, scale)


def _assert_equals_fresh(form, got, module, inp, ref, label):
    """check (a): the same call on fresh Parameters cloned from the current weights -- the same kernel, the same inputs, a form just
    built: the same bits.  (MIOpen's route: inside the bound.)"""
    want = form.call(form.fresh(module), inp)
    assert len(got) == len(want)
    for i, (g, w, r) in enumerate(zip(got, want, ref)):
        if form.exact:
            assert torch.equal(g, w), '%s, %s, output %d: differs from the call on fresh Parameters by %.3g (max |fp64| %.3g)' % (
                form.name, label, i, dc.max_abs(g - w), dc.max_abs(r))
        else:
            assert dc.max_abs(g - w) <= form.bound * dc.max_abs(r), (form.name, label, i)


@pytest.mark.parametrize('pair', dc.pairs(on_gpu=True), ids=dc.pair_id)
def test_every_form_follows_every_writer(pair, monkeypatch):
    form, writer = pair
    with form.routed(monkeypatch):
        module, inp_cpu, inp = _setup(form)
        got = form.call(module, inp)                       # fills the cache
        form.assert_tags(module)
        _assert_within_bound(form, got, _FIRST_REF[form.name], 'before')
        phases = []

        def check(label):
            got = form.call(module, inp)
            form.assert_tags(module)
            ref = form.ref(module, inp_cpu)
            _assert_equals_fresh(form, got, module, inp, ref, label)
            _assert_within_bound(form, got, ref, label)
            phases.append(label)
        writer.fn(dc.Case(form, module, DEV, None), check)
        assert len(phases) == len(writer.writes)


@pytest.mark.parametrize('writer', ['adam', 'fused_step'])
@pytest.mark.parametrize('form', dc.FORMS, ids=dc.FORM_IDS)
def test_after_a_write_the_cache_still_caches(form, writer, monkeypatch):
    """The call after a write rebuilds the row's forms (new objects); two further calls rebuild nothing: no weight transform, no
    bf16 packing, and the cached objects stay the ones they were."""
    if writer == 'fused_step' and not form.trained:
        writer = 'load_state_dict'                         # the inference-only rows: another writer in the fused step's place
    counts = {'transform': 0, 'pack': 0}
    transform, launch = conv_ops._transform, _native.launch

    def counted_transform(*a, **k):
        counts['transform'] += 1
        return transform(*a, **k)

    def counted_launch(name, *a, **k):
        counts['pack'] += name == 'tai_conv_bf16_pack_weights'
        return launch(name, *a, **k)
    monkeypatch.setattr(conv_ops, '_transform', counted_transform)
    monkeypatch.setattr(_native, 'launch', counted_launch)
    with form.routed(monkeypatch):
        module, _, inp = _setup(form)
        form.call(module, inp)
        first = form.derived(module)
        built = dict(counts)
        assert built['transform'] + built['pack'] > 0 or all(t[0] in ('direct', 'input_half') for _, t, _ in first)
        form.call(module, inp)
        assert counts == built and all(a[2] is b[2] for a, b in zip(first, form.derived(module)))       # nothing changed: nothing rebuilt
        dc.WRITER[writer].fn(dc.Case(form, module, DEV, None), lambda label: None)
        form.call(module, inp)
        second = form.derived(module)
        assert all(a[2] is not b[2] for a, b in zip(first, second)), 'a form survived the write'
        assert {k: counts[k] - built[k] for k in counts} == built, (counts, built)                       # rebuilt once, all of them
        after = dict(counts)
        for _ in range(2):
            form.call(module, inp)
        assert counts == after and all(a[2] is b[2] for a, b in zip(second, form.derived(module)))


# ---------------------------------------------------------------------------------------------------------------- the model

MODEL = '{"class": "TAIFillInModel", "args": [16, 1, 3, 51], "kwargs": {"num_block": 5, "kf_dim": 16}}'
K = T = F = 3
SIZE, B, LR = 64, 2, 1e-2
KEYS = ('pred', 'pred_forward', 'pred_backward', 'interp_net_outputs_1', 'interp_net_outputs_2')
_CLIPS = {}


def _clips(i):
    if 'all' not in _CLIPS:
        _CLIPS['all'] = torch.from_numpy(synthetic.make_clips(4 * B, K + T + F, 1, SIZE, SIZE, synthetic.SEEDS['cfg3']))
    return _CLIPS['all'][B * (i % 4):B * (i % 4) + B]


def _env(tmp_path, name, **kw):
    torch.manual_seed(0)
    np.random.seed(0)
    env = create_training_environment(vfi.create_model(MODEL), 1, str(tmp_path / 'ckpt'), name, K, T, F, [SIZE, SIZE], 1.0, 0.02, LR, 0.5,
                                      16, 3, 3, [0, 0], device=DEV, **kw)
    env.K, env.T, env.F = K, T, F
    return env


def _update(env, i):
    P, GT, Fo = synthetic.split_clip(_clips(i), K, T, F)
    env.train()
    env.train_step(P, Fo, GT)


def _wino_tagged(generator):
    return [n for n, p in generator.named_parameters() if any(t[0].startswith('wino') for t in getattr(p, '_tai_derived', {}))]


def _assert_forward_is_the_fresh_generators(env, i, train, what):
    """The environment's forward on clips ``i`` against a generator made by create_model, loaded from the environment's current
    weights, on the same device and under the same routes: every output, bit for bit."""
    P, GT, Fo = synthetic.split_clip(_clips(i), K, T, F)
    if train:
        env.set_train_inputs(P, Fo, GT)
        env.train()
        env.forward_train()
    else:
        env.set_test_inputs(P, Fo)
        env.eval()
        env.forward_test()
    got = {k: v.detach().clone() for k, v in env.gen_output.items() if torch.is_tensor(v)}
    assert set(KEYS) <= set(got)
    assert _wino_tagged(env.generator), 'no generator weight carries a Winograd form: the comparison would be vacuous'
    fresh = vfi.create_model(MODEL).to(DEV)
    fresh.load_state_dict(env.generator.state_dict())
    fresh.train(train)
    with torch.set_grad_enabled(train):
        want = fresh(T, env.preceding_frames, env.following_frames)
    for k in got:
        assert torch.equal(got[k], want[k].detach()), '%s: %s differs from the fresh generator\'s by %.3g (max %.3g)' % (
            what, k, dc.max_abs(got[k] - want[k].detach()), dc.max_abs(want[k]))


@pytest.mark.parametrize('mode', ['fused_step_ema', 'fused_step', 'optimizer_step'])
def test_the_forward_after_an_update_is_computed_from_the_current_weights(mode, tmp_path, monkeypatch):
    """``optimizer_step`` is the control: torch.optim.Adam moves the version counters.  The fused step writes through raw pointers."""
    monkeypatch.setattr(conv_ops, 'WINO_MIN_WORKGROUPS', 0)
    env = _env(tmp_path, mode, fused_step=mode != 'optimizer_step', ema_decay=0.9 if mode == 'fused_step_ema' else None)
    before = [p.detach().clone() for p in env.generator.parameters()]
    for update in (1, 2):
        _update(env, update - 1)
        env.sync_guard()
        _assert_forward_is_the_fresh_generators(env, update, True, '%s, after update %d' % (mode, update))
    assert sum(not torch.equal(a, p.detach()) for a, p in zip(before, env.generator.parameters())) > 20


def test_the_forward_after_validation_and_the_next_fused_update(tmp_path, monkeypatch):
    """Validation exchanges p.data with the average and bumps the epoch on the way in and out; the update after it steps through raw
    pointers again: the forward after each is the fresh generator's."""
    monkeypatch.setattr(conv_ops, 'WINO_MIN_WORKGROUPS', 0)
    env = _env(tmp_path, 'val', fused_step=True, ema_decay=0.9)
    _update(env, 0)
    opt = TrainOptions().parse(['--K', str(K), '--T', str(T), '--F', str(F), '--model_key', 'x', '--c_dim', '1', '--image_size', str(SIZE),
                                '--batch_size', str(B), '--val_synthetic', '2', '--name', 'val', '--checkpoints_dir', str(tmp_path / 'ckpt')])
    lines = []
    validation.Validator(opt, start_best=(-1e9, -1e9)).validate(env, 1, log=lines.append)
    assert any(l.endswith(' weights=ema') for l in lines), lines
    _assert_forward_is_the_fresh_generators(env, 1, True, 'after validation')
    _update(env, 1)
    _assert_forward_is_the_fresh_generators(env, 2, True, 'after validation and the next update')
    _assert_forward_is_the_fresh_generators(env, 2, False, 'after validation and the next update, forward_test')


def test_the_forward_after_a_replayed_update(tmp_path, monkeypatch):
    """A replayed update recomputes the derived weights before its optimizer steps and moves no version counter; train_step drops
    them all after the replay.  The eager forward after the capture caches forms under the version the capture left behind (the
    capturing call ran Adam's Python, which moved the counters): it is the forward after the NEXT replay, a pure replay, that would
    be served those forms."""
    monkeypatch.setattr(conv_ops, 'WINO_MIN_WORKGROUPS', 0)
    env = _env(tmp_path, 'graph', graph_step=True)
    for i in range(3):                                     # two eager updates, the capture with its first replay
        _update(env, i)
    assert [1 for v in env._step_graphs.values() if 'graph' in v] == [1]
    _assert_forward_is_the_fresh_generators(env, 0, False, 'after the captured update')
    for i in (3, 4):                                       # pure replays
        versions = [p._version for p in env.generator.parameters()]
        weights = [p.detach().clone() for p in env.generator.parameters()]
        _update(env, i)
        assert versions == [p._version for p in env.generator.parameters()]
        assert sum(not torch.equal(a, p.detach()) for a, p in zip(weights, env.generator.parameters())) > 20
        _assert_forward_is_the_fresh_generators(env, 0, False, 'after replay %d' % (i - 2))


def test_the_discriminator_keeps_no_derived_form_on_a_parameter(monkeypatch):
    """tai_sn_power_iteration rescales the discriminator's weights through raw pointers in every forward.  That is safe because its
    convolutions run from per-call tensors (w0, a clone, and w3, its space-to-depth form): whatever conv_ops caches, it caches on
    those, never on a Parameter."""
    from video_frame_inpainting_amd.sn_discriminator import SNDiscriminator
    from video_frame_inpainting_amd.util import weights_init
    monkeypatch.setattr(conv_ops, 'WINO_MIN_WORKGROUPS', 0)
    taken = []
    plain = conv_ops.wino_conv3x3_plain

    def counted(x, weight, transposed=False):
        y = plain(x, weight, transposed)
        if y is not None:
            taken.append((weight, dict(getattr(weight, '_tai_derived', {}))))
        return y
    monkeypatch.setattr(conv_ops, 'wino_conv3x3_plain', counted)
    torch.manual_seed(4)
    disc = SNDiscriminator((32, 32), 1, 3, 16, 3).to(DEV)
    disc.apply(weights_init)
    x = torch.randn(2, 5, 1, 32, 32, device=DEV)
    disc(x).pow(2).mean().backward()
    params = {id(p) for p in disc.parameters()}
    assert taken and all(cache for _, cache in taken)                   # the Winograd route ran, from cached forms ...
    assert not any(id(w) in params for w, _ in taken)                   # ... of tensors that are no Parameter
    for n, p in disc.named_parameters():
        assert p.grad is not None and not getattr(p, '_tai_derived', None), n


def test_a_graphed_eval_environment_follows_the_load_of_a_second_snapshot(tmp_path, monkeypatch):
    """use_graph=True: ``load`` drops the captured forwards and the derived weights; the output after it is a fresh environment's."""
    monkeypatch.setattr(conv_ops, 'WINO_MIN_WORKGROUPS', 0)
    os.makedirs(tmp_path / 'exp')
    for i, name in enumerate(('a.ckpt', 'b.ckpt')):
        torch.save({'generator': synthetic.seeded_init(vfi.create_model(MODEL), 30 + i).state_dict()}, tmp_path / 'exp' / name)
    P, _, Fo = synthetic.split_clip(_clips(0), K, T, F)

    def forward(env):
        env.set_test_inputs(P, Fo)
        env.T = T
        env.eval()
        env.forward_test()
        return {k: v.detach().clone() for k, v in env.gen_output.items() if torch.is_tensor(v)}
    env = create_eval_environment(vfi.create_model(MODEL), str(tmp_path), 'exp', 'a.ckpt', [0, 0], device=DEV, use_graph=True)
    first = forward(env)
    assert _wino_tagged(env.generator)
    env.load('b.ckpt')
    second = forward(env)
    again = forward(env)                                   # a replay of the graph captured after the load
    want = forward(create_eval_environment(vfi.create_model(MODEL), str(tmp_path), 'exp', 'b.ckpt', [0, 0], device=DEV, use_graph=True))
    for k in KEYS:
        assert torch.equal(second[k], want[k]) and torch.equal(again[k], want[k]), k
        assert not torch.equal(first[k], second[k]), k
