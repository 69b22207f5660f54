"""train.py --fused_step --lr_schedule --warmup_updates --weight_decay on the GPU: ``tai_fused_step_decay`` through the C ABI against the
numpy restatement (tests/fused_step_decay_ref.py) bit for bit, every tensor between guard bands that must come back untouched, and
the training environment: a rate of zero, a run cut in two, and the derived weights after a decayed update."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_step_decay_ref as ref  # noqa: E402
import test_gpu_exact_resume as resume  # noqa: E402  (the reduced-width model of the GPU suite's training runs)

import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import _native, conv_ops, fused_step, grad_guard, run_state, synthetic, tai  # noqa: E402
from video_frame_inpainting_amd.environments import create_training_environment  # noqa: E402
from video_frame_inpainting_amd.fused_step import Schedule  # noqa: E402

pytestmark = pytest.mark.gpu

SPEC, K, T, F, SIZE = resume.SPEC, resume.K, resume.T, resume.F, resume.SIZE
DEV = 'cuda:0'
LR, B1, B2, WD, D = 1e-3, 0.5, 0.999, 0.1, 0.99
W, TABLE_LEN = 5, 40
SCHED = dict(kind='cosine', W=W, r=0.1, N=TABLE_LEN - 1)
# (elements, words behind a 16-byte boundary): one element; a short segment; a full aligned segment (the 16-byte path); a full segment and
# a one-element second one; two full segments and a tail; an empty entry; a full segment 4 bytes off (the 4-byte path on a full segment)
ENTRIES = ((1, 0), (16383, 0), (16384, 0), (16385, 0), (40000, 0), (0, 0), (16384, 1))
FLAGS = (1, 0, 1, 1, 0, 1, 0)                     # with its complement both paths see both values
BAND = 64
SENTINEL = np.float32(-123456.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _host_table(seed=3):
    rng = np.random.RandomState(seed)
    table = []
    for i, (n, _) in enumerate(ENTRIES):
        p = rng.standard_normal(n).astype(np.float32)
        g = (rng.standard_normal(n) * np.exp2(rng.randint(-30, 8, n).astype(np.float64))).astype(np.float32)
        m = (rng.standard_normal(n) * 1e-2).astype(np.float32)
        v = ((rng.standard_normal(n) * 1e-2) ** 2).astype(np.float32)
        if n > 100:
            g[:10], m[10:20], v[20:30], p[30:40] = 0, 0, 0, 0
            p[40:50], g[50:60] = 1e-42, 1e-42                              # denormals
        e = (p + np.float32(0.5)).astype(np.float32) if i % 3 != 1 else None
        table.append((p, g, m, v, e))
    return table


TABLE = _host_table()                                                      # shared, never written
_WANT = {}


def _want(tprime, c, flags):
    """The restatement's table after step t' under clip coefficient c, computed once per case."""
    key = (tprime, c, flags)
    if key not in _WANT:
        step_size, bc2s, decay = ref.scalars(LR, B1, B2, TABLE_LEN, wd=WD, **SCHED)
        out = []
        for (p, g, m, v, e), f in zip(TABLE, flags):
            p1, m1, v1, e1 = ref.step(p, g, m, v, e, c, step_size[tprime - 1], bc2s[tprime - 1], decay[tprime - 1] if f else None, B1, B2, D)
            out.append((p1, g, m1, v1, e1))
        _WANT[key] = out
    return _WANT[key]


class Banded(object):
    """A tensor between two bands of SENTINEL in one buffer; its data starts ``words`` 4-byte words behind a 16-byte boundary."""

    def __init__(self, values, words=0):
        n = values.size
        self.buf = torch.full((n + 2 * BAND + 8,), float(SENTINEL), device=DEV)
        self.first = BAND + words + (16 - self.buf.data_ptr() % 16) % 16 // 4
        self.t = self.buf[self.first:self.first + n]
        assert n == 0 or self.t.data_ptr() % 16 == 4 * words
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(values).reshape(-1)))

    def bands_untouched(self):
        host = self.buf.cpu().numpy()
        outside = np.concatenate([host[:self.first], host[self.first + self.t.numel():]])
        return bool(np.all(_bits(outside) == _bits([SENTINEL])[0]))


def _device_table(table, entries=ENTRIES):
    """-> rows of [p, g, m, v, e or None, step or None] as Banded; the step tensor is left out of every second entry."""
    out = []
    for i, ((p, g, m, v, e), (_, words)) in enumerate(zip(table, entries)):
        row = [Banded(x, words) for x in (p, g, m, v)]
        row.append(None if e is None else Banded(e, words))
        row.append(Banded(np.array([-1.0], np.float32)) if i % 2 == 0 else None)
        out.append(row)
    return out


def _record(verdict, c, tprime, which=0):
    rec = np.zeros(fused_step.REC_WORDS, np.int64)
    rec[fused_step.R_VERDICT + which] = verdict
    rec[fused_step.R_COEFF + which] = int(np.array([c], np.float32).view(np.uint32)[0])
    rec[fused_step.R_TPRIME + which] = tprime
    return torch.from_numpy(rec).to(DEV)


def _scalars():
    return torch.from_numpy(np.concatenate(fused_step.scheduled_table(LR, B1, B2, TABLE_LEN, Schedule('cosine', W, min_ratio=0.1), WD, TABLE_LEN - 1))).to(DEV)


def _launch(dev, flags, rec, scalars, which=0, blocks=0, entry='tai_fused_step_decay'):
    t = lambda b: None if b is None else b.t
    rows, n_segments = fused_step.step_rows([t(d[0]) for d in dev], [t(d[1]) for d in dev], [t(d[2]) for d in dev], [t(d[3]) for d in dev],
                                            [None if d[5] is None else d[5].t[0] for d in dev], [t(d[4]) for d in dev])
    k = fused_step.constants(B1, B2, D)
    table = torch.from_numpy(rows).to(DEV)
    consts = (float(k.w1), float(k.b2), float(k.w2), float(k.eps), float(k.wE))
    stream = torch.cuda.current_stream().cuda_stream
    if entry == 'tai_fused_step_decay':
        words = np.asarray(flags, np.int64)
        dev_flags = torch.from_numpy(words).to(DEV)
        rc = _native.lib().tai_fused_step_decay(table.data_ptr(), rows.ctypes.data, dev_flags.data_ptr(), words.ctypes.data, rows.shape[0], n_segments,
                                                scalars.data_ptr(), TABLE_LEN, *consts, rec.data_ptr(), which, blocks, None, stream)
    else:
        rc = _native.lib().tai_fused_step(table.data_ptr(), rows.ctypes.data, rows.shape[0], n_segments, scalars.data_ptr(), TABLE_LEN, *consts,
                                          rec.data_ptr(), which, 0, blocks, None, stream)
    _native.check(rc, entry)
    torch.cuda.synchronize()
    return n_segments


def _assert_table(dev, want, step_value, what=''):
    for i, (d, w) in enumerate(zip(dev, want)):
        for j, name in ((0, 'p'), (1, 'g'), (2, 'm'), (3, 'v'), (4, 'e')):
            if d[j] is not None:
                assert np.array_equal(_bits(d[j].t.cpu().numpy()), _bits(w[j])), '%s entry %d (%d elements): %s differs' % (what, i, d[0].t.numel(), name)
        if d[5] is not None:
            assert float(d[5].t[0]) == step_value
        assert all(b.bands_untouched() for b in d if b is not None), '%s entry %d: a guard band was written' % (what, i)


def test_decay_kernel_equals_the_restatement_at_every_path_verdict_and_step():
    scalars = _scalars()
    inverse = tuple(1 - f for f in FLAGS)
    for tprime in (1, W, W + 1, TABLE_LEN):
        for c, verdict in ((1.0, grad_guard.OK), (0.25, grad_guard.CLIPPED)):
            for flags in (FLAGS, inverse):
                want = _want(tprime, c, flags)
                for blocks in (1, 0):                                      # one workgroup strides over all segments; the library's choice
                    dev = _device_table(TABLE)
                    n_segments = _launch(dev, flags, _record(verdict, c, tprime), scalars, blocks=blocks)
                    assert n_segments == sum(-(-n // 16384) for n, _ in ENTRIES) == 9
                    _assert_table(dev, want, tprime, 't=%d c=%g blocks=%d' % (tprime, c, blocks))
    assert any(not np.array_equal(_bits(a[0]), _bits(b[0])) for a, b in zip(_want(W, 1.0, FLAGS), _want(W, 1.0, inverse)))     # the flag matters
    # the discriminator's slot of the record
    dev = _device_table(TABLE)
    _launch(dev, FLAGS, _record(grad_guard.CLIPPED, 0.25, W, which=1), scalars, which=1)
    _assert_table(dev, _want(W, 0.25, FLAGS), W, 'which=1')
    # repetition from equal state, and per entry without the other entries
    only = 3
    dev = _device_table(TABLE[only:only + 1], ENTRIES[only:only + 1])
    _launch(dev, FLAGS[only:only + 1], _record(grad_guard.OK, 1.0, W), scalars)
    _assert_table(dev, _want(W, 1.0, FLAGS)[only:only + 1], W, 'alone')


def test_a_skipped_verdict_moves_no_byte():
    scalars = _scalars()
    dev = _device_table(TABLE)
    for rec in (_record(grad_guard.SKIPPED, 0.5, 3), _record(grad_guard.OK, 1.0, 0), _record(grad_guard.OK, 1.0, TABLE_LEN + 1)):
        for blocks in (1, 0):
            _launch(dev, FLAGS, rec, scalars, blocks=blocks)
            _assert_table(dev, TABLE, -1.0, 'skipped')


def test_all_flags_zero_is_tai_fused_step_and_an_unflagged_nonfinite_p_stays_as_it_leaves_it():
    scalars = _scalars()                                                   # (its first two rows are tai_fused_step's [2][table_len])
    table = [tuple(None if x is None else x.copy() for x in row) for row in TABLE]
    for i in (1, 4, 6):                                                    # the entries FLAGS leaves unflagged: both paths
        table[i][0][100:104] = [np.inf, -np.inf, np.nan, -np.nan]
    for flags in ((0,) * len(FLAGS), FLAGS):
        a, b = _device_table(table), _device_table(table)
        _launch(a, flags, _record(grad_guard.OK, 1.0, W + 1), scalars)
        _launch(b, None, _record(grad_guard.OK, 1.0, W + 1), scalars, entry='tai_fused_step')
        for i, (da, db) in enumerate(zip(a, b)):
            for j in range(5):
                if da[j] is not None and (j not in (0, 4) or not flags[i]):        # (a flagged entry's p and its average differ)
                    assert torch.equal(da[j].t.view(torch.int32), db[j].t.view(torch.int32)), (flags, i, j)
            assert all(x.bands_untouched() for x in da if x is not None)
            if flags[i] and da[0].t.numel():
                assert not torch.equal(da[0].t.view(torch.int32), db[0].t.view(torch.int32))            # ... and the flagged ones decayed
    step_size, bc2s, _ = ref.scalars(LR, B1, B2, TABLE_LEN, wd=WD, **SCHED)
    p, g, m, v, e = table[6]
    want = ref.step(p, g, m, v, e, 1.0, step_size[W], bc2s[W], None, B1, B2, D)[0]
    assert np.array_equal(_bits(a[6][0].t.cpu().numpy()), _bits(want)) and np.isnan(want[102]) and np.isinf(want[100])


def test_a_bad_flag_word_is_refused_before_launching():
    scalars = _scalars()
    dev = _device_table(TABLE)
    for bad in (2, 3, -1):
        with pytest.raises(RuntimeError, match='flag word must be 0 or 1'):
            _launch(dev, (1, 0, bad, 0, 0, 0, 0), _record(grad_guard.OK, 1.0, 1), scalars)
    torch.cuda.synchronize()
    _assert_table(dev, TABLE, -1.0, 'refused')


# ---------------------------------------------------------------------------------------------------------------- the training environment

@pytest.fixture
def reproducible():
    previous = (tai.set_reproducible_backward(True), torch.backends.cudnn.deterministic)
    torch.backends.cudnn.deterministic = True
    yield
    tai.set_reproducible_backward(previous[0])
    torch.backends.cudnn.deterministic = previous[1]


def _env(tmp_path, name, guard=None, seed=0, **kw):
    torch.manual_seed(seed)
    np.random.seed(seed)
    return create_training_environment(vfi.create_model(SPEC), 1, str(tmp_path / 'ckpt'), name, K, T, F, [SIZE, SIZE], 1.0, 0.02, 1e-4, B1, 8,
                                       3, 3, [0, 0], device=DEV, guard=guard, **kw)


_CLIPS = torch.from_numpy(synthetic.make_clips(6, K + T + F, 1, SIZE, SIZE, 1002))


def _update(env, clips):
    env.K, env.T, env.F = K, T, F
    env.train()
    env.train_step(clips[:, :K], clips[:, K + T:], clips[:, K:K + T])


def _generator_state(env):
    st = env.optimizer_G.state
    return {n: (p.detach().clone(), st[p]['exp_avg'].clone()) for n, p in env.generator.named_parameters() if p in st and len(st[p])}


def test_with_a_rate_of_zero_the_weights_stand_still_and_the_moments_move(tmp_path, reproducible, monkeypatch):
    launched = []
    real = _native.launch
    monkeypatch.setattr(_native, 'launch', lambda name, *a: (launched.append(name), real(name, *a))[1])
    env = _env(tmp_path, 'zero', fused_step=True, max_iter=10, lr_schedule=Schedule('step', 0, 1, 0.0), weight_decay=1e-2)
    states = []
    for update in range(3):
        _update(env, _CLIPS[update:update + 2])
        states.append(_generator_state(env))
    steps = [n for n in launched if n.startswith('tai_fused_step')]
    assert steps == ['tai_fused_step_decay', 'tai_fused_step'] * 3         # the generator decays, the discriminator never does
    assert len(states[0]) > 20
    for name in states[0]:
        assert torch.equal(states[1][name][0], states[0][name][0]) and torch.equal(states[2][name][0], states[0][name][0]), name
    assert any(not torch.equal(states[1][n][1], states[0][n][1]) for n in states[0])
    assert any(not torch.equal(states[2][n][1], states[1][n][1]) for n in states[0])
    assert all(float(st['step']) == 3 for st in env.optimizer_G.state.values())
    env.sync_guard()
    assert env.fused.rates_suffix() == ' lr_G=0 lr_D=0'
    # every new flag at its default: today's launches
    del launched[:]
    plain = _env(tmp_path, 'plain', fused_step=True, max_iter=10, lr_D=None, lr_schedule=None, weight_decay=0.0)
    _update(plain, _CLIPS[:2])
    assert [n for n in launched if n.startswith(('tai_fused_step', 'tai_step_verdict'))] == ['tai_step_verdict', 'tai_fused_step'] * 2
    assert plain.fused.rates_suffix() == '' and plain.fused._opt['G'].scalars.numel() == 2 * plain.fused.table_len


RUN = dict(fused_step=True, ema_decay=0.99, max_iter=6, lr_schedule=Schedule('cosine', 2, min_ratio=0.05), weight_decay=1e-2, lr_D=5e-5)


def _leg(tmp_path, name, first, last):
    env = _env(tmp_path, name, grad_guard.GradGuard(clip_grad_norm=1.0, patience=4), seed=first + 11, resumable=True, **RUN)
    order = np.random.RandomState(9)
    if first:
        assert env.exact_resume and env.start_update == first
        order.set_state(run_state.numpy_state(env.restored_data_state['order']))
    env.data_state_source = lambda: {'kind': 'synthetic', 'order': order.get_state()}
    for _u in range(first, last):
        _update(env, _CLIPS[order.randint(0, 6, 2)])
    env.save('model_latest.ckpt', last, 0, 0)
    return env


def test_three_plus_three_updates_equal_six_with_the_flags_on(tmp_path, reproducible):
    straight = _leg(tmp_path, 'straight', 0, 6)
    _leg(tmp_path, 'split', 0, 3)
    split = _leg(tmp_path, 'split', 3, 6)
    assert run_state.digest(straight) == run_state.digest(split)
    for a, b in zip(straight.generator.parameters(), split.generator.parameters()):
        assert torch.equal(a, b)
    assert all(torch.equal(straight.fused.ema[n], split.fused.ema[n]) for n in straight.fused.ema) and straight.fused.ema
    assert straight.fused.rates_suffix() == split.fused.rates_suffix() and 'lr_G=' in split.fused.rates_suffix()
    assert all(float(st['step']) == 6 for st in split.optimizer_G.state.values())
    with pytest.raises(ValueError, match='--max_iter 8'):
        _env(tmp_path, 'split', grad_guard.GradGuard(clip_grad_norm=1.0, patience=4), resumable=True, **dict(RUN, max_iter=8))


def test_the_forward_after_a_decayed_update_is_a_fresh_generators(tmp_path, reproducible):
    env = _env(tmp_path, 'fresh', fused_step=True, max_iter=10, lr_schedule=Schedule('cosine', 2), weight_decay=0.05)
    clips = _CLIPS[:2].to(DEV)

    def forward(model):
        model.eval()
        with torch.no_grad():
            return model(T, clips[:, :K], clips[:, K + T:])['pred'].clone()
    before = forward(env.generator)                                        # (the derived forms of the weights exist from here on)
    for update in range(2):
        _update(env, _CLIPS[update:update + 2])
    after = forward(env.generator)
    torch.manual_seed(5)
    fresh = vfi.create_model(SPEC).to(DEV)
    fresh.load_state_dict(env.generator.state_dict())
    conv_ops.invalidate_derived(fresh)
    assert torch.equal(after, forward(fresh)) and not torch.equal(after, before)
