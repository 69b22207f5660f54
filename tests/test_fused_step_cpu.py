"""The fused optimizer step without a GPU (train.py --fused_step [--ema_decay d]): the host path against the numpy restatement bit for
bit, the scalar table, closeness to torch.optim.Adam inside a derived bound, the guard's verdicts / counters / give-up on the CPU
training environment against the unfused guard, the weight average, the refusals, two gloo ranks skipping together, exact resume over
three processes, snapshots moving between fused and unfused runs, and the library's new entry points."""
import ctypes
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_step_ref as ref  # noqa: E402

import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import _native, environments, fused_step, grad_guard, parallel, run_state, synthetic  # noqa: E402
from video_frame_inpainting_amd.environments import create_training_environment  # noqa: E402
from video_frame_inpainting_amd.options import TestOptions as PredictOptions, TrainOptions  # noqa: E402

K, T, F = 3, 2, 3
LR, B1, B2 = 1e-3, 0.5, 0.999
EPS = 2.0 ** -23


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- the definition

def _case(kind, n, seed):
    rng = np.random.RandomState(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    m = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    v = (rng.standard_normal(n) * 1e-2).astype(np.float32) ** 2
    if kind == 'zero_moments':
        m[:], v[:] = 0, 0
    elif kind == 'zero_grad':
        g[:] = 0
    elif kind == 'denormal':
        g = (rng.standard_normal(n) * 1e-42).astype(np.float32)
        m = (rng.standard_normal(n) * 1e-41).astype(np.float32)
        v = np.abs(rng.standard_normal(n) * 1e-44).astype(np.float32)
    elif kind == 'large':
        g = (rng.standard_normal(n) * np.exp2(rng.randint(60, 127, n).astype(np.float64))).astype(np.float32)
        g[~np.isfinite(g)] = np.float32(3e38)
    return p, g, m, v


@pytest.mark.parametrize('kind', ['random', 'zero_moments', 'zero_grad', 'denormal', 'large'])
def test_host_path_equals_the_restatement_bit_for_bit(kind):
    n = 20011
    for t, c, d, beta1 in ((1, 1.0, None, 0.5), (1, 0.37, 0.99, 0.5), (2, 1.0, 0.999, 0.9), (7, 0.0123, None, 0.9), (1000, 0.9999999, 0.5, 0.5)):
        if kind == 'zero_moments' and t != 1:
            continue
        p, g, m, v = _case(kind, n, 100 + t)
        e = None if d is None else (p + np.float32(0.01)).astype(np.float32)
        want = ref.step(p, g, m, v, e, c, t, LR, beta1, B2, d)
        step_size, bc2s = fused_step.scalar_table(LR, beta1, B2, t)
        k = fused_step.constants(beta1, B2, d)
        hp, hm, hv, he, hg = p.copy(), m.copy(), v.copy(), None if e is None else e.copy(), g.copy()
        fused_step.host_step(hp, hg, hm, hv, he, c, step_size[t - 1], bc2s[t - 1], k)
        assert np.array_equal(_bits(hg), _bits(g))                         # .grad is not written back
        for have, w in zip((hp, hm, hv), want[:3]):
            assert np.array_equal(_bits(have), _bits(w)), (kind, t)
        if d is not None:
            assert np.array_equal(_bits(he), _bits(want[3]))
        assert not np.array_equal(_bits(hm), _bits(m)) or kind == 'zero_grad' and not m.any()


def test_scalar_table_is_the_python_formulas_rounded_to_fp32():
    for lr, b1, b2 in ((1e-4, 0.5, 0.999), (1e-3, 0.9, 0.999)):
        step_size, bc2s = fused_step.scalar_table(lr, b1, b2, 3000)
        rs, rb = ref.scalars(lr, b1, b2, 3000)
        assert step_size.dtype == bc2s.dtype == np.float32
        assert np.array_equal(_bits(step_size), _bits(rs)) and np.array_equal(_bits(bc2s), _bits(rb))
        assert step_size[0] == np.float32(lr / (1 - b1)) and bc2s[4] == np.float32(math.sqrt(1 - b2 ** 5))
        k = fused_step.constants(b1, b2, 0.999)
        assert (k.w1, k.b2, k.w2, k.eps, k.wE) == (np.float32(1 - b1), np.float32(b2), np.float32(1 - b2), np.float32(1e-8),
                                                   np.float32(1 - 0.999))
        assert all(type(x) is np.float32 for x in k)


@pytest.mark.parametrize('beta1', [0.5, 0.9])
@pytest.mark.parametrize('t', [1, 2, 5, 100, 100000])
def test_close_to_torch_adam_inside_the_derived_bound(t, beta1):
    """Both sides evaluate the same expression with a handful of roundings each, and m' may be a cancellation, so the error of m enters p
    through step_size / s and not relative to |u| (u = step_size m' / s):
        |dm| <= 2 eps (|m| + |g|);  |dv| <= 4 eps v';  |dp| <= eps (2 (|p| + |u|) + 2 (step_size / s)(|m| + |g|) + 16 |u|),  eps = 2^-23."""
    n = 300000
    rng = np.random.RandomState(t + int(10 * beta1))
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * np.exp2(rng.randint(-20, 4, n).astype(np.float64))).astype(np.float32)
    if t == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m = (rng.standard_normal(n) * np.exp2(rng.randint(-20, 4, n).astype(np.float64))).astype(np.float32)
        v = ((rng.standard_normal(n) * np.exp2(rng.randint(-20, 4, n).astype(np.float64))) ** 2).astype(np.float32)
        w1 = 1 - beta1
        m[:n // 4] = (-g[:n // 4].astype(np.float64) * w1 / (1 - w1)).astype(np.float32)      # planted: m' = m + w1 (g - m) cancels
    param = torch.nn.Parameter(torch.from_numpy(p.copy()))
    param.grad = torch.from_numpy(g.copy())
    opt = torch.optim.Adam([param], lr=LR, betas=(beta1, B2), foreach=False)
    if t > 1:
        opt.state[param].update(step=torch.tensor(float(t - 1)), exp_avg=torch.from_numpy(m.copy()), exp_avg_sq=torch.from_numpy(v.copy()))
    opt.step()
    st = opt.state[param]
    assert float(st['step']) == t
    p1, m1, v1, _ = ref.step(p, g, m, v, None, 1.0, t, LR, beta1, B2)
    step_size, bc2s = ref.scalars(LR, beta1, B2, t)
    p64, g64, m64 = np.abs(p.astype(np.float64)), np.abs(g.astype(np.float64)), np.abs(m.astype(np.float64))
    s = np.sqrt(v1.astype(np.float64)) / float(bc2s[-1]) + 1e-8
    u = float(step_size[-1]) * np.abs(m1.astype(np.float64)) / s
    dm = np.abs(st['exp_avg'].numpy().astype(np.float64) - m1)
    dv = np.abs(st['exp_avg_sq'].numpy().astype(np.float64) - v1)
    dp = np.abs(param.detach().numpy().astype(np.float64) - p1)
    bound_m = 2 * EPS * (m64 + g64)
    bound_v = 4 * EPS * v1.astype(np.float64)
    bound_p = EPS * (2 * (p64 + u) + 2 * (float(step_size[-1]) / s) * (m64 + g64) + 16 * u)
    tiny = np.finfo(np.float32).tiny
    ratios = [float(np.max(d / np.maximum(b, tiny))) for d, b in ((dm, bound_m), (dv, bound_v), (dp, bound_p))]
    print('t = %d beta1 = %.1f: worst |dm|, |dv|, |dp| over their bounds: %.3f %.3f %.3f' % ((t, beta1) + tuple(ratios)))
    assert np.all(dm <= bound_m) and np.all(dv <= bound_v + 2.0 ** -149) and np.all(dp <= bound_p)


# ---------------------------------------------------------------------------------------------------------------- flags and refusals

BASE = ['--K', '2', '--T', '2', '--F', '2', '--model_key', 'TAI_gray']


def test_flags_parse_default_off():
    opt = TrainOptions().parse(BASE, require_gpu=False)
    assert opt.fused_step is False and opt.ema_decay is None
    opt = TrainOptions().parse(BASE + ['--fused_step', '--ema_decay', '0.999'], require_gpu=False)
    assert opt.fused_step is True and opt.ema_decay == 0.999
    opt = PredictOptions().parse(BASE + ['--qual_result_root', 'x'], require_gpu=False)
    assert opt.weights == 'raw'
    assert PredictOptions().parse(BASE + ['--qual_result_root', 'x', '--weights', 'ema'], require_gpu=False).weights == 'ema'


def _make(root, name, resumable=False, guard=None, seed=0, **kw):
    torch.manual_seed(seed)
    np.random.seed(seed)
    return create_training_environment(vfi.MCNetFillInModel(4, 1, 3), 1, str(root), name, K, T, F, [32, 32], 1.0, 0.02, LR, B1, 4, 2, 3,
                                       [0, 0], device='cpu', resumable=resumable, guard=guard, **kw)


def test_refusals_each_with_its_message(monkeypatch, tmp_path):
    import train
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)         # the option parser's own check; nothing else is reached
    monkeypatch.setattr(train, '_run', lambda *a, **k: pytest.fail('the run was started'))
    with pytest.raises(SystemExit) as e:
        train.main(BASE + ['--ema_decay', '0.99'])
    assert '--fused_step' in str(e.value) and e.value.code not in (0, None)
    for d in ('0', '1', '1.5', '-0.1'):
        with pytest.raises(SystemExit) as e:
            train.main(BASE + ['--fused_step', '--ema_decay', d])
        assert 'between 0 and 1' in str(e.value)
    with pytest.raises(SystemExit) as e:
        train.main(BASE + ['--fused_step', '--graph_step'])
    assert '--graph_step' in str(e.value) and '--fused_step' in str(e.value)
    with pytest.raises(ValueError, match='fused'):
        _make(tmp_path, 'x', graph_step=True, fused_step=True)
    with pytest.raises(ValueError, match='--fused_step'):
        _make(tmp_path, 'x', ema_decay=0.9)
    for d in (0.0, 1.0, 2.0):
        with pytest.raises(ValueError, match='between 0 and 1'):
            _make(tmp_path, 'x', fused_step=True, ema_decay=d)
    # predict.py --weights ema on a snapshot without the key: refused, naming the key and the file
    env = _make(tmp_path, 'plain')
    env.save('model_best.ckpt', 0, 0, 0)
    torch.manual_seed(0)
    with pytest.raises(RuntimeError) as e:
        environments.create_eval_environment(vfi.MCNetFillInModel(4, 1, 3), str(tmp_path), 'plain', 'model_best.ckpt', [0, 0], device='cpu',
                                             weights='ema')
    assert 'generator_ema' in str(e.value) and 'model_best.ckpt' in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- training environment (CPU)

_CLIPS = torch.from_numpy(synthetic.make_clips(6, K + T + F, 1, 32, 32, 77))


def _step(env, clips=None):
    clips = _CLIPS[:2] if clips is None else clips
    env.K, env.T, env.F = K, T, F
    env.train()
    env.train_step(clips[:, :K], clips[:, K + T:], clips[:, K:K + T])


def _plant(env, script):
    """``script[update] = (bad elements planted in the generator's gradients, ... in the discriminator's)`` between each backward pass and
    what follows it (the all-reduce is the hook: it runs between ``backward()`` and the step)."""
    env._update = 0

    def hook(which, module, reducer):
        inner = reducer.allreduce_

        def planted():
            counts = script.get(env._update, (0, 0))[which]
            grads = [p.grad for p in module.parameters() if p.grad is not None]
            if counts:
                grads[2].view(-1)[:counts] = float('nan')
                grads[5].view(-1)[:1] = float('inf')
            inner()
            env._update += which                                         # D closes the update
        reducer.allreduce_ = planted
    hook(0, env.generator, env._reducer_G)
    hook(1, env.discriminator, env._reducer_D)


def _train_state(env, d_weights=True):
    out = dict(('G.' + k, v.clone()) for k, v in env.generator.state_dict().items())
    if d_weights:
        out.update(('D.' + k, v.clone()) for k, v in env.discriminator.state_dict().items())
    for tag, opt in (('oG', env.optimizer_G), ('oD', env.optimizer_D)):
        for i, p in enumerate(opt.param_groups[0]['params']):
            out.update(('%s.%d.%s' % (tag, i, k), torch.as_tensor(v).clone()) for k, v in opt.state.get(p, {}).items())
    if env.fused is not None:
        out.update(('E.' + k, v.clone()) for k, v in env.fused.ema.items())
    return out


def _same(a, b, keys=None):
    keys = list(a) if keys is None else keys
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in keys)


def test_guarded_fused_environment_against_the_unfused_guard(tmp_path):
    script = {1: (3, 0), 2: (0, 2), 4: (1, 1), 5: (2, 0), 6: (0, 4)}      # updates 4, 5, 6 in a row: patience 3 gives up in update 6
    logs = {}
    for name, kw in (('unfused', {}), ('fused', dict(fused_step=True, ema_decay=0.9))):
        env = _make(tmp_path, name, guard=grad_guard.GradGuard(clip_grad_norm=1e-3, patience=3), **kw)
        _plant(env, script)
        log = []
        for update in range(8):
            torch.manual_seed(update)
            before = _train_state(env, d_weights=False)
            try:
                _step(env)
                gave_up = None
            except grad_guard.GuardGaveUp as e:
                gave_up = str(e)
            after = _train_state(env, d_weights=False)
            verdicts = (env.guard.verdict['G'], env.guard.verdict['D'])
            log.append((verdicts, env.guard.counters(), gave_up, env.guard.log_suffix().split('skipped=')[1]))
            if name == 'fused':
                groups = {tag: any(not torch.equal(before[k], after[k]) for k in before if k.startswith(tag)) for tag in ('G.', 'oG.', 'oD.', 'E.')}
                if update == 0:
                    assert set(after) > set(before)                         # (moments and EMA appear with the first step)
                elif update >= 7:                                           # gave up in update 6: nothing moves after it
                    assert gave_up and not any(groups.values()), (update, groups)
                else:
                    assert bool(gave_up) == (update == 6)                   # (its generator step was a healthy one and was made)
                    sk_G, sk_D = verdicts[0] == grad_guard.SKIPPED, verdicts[1] == grad_guard.SKIPPED
                    assert groups == {'G.': not sk_G, 'oG.': not sk_G, 'E.': not sk_G, 'oD.': not sk_D}, (update, groups)
        logs[name] = log
    for update, (a, b) in enumerate(zip(logs['unfused'][:7], logs['fused'][:7])):
        assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3], (update, a, b)
    assert logs['unfused'][6][2] is not None and logs['unfused'][6][2] == logs['fused'][6][2]
    assert all(l[2] is None for l in logs['unfused'][:6] + logs['fused'][:6])
    assert 'non-finite' in logs['fused'][6][2] and logs['fused'][7][2] == logs['fused'][6][2]
    assert logs['fused'][6][1] == {'skipped_G': 3, 'skipped_D': 3, 'consecutive': 3}
    # clipping happened (1e-3 is far below the norm of these gradients) and the verdicts said so
    assert logs['fused'][0][0] == (grad_guard.CLIPPED, grad_guard.CLIPPED) and logs['fused'][1][0][0] == grad_guard.SKIPPED


def test_fused_step_on_the_environment_equals_the_restatement_and_is_close_to_adam(tmp_path):
    """One update, same seeds: the fused environment's weights and moments are the restatement's applied to the unfused environment's
    gradients (which are the same bits: nothing has stepped yet), and its ``step`` tensors hold 1."""
    plain, fused = _make(tmp_path, 'p'), _make(tmp_path, 'f', fused_step=True, ema_decay=0.75)
    starts = [p.detach().clone() for p in fused.generator.parameters()]
    for e in (plain, fused):
        torch.manual_seed(1)
        _step(e)
    n_checked = 0
    for (name, pp), pf, p0 in zip(plain.generator.named_parameters(), fused.generator.parameters(), starts):
        if pp.grad is None:
            assert pf.grad is None and pf not in fused.optimizer_G.state and name not in fused.fused.ema and torch.equal(pf, p0)
            continue
        assert torch.equal(pp.grad, pf.grad)
        z = np.zeros(p0.numel(), np.float32)
        p1, m1, v1, e1 = ref.step(p0.numpy().reshape(-1), pf.grad.numpy().reshape(-1), z, z, p0.numpy().reshape(-1), 1.0, 1, LR, B1, B2, 0.75)
        st = fused.optimizer_G.state[pf]
        assert np.array_equal(_bits(pf.detach().numpy().reshape(-1)), _bits(p1))
        assert np.array_equal(_bits(st['exp_avg'].numpy().reshape(-1)), _bits(m1))
        assert np.array_equal(_bits(st['exp_avg_sq'].numpy().reshape(-1)), _bits(v1))
        assert np.array_equal(_bits(fused.fused.ema[name].numpy()), _bits(e1))
        assert st['step'].dtype == torch.float32 and st['step'].dim() == 0 and float(st['step']) == 1.0
        assert torch.allclose(pf, pp, rtol=0, atol=1e-6)
        n_checked += 1
    assert n_checked > 10


def test_ema_is_the_recurrence_over_the_recorded_weights_and_keys_only_with_the_flag(tmp_path):
    d = 0.8
    env = _make(tmp_path, 'ema', fused_step=True, ema_decay=d)
    start = {n: p.detach().clone() for n, p in env.generator.named_parameters()}
    recorded = []
    for update in range(4):
        _step(env, _CLIPS[update:update + 2])
        recorded.append({n: p.detach().clone() for n, p in env.generator.named_parameters()})
    assert env.fused.ema and all(p.grad is not None for n, p in env.generator.named_parameters() if n in env.fused.ema)
    assert set(env.fused.ema) == {n for n, p in env.generator.named_parameters() if p.grad is not None}
    for n, e in env.fused.ema.items():
        want = ref.ema_recurrence(start[n].numpy().reshape(-1), [r[n].numpy().reshape(-1) for r in recorded], d)
        assert e.dim() == 1 and e.dtype == torch.float32 and np.array_equal(_bits(e.numpy()), _bits(want)), n
    env.save('model_latest.ckpt', 4, 0, 0)
    snap = torch.load(str(tmp_path / 'ema' / 'model_latest.ckpt'), weights_only=False)
    today = {'updates', 'sum_avg_psnr_err', 'sum_avg_ssim_err', 'generator', 'optimizer_G', 'discriminator', 'optimizer_D'}
    assert set(snap) == today | {'generator_ema'}
    assert list(snap['generator_ema']) == list(snap['generator'])
    for k, v in snap['generator_ema'].items():
        assert v.shape == snap['generator'][k].shape
        assert torch.equal(v.reshape(-1), env.fused.ema[k]) if k in env.fused.ema else torch.equal(v, snap['generator'][k])
    assert any(not torch.equal(snap['generator_ema'][k], snap['generator'][k]) for k in env.fused.ema)
    # the eager optimizer's form of ``step``: a float32 scalar on the host
    assert all(st['step'].dtype == torch.float32 and st['step'].dim() == 0 and float(st['step']) == 4 for st in snap['optimizer_G']['state'].values())
    # a generator loaded from generator_ema is what predict.py --weights ema runs
    torch.manual_seed(0)
    ev = environments.create_eval_environment(vfi.MCNetFillInModel(4, 1, 3), str(tmp_path), 'ema', 'model_latest.ckpt', [0, 0], device='cpu',
                                              weights='ema')
    assert all(torch.equal(v, snap['generator_ema'][k]) for k, v in ev.generator.state_dict().items())
    for name, kw in (('nf', {}), ('f', dict(fused_step=True))):
        other = _make(tmp_path, name, **kw)
        _step(other)
        other.save('model_latest.ckpt', 1, 0, 0)
        assert set(torch.load(str(tmp_path / name / 'model_latest.ckpt'), weights_only=False)) == today
    # a non-finite average is not written over a snapshot
    guarded = _make(tmp_path, 'g', guard=grad_guard.GradGuard(), fused_step=True, ema_decay=d)
    _step(guarded)
    next(iter(guarded.fused.ema.values()))[0] = float('nan')
    with pytest.raises(environments.SnapshotRefused, match='generator_ema'):
        guarded.save('model_latest.ckpt', 1, 0, 0)


def test_validation_scores_the_average_and_puts_the_weights_back(tmp_path):
    env = _make(tmp_path, 'v', fused_step=True, ema_decay=0.5)
    for _ in range(2):
        _step(env)
    params = dict(env.generator.named_parameters())
    before = {n: (p.data_ptr(), p.detach().clone()) for n, p in params.items()}
    with fused_step.averaged_weights(env) as scored:
        assert scored.active
        for n, p in env.generator.named_parameters():
            assert p is params[n]                                          # the Parameter objects stay
            assert torch.equal(p.detach().reshape(-1), env.fused.ema[n]) if n in env.fused.ema else p.data_ptr() == before[n][0]
    assert all(p.data_ptr() == before[n][0] and torch.equal(p.detach(), before[n][1]) for n, p in env.generator.named_parameters())
    assert not fused_step.averaged_weights(_make(tmp_path, 'w', fused_step=True)).active


def test_snapshots_move_between_fused_and_unfused_runs(tmp_path):
    fused = _make(tmp_path, 'a', fused_step=True)
    for _ in range(2):
        _step(fused)
    fused.save('model_latest.ckpt', 2, 0, 0)
    onto = _make(tmp_path, 'a', seed=5)                                   # an unfused run continues a fused snapshot
    assert onto.start_update == 2 and _same(_train_state(fused), _train_state(onto))
    _step(onto)
    assert all(float(st['step']) == 3 for st in onto.optimizer_G.state.values())
    onto.save('model_latest.ckpt', 3, 0, 0)
    back = _make(tmp_path, 'a', seed=6, fused_step=True, ema_decay=0.9)   # ... and a fused run the unfused one's, the average starting there
    assert back.start_update == 3 and _same(_train_state(onto), _train_state(back))
    assert int(back.fused.rec[fused_step.R_T]) == 3 and int(back.fused.rec[fused_step.R_T + 1]) == 3
    weights = {n: p.detach().clone() for n, p in back.generator.named_parameters()}
    _step(back)
    assert all(float(st['step']) == 4 and st['step'].dtype == torch.float32 for st in back.optimizer_G.state.values())
    for n, e in back.fused.ema.items():
        p1 = dict(back.generator.named_parameters())[n].detach().numpy().reshape(-1)
        assert np.array_equal(_bits(e.numpy()), _bits(ref.ema_recurrence(weights[n].numpy().reshape(-1), [p1], 0.9)))


# ---------------------------------------------------------------------------------------------------------------- exact resume

FLAGS = dict(fused_step=True, ema_decay=0.9)


def _resume_leg(_, root, name, first, last, out):
    """Updates first + 1 ... last of the run ``name`` in a process of its own; starts from the snapshot if there is one."""
    env = _make(root, name, resumable=True, guard=grad_guard.GradGuard(clip_grad_norm=1e-3, patience=4), seed=first + 11, **FLAGS)
    order = np.random.RandomState(9)
    if first:
        assert env.exact_resume and env.start_update == first
        order.set_state(run_state.numpy_state(env.restored_data_state['order']))
    env.data_state_source = lambda: {'kind': 'synthetic', 'order': order.get_state()}
    _plant(env, {1: (2, 0)} if not first else {})                          # (the straight run's update 1 and the split run's: a skip)
    clipped = []
    for _u in range(first, last):
        clips = _CLIPS[order.randint(0, 6, 2)]
        _step(env, clips)
        clipped.append(env.guard.verdict['G'])
    env.save('model_latest.ckpt', last, 0, 0)
    torch.save({'state': _train_state(env), 'counters': env.guard.counters(), 'digest': run_state.digest(env), 'verdicts': clipped}, out)


def test_three_plus_three_updates_in_two_processes_equal_six_in_one(tmp_path):
    root = str(tmp_path)
    mp.spawn(_resume_leg, args=(root, 'straight', 0, 6, os.path.join(root, 'a.pt')), nprocs=1, join=True)
    mp.spawn(_resume_leg, args=(root, 'split', 0, 3, os.path.join(root, 'b.pt')), nprocs=1, join=True)
    mp.spawn(_resume_leg, args=(root, 'split', 3, 6, os.path.join(root, 'c.pt')), nprocs=1, join=True)
    a, c = torch.load(os.path.join(root, 'a.pt'), weights_only=False), torch.load(os.path.join(root, 'c.pt'), weights_only=False)
    assert a['verdicts'][:3] == [grad_guard.CLIPPED, grad_guard.SKIPPED, grad_guard.CLIPPED] and grad_guard.CLIPPED in c['verdicts']
    assert any(k.startswith('E.') for k in a['state']) and _same(a['state'], c['state'])
    assert a['counters'] == c['counters'] == {'skipped_G': 1, 'skipped_D': 0, 'consecutive': 0}
    assert a['digest'] == c['digest']
    sa = torch.load(os.path.join(root, 'straight', 'model_latest.ckpt'), weights_only=False)
    sc = torch.load(os.path.join(root, 'split', 'model_latest.ckpt'), weights_only=False)
    assert sa['run_state']['digest'] == sc['run_state']['digest'] == a['digest'] and sa['run_state']['version'] == 1
    assert sa['run_state']['ema'] == [k[2:] for k in a['state'] if k.startswith('E.')]
    # the digest of a run without the flags is the table of today: no entry is added
    plain = _make(tmp_path, 'plain', resumable=True)
    with_step = _make(tmp_path, 'fs', resumable=True, fused_step=True)
    assert run_state.digest(plain) == run_state.digest(with_step)
    assert 'ema' not in run_state.capture(with_step)


# ---------------------------------------------------------------------------------------------------------------- data parallel (gloo)

def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    parallel.init_from_env(backend='gloo')
    env = _make(out_dir, 'dp', guard=grad_guard.GradGuard(clip_grad_norm=1e-3, patience=3), seed=7 + rank, fused_step=True, ema_decay=0.9)
    env.sync_replicas()
    _plant(env, {1: (2, 0)} if rank == 1 else {})                          # rank 1 alone, before the all-reduce
    log = []
    for update in range(3):
        torch.manual_seed(40 + update)                                     # (the spectral-norm vectors are drawn in the first forward)
        before = _train_state(env, d_weights=False)
        _step(env, _CLIPS[2 * rank + update:2 * rank + update + 2])        # each rank trains on its own clips
        env.sync_guard(agree=True)
        after = _train_state(env, d_weights=False)
        log.append((env.guard.verdict['G'], env.guard.verdict['D'], env.guard.counters(),
                    any(not torch.equal(before[k], after[k]) for k in before if k[:2] in ('G.', 'oG', 'E.'))))
    torch.save({'log': log, 'state': _train_state(env)}, os.path.join(out_dir, 'rank%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_skip_together_and_end_identical(tmp_path):
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = torch.load(tmp_path / 'rank0.pt', weights_only=False), torch.load(tmp_path / 'rank1.pt', weights_only=False)
    assert a['log'] == b['log']
    assert [l[0] for l in a['log']] == [grad_guard.CLIPPED, grad_guard.SKIPPED, grad_guard.CLIPPED]
    assert [l[3] for l in a['log']] == [True, False, True]
    assert a['log'][2][2] == {'skipped_G': 1, 'skipped_D': 0, 'consecutive': 0}
    assert any(k.startswith('E.') for k in a['state']) and _same(a['state'], b['state'])


# ---------------------------------------------------------------------------------------------------------------- library

def test_header_declares_and_library_exports_the_entry_points():
    names = ['tai_fused_step', 'tai_fused_step_workspace_bytes', 'tai_step_verdict', 'tai_step_verdict_workspace_bytes']
    declared = _native.declared_symbols()
    assert all(n in declared for n in names)
    assert os.path.exists(_native.LIB_PATH)
    _native.verify(_native.LIB_PATH)
    L = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(L, n) for n in names)
    L.tai_sepconv_version.restype = ctypes.c_int
    assert L.tai_sepconv_version() >= 800
    L.tai_step_verdict_workspace_bytes.restype = ctypes.c_longlong
    assert L.tai_step_verdict_workspace_bytes() == 8 * fused_step.REC_WORDS
    L.tai_fused_step_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_longlong]
    L.tai_fused_step_workspace_bytes.restype = ctypes.c_longlong
    assert L.tai_fused_step_workspace_bytes(3, 10) == 0 and L.tai_fused_step_workspace_bytes(0, 10) < 0
    header = open(_native.HEADER).read()
    for line in ("m' = m + w1 * (g1 - m)", "v' = b2 * v + (w2 * g1) * g1", "s  = sqrt(v') / bc2s[t'] + eps", "p' = p - step_size[t'] * (m' / s)",
                 "e' = e + wE * (p' - e)"):
        assert line in header                                              # the definition is written down where the declaration is
    # the kernel's arithmetic is compiled as written: the only fused multiply-adds of the step kernels sit inside the compiler's
    # correctly rounded division and square root, and the kernels use no scratch memory
    asm_path = os.path.join(os.path.dirname(_native.HEADER), '..', 'build', 'sepconv_capi-hip-amdgcn-amd-amdhsa-gfx950.s')
    if os.path.exists(asm_path):
        from video_frame_inpainting_amd import _isa_check
        found = _isa_check.kernels(open(asm_path).read(), '_ZN5fstep13step_segments')
        assert len(found) == 2
        assert _isa_check.check_fused_step(open(asm_path).read()) == []
