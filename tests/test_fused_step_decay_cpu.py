"""The learning-rate schedule, the warm-up and the decoupled weight decay of the fused step without a GPU (train.py --fused_step
--lr_schedule --warmup_updates --lr_decay_every --lr_gamma --lr_min_ratio --weight_decay, --lr_D): the scheduled table and the host
step against the numpy restatement bit for bit, closeness to torch.optim.AdamW inside a derived bound, the CPU training environment
driven by its recorded gradients, the flags and their refusals, exact resume, and the library's new entry points."""
import ctypes
import itertools
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_step_decay_ref as ref  # noqa: E402
import fused_step_ref as plain_ref  # noqa: E402

import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import _isa_check, _native, fused_step, grad_guard, run_state, synthetic  # noqa: E402
from video_frame_inpainting_amd.environments import create_training_environment  # noqa: E402
from video_frame_inpainting_amd.fused_step import Schedule  # noqa: E402
from video_frame_inpainting_amd.options import TrainOptions  # noqa: E402

K = T = F = 2
LR, B1, B2 = 1e-3, 0.5, 0.999
EPS = 2.0 ** -23


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- the schedule's table

def test_scheduled_table_equals_the_restatement_bit_for_bit():
    for kind, W, N, E, g, r in itertools.product(fused_step.SCHEDULES, (0, 1, 7), (10, 3000), (1, 4), (0.0, 0.5), (0.0, 0.1, 1.0)):
        have = fused_step.scheduled_table(LR, B1, B2, N + 1, Schedule(kind, W, E, g, r), 1e-2, N)
        want = ref.scalars(LR, B1, B2, N + 1, wd=1e-2, kind=kind, W=W, E=E, g=g, r=r, N=N)
        for h, w in zip(have, want):
            assert h.dtype == np.float32 and np.array_equal(_bits(h), _bits(w)), (kind, W, N, E, g, r)


def test_neutral_settings_are_the_scalar_table_and_spot_values_are_the_formulas():
    for lr, b1 in ((1e-4, 0.5), (1e-3, 0.9)):
        step_size, bc2s, decay = fused_step.scheduled_table(lr, b1, B2, 3000)
        s0, b0 = fused_step.scalar_table(lr, b1, B2, 3000)
        assert np.array_equal(_bits(step_size), _bits(s0)) and np.array_equal(_bits(bc2s), _bits(b0)) and not decay.any()
    L, W, N, r, wd = 2e-4, 7, 50, 0.1, 1e-2
    step_size, _, decay = fused_step.scheduled_table(L, B1, B2, N, Schedule('cosine', W, min_ratio=r), wd, N)
    assert step_size[0] == np.float32((L / W) / (1 - B1))                          # t' = 1 under a warm-up
    assert step_size[W - 1] == np.float32(L / (1 - B1 ** W))                       # t' = W: the base rate
    assert step_size[N - 1] == np.float32(L * r / (1 - B1 ** N))                   # the cosine's last element (cos(pi) == -1.0 exactly)
    for t in (1, W, W + 1, 30, N):
        assert decay[t - 1] == np.float32(ref.lr(t, L, kind='cosine', W=W, r=r, N=N) * wd)
    mid = W + (N - W) // 2
    u = (mid - W) / (N - W)
    assert step_size[mid - 1] == np.float32((L * (r + (1 - r) * (0.5 * (1 + math.cos(math.pi * u))))) / (1 - B1 ** mid))
    stepped, _, _ = fused_step.scheduled_table(L, B1, B2, 20, Schedule('step', 0, 4, 0.5))
    assert [stepped[t - 1] for t in (4, 5, 9)] == [np.float32(L / (1 - B1 ** 4)), np.float32(L * 0.5 / (1 - B1 ** 5)),
                                                   np.float32(L * 0.25 / (1 - B1 ** 9))]
    rates = fused_step.learning_rates(L, 20, Schedule('step', 0, 1, 0.0))
    assert rates[0] == L and not any(rates[1:])                                    # 0 ** 0 == 1, then 0


# ---------------------------------------------------------------------------------------------------------------- the host step

def _case(kind, n, seed):
    rng = np.random.RandomState(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    m = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    v = (rng.standard_normal(n) * 1e-2).astype(np.float32) ** 2
    if kind == 'denormal':
        p = (rng.standard_normal(n) * 1e-40).astype(np.float32)
        g = (rng.standard_normal(n) * 1e-42).astype(np.float32)
        m = (rng.standard_normal(n) * 1e-41).astype(np.float32)
        v = np.abs(rng.standard_normal(n) * 1e-44).astype(np.float32)
    elif kind == 'zeros':
        p[::3], g[::5], m[::7], v[::7] = 0, 0, 0, 0
    elif kind == 'nonfinite_p':
        p[:4] = [np.inf, -np.inf, np.nan, 1.0]
    return p, g, m, v


@pytest.mark.parametrize('kind', ['random', 'denormal', 'zeros', 'nonfinite_p'])
def test_host_step_with_decay_equals_the_restatement_bit_for_bit(kind):
    n = 20011
    sched = dict(kind='cosine', W=3, r=0.05, N=40)
    step_size, bc2s, decay = fused_step.scheduled_table(LR, B1, B2, 41, Schedule('cosine', 3, min_ratio=0.05), 0.05, 40)
    for t, c, d, flagged in ((1, 1.0, None, True), (3, 0.37, 0.99, True), (4, 1.0, 0.999, False), (20, 0.0123, None, True), (41, 1.0, 0.5, True)):
        if kind == 'nonfinite_p' and flagged:
            continue                                                       # (a non-finite p belongs to the unflagged entries here)
        p, g, m, v = _case(kind, n, 100 + t)
        e = None if d is None else (p + np.float32(0.01)).astype(np.float32)
        rs, rb, rd = ref.scalars(LR, B1, B2, 41, wd=0.05, **sched)
        want = ref.step(p, g, m, v, e, c, rs[t - 1], rb[t - 1], rd[t - 1] if flagged else None, B1, B2, d)
        k = fused_step.constants(B1, B2, d)
        hp, hm, hv, he, hg = p.copy(), m.copy(), v.copy(), None if e is None else e.copy(), g.copy()
        fused_step.host_step(hp, hg, hm, hv, he, c, step_size[t - 1], bc2s[t - 1], k, decay[t - 1] if flagged else None)
        assert np.array_equal(_bits(hg), _bits(g))
        for have, w in zip((hp, hm, hv), want[:3]):
            assert np.array_equal(_bits(have), _bits(w)), (kind, t)
        if d is not None:
            assert np.array_equal(_bits(he), _bits(want[3]))
        if not flagged:                                                    # ... and it is the step without the decay line
            old = plain_ref.step(p, g, m, v, e, c, t, ref.lr(t, LR, **sched), B1, B2, d)
            assert np.array_equal(_bits(hp), _bits(old[0]))
        elif kind == 'random':
            assert not np.array_equal(_bits(hp), _bits(ref.step(p, g, m, v, e, c, rs[t - 1], rb[t - 1], None, B1, B2, d)[0]))


def test_a_flagged_entry_with_decay_zero_is_the_unflagged_one():
    p, g, m, v = _case('random', 5000, 3)
    step_size, bc2s, decay = fused_step.scheduled_table(LR, B1, B2, 5, Schedule('step', 0, 1, 0.0), 0.1)
    assert decay[0] > 0 and decay[1] == 0 and step_size[1] == 0
    k = fused_step.constants(B1, B2)
    for t in (1, 2):
        a, b = [x.copy() for x in (p, m, v)], [x.copy() for x in (p, m, v)]
        fused_step.host_step(a[0], g, a[1], a[2], None, 1.0, np.float32(1e-3), bc2s[t - 1], k, decay[t - 1])
        fused_step.host_step(b[0], g, b[1], b[2], None, 1.0, np.float32(1e-3), bc2s[t - 1], k, None)
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[1:], b[1:]))
        assert np.array_equal(_bits(a[0]), _bits(b[0])) == (t == 2)


# ---------------------------------------------------------------------------------------------------------------- closeness to AdamW

@pytest.mark.parametrize('beta1', [0.5, 0.9])
def test_close_to_torch_adamw_inside_the_derived_bound(beta1):
    """50 steps under a warm-up and a cosine with the same lr(t') set on torch's group before each step.  The bound is for ONE step from
    equal state, so each step starts torch.optim.AdamW from the restatement's state; it is the bound of
    test_fused_step_cpu.test_close_to_torch_adam_inside_the_derived_bound,
        |dm| <= 2 eps (|m| + |g|);  |dv| <= 4 eps v';  |dp| <= eps (2 (|p| + |u|) + 2 (step_size / s)(|m| + |g|) + 16 |u|),  eps = 2^-23,
    plus the decay line's own rounding.  torch multiplies p by f32(1 - a) (a = lr wd; relative error 2^-24, one rounded product: half
    an ulp), the definition subtracts the rounded product f32(a) p (relative errors 2^-24 each, of a term a |p|) from p (half an ulp):
    |p (1 - a) - (p - a p)| <= eps |p| (0.5 + 0.5 + 0.5 + 2 a) = 1.5 ulp of p and a term of relative size a; |p1| <= |p|, so the Adam
    part's bound stands with |p|.  The worst ratios and the free-running distance after the 50 steps are printed."""
    n, steps, wd, L = 100000, 50, 1e-2, 1e-3
    sched = dict(kind='cosine', W=5, r=0.01, N=steps)
    rng = np.random.RandomState(int(10 * beta1))
    p = rng.standard_normal(n).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    step_size, bc2s, decay = ref.scalars(L, beta1, B2, steps, wd=wd, **sched)
    param = torch.nn.Parameter(torch.from_numpy(p.copy()))
    free = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.AdamW([param], lr=L, betas=(beta1, B2), weight_decay=wd, foreach=False)
    opt_free = torch.optim.AdamW([free], lr=L, betas=(beta1, B2), weight_decay=wd, foreach=False)
    worst = [0.0, 0.0, 0.0]
    tiny = np.finfo(np.float32).tiny
    for t in range(1, steps + 1):
        g = (rng.standard_normal(n) * np.exp2(rng.randint(-20, 4, n).astype(np.float64))).astype(np.float32)
        rate = ref.lr(t, L, **sched)
        for o, q in ((opt, param), (opt_free, free)):
            o.param_groups[0]['lr'] = rate
            q.grad = torch.from_numpy(g.copy())
        with torch.no_grad():
            param.copy_(torch.from_numpy(p))
        if t > 1:
            opt.state[param].update(step=torch.tensor(float(t - 1)), exp_avg=torch.from_numpy(m.copy()), exp_avg_sq=torch.from_numpy(v.copy()))
        opt.step()
        opt_free.step()
        p1, m1, v1, _ = ref.step(p, g, m, v, None, 1.0, step_size[t - 1], bc2s[t - 1], decay[t - 1], beta1, B2)
        st = opt.state[param]
        assert float(st['step']) == t
        p64, g64, m64 = np.abs(p.astype(np.float64)), np.abs(g.astype(np.float64)), np.abs(m.astype(np.float64))
        s = np.sqrt(v1.astype(np.float64)) / float(bc2s[t - 1]) + 1e-8
        u = float(step_size[t - 1]) * np.abs(m1.astype(np.float64)) / s
        dm = np.abs(st['exp_avg'].numpy().astype(np.float64) - m1)
        dv = np.abs(st['exp_avg_sq'].numpy().astype(np.float64) - v1)
        dp = np.abs(param.detach().numpy().astype(np.float64) - p1)
        bound_m = 2 * EPS * (m64 + g64)
        bound_v = 4 * EPS * v1.astype(np.float64)
        bound_p = EPS * (2 * (p64 + u) + 2 * (float(step_size[t - 1]) / s) * (m64 + g64) + 16 * u) + EPS * p64 * (1.5 + 2 * rate * wd)
        worst = [max(w, float(np.max(d / np.maximum(b, tiny)))) for w, d, b in zip(worst, (dm, dv, dp), (bound_m, bound_v, bound_p))]
        assert np.all(dm <= bound_m) and np.all(dv <= bound_v + 2.0 ** -149) and np.all(dp <= bound_p), t
        p, m, v = p1, m1, v1
    drift = float(np.max(np.abs(free.detach().numpy().astype(np.float64) - p)))
    print('beta1 = %.1f, 50 steps: worst |dm|, |dv|, |dp| over their bounds: %.3f %.3f %.3f; free-running AdamW ends %.3g away (max abs)'
          % ((beta1,) + tuple(worst) + (drift,)))
    assert drift < 1e-4                                                    # (a sanity figure: the weights are of size 1 and moved by ~1e-2)


# ---------------------------------------------------------------------------------------------------------------- training environment (CPU)

_CLIPS = torch.from_numpy(synthetic.make_clips(6, K + T + F, 1, 32, 32, 77))
COSINE = Schedule('cosine', 2, min_ratio=0.01)


def _make(root, name, resumable=False, guard=None, seed=0, **kw):
    torch.manual_seed(seed)
    np.random.seed(seed)
    return create_training_environment(vfi.MCNetFillInModel(4, 1, 3), 1, str(root), name, K, T, F, [32, 32], 1.0, 0.02, LR, B1, 4, 2, 3,
                                       [0, 0], device='cpu', resumable=resumable, guard=guard, **kw)


def _step(env, clips=None):
    clips = _CLIPS[:2] if clips is None else clips
    env.K, env.T, env.F = K, T, F
    env.train()
    env.train_step(clips[:, :K], clips[:, K + T:], clips[:, K:K + T])


def _record(env):
    """-> log; log[update][which] = {name: (p, g)} as they stand between the backward pass and the step (the all-reduce is the hook)."""
    log = []

    def hook(which, module, reducer):
        inner = reducer.allreduce_

        def recording():
            inner()
            if which == 'G' or not log or 'D' in log[-1]:
                log.append({})
            log[-1][which] = {n: (p.detach().clone(), p.grad.detach().clone()) for n, p in module.named_parameters() if p.grad is not None}
        reducer.allreduce_ = recording
    hook('G', env.generator, env._reducer_G)
    hook('D', env.discriminator, env._reducer_D)
    return log


def _state(env, which):
    module, opt = (env.generator, env.optimizer_G) if which == 'G' else (env.discriminator, env.optimizer_D)
    return {n: (p.detach().clone(), opt.state[p]['exp_avg'].clone(), opt.state[p]['exp_avg_sq'].clone())
            for n, p in module.named_parameters() if p in opt.state and len(opt.state[p])}


def test_three_updates_equal_the_restatement_driven_by_the_recorded_gradients(tmp_path):
    N, wd, lr_D = 10, 1e-2, 3e-4
    env = _make(tmp_path, 'c', fused_step=True, max_iter=N, lr_schedule=COSINE, weight_decay=wd, lr_D=lr_D)
    log, after = _record(env), []
    for update in range(3):
        _step(env, _CLIPS[update:update + 2])
        after.append({w: _state(env, w) for w in 'GD'})
    assert len(log) == 3 and all(set(l) == {'G', 'D'} for l in log)
    sched = dict(kind='cosine', W=2, r=0.01, N=N)
    dims = {'G': {n: p.dim() for n, p in env.generator.named_parameters()}, 'D': {n: p.dim() for n, p in env.discriminator.named_parameters()}}
    checked = {'weights': 0, 'biases': 0, 'D': 0}
    for which, L in (('G', LR), ('D', lr_D)):
        step_size, bc2s, decay = ref.scalars(L, B1, B2, N + 1, wd=wd if which == 'G' else 0.0, **sched)
        for name in log[0][which]:
            z = np.zeros(log[0][which][name][0].numel(), np.float32)
            m, v = z, z
            decays = which == 'G' and dims[which][name] >= 2
            for t in range(1, 4):
                p, g = (x.numpy().reshape(-1) for x in log[t - 1][which][name])
                if which == 'G' and t > 1:                                 # nothing but the step writes the generator's weights
                    assert np.array_equal(_bits(p), _bits(after[t - 2]['G'][name][0].numpy().reshape(-1)))
                m0, v0 = m, v
                p1, m, v, _ = ref.step(p, g, m0, v0, None, 1.0, step_size[t - 1], bc2s[t - 1], decay[t - 1] if decays else None, B1, B2)
                have = [x.numpy().reshape(-1) for x in after[t - 1][which][name]]
                assert all(np.array_equal(_bits(h), _bits(w)) for h, w in zip(have, (p1, m, v))), (which, name, t)
                # a run with wd = 0 given the same gradients (the step without the line, tests/fused_step_ref.py): biases and every
                # discriminator parameter are its values; the weights are not
                old = plain_ref.step(p, g, m0, v0, None, 1.0, t, ref.lr(t, L, **sched), B1, B2)
                assert np.array_equal(_bits(have[0]), _bits(old[0])) == (not decays), (which, name, t)
            checked['D' if which == 'D' else ('weights' if decays else 'biases')] += 1
    assert min(checked.values()) >= 3, checked
    assert all(g['weight_decay'] == 0 for o in (env.optimizer_G, env.optimizer_D) for g in o.param_groups)
    assert all(float(st['step']) == 3 for st in env.optimizer_G.state.values() if len(st))
    env.sync_guard()
    assert env.fused.rates_suffix() == ' lr_G=%.6g lr_D=%.6g' % (ref.lr(3, LR, **sched), ref.lr(3, lr_D, **sched))


def test_with_a_rate_of_zero_the_weights_stand_still_and_the_moments_move(tmp_path):
    """step, E = 1, g = 0: lr(1) = L and lr(t') = 0 from t' = 2 -- the table is what steers the step."""
    env = _make(tmp_path, 'z', fused_step=True, max_iter=10, lr_schedule=Schedule('step', 0, 1, 0.0), weight_decay=1e-2)
    states = []
    for update in range(3):
        _step(env, _CLIPS[update:update + 2])
        states.append(_state(env, 'G'))
    assert len(states[0]) > 10
    for name in states[0]:
        assert torch.equal(states[1][name][0], states[0][name][0]) and torch.equal(states[2][name][0], states[0][name][0]), name
    assert any(not torch.equal(states[1][n][1], states[0][n][1]) for n in states[0])
    assert any(not torch.equal(states[2][n][1], states[1][n][1]) for n in states[0])
    env.sync_guard()
    assert env.fused.rates_suffix() == ' lr_G=0 lr_D=0'


# ---------------------------------------------------------------------------------------------------------------- flags and refusals

BASE = ['--K', '2', '--T', '2', '--F', '2', '--model_key', 'TAI_gray']


def test_flags_parse_with_defaults_off():
    opt = TrainOptions().parse(BASE, require_gpu=False)
    assert (opt.lr_D, opt.lr_schedule, opt.warmup_updates, opt.lr_min_ratio, opt.weight_decay) == (None, 'constant', 0, 0.01, 0.0)
    sc = Schedule(opt.lr_schedule, opt.warmup_updates, opt.lr_decay_every, opt.lr_gamma, opt.lr_min_ratio)
    sc.check()
    assert not sc.on and fused_step.needs_fused_step(sc, opt.weight_decay) is None
    opt = TrainOptions().parse(BASE + ['--fused_step', '--lr_D', '4e-4', '--lr_schedule', 'cosine', '--warmup_updates', '100', '--lr_min_ratio', '0.1',
                                       '--lr_decay_every', '7', '--lr_gamma', '0.3', '--weight_decay', '1e-4'], require_gpu=False)
    assert (opt.lr_D, opt.lr_schedule, opt.warmup_updates, opt.lr_min_ratio, opt.lr_decay_every, opt.lr_gamma, opt.weight_decay) == (
        4e-4, 'cosine', 100, 0.1, 7, 0.3, 1e-4)


def test_refusals_each_with_its_message(monkeypatch, tmp_path):
    import train
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)         # the option parser's own check; nothing else is reached
    started = []
    monkeypatch.setattr(train, '_run', lambda opt, stop: started.append(opt))
    for flags, flag in ((['--lr_schedule', 'cosine'], '--lr_schedule'), (['--lr_schedule', 'step'], '--lr_schedule'),
                        (['--warmup_updates', '5'], '--warmup_updates'), (['--weight_decay', '1e-4'], '--weight_decay')):
        with pytest.raises(SystemExit) as e:
            train.main(BASE + flags)
        assert flag in str(e.value) and '--fused_step' in str(e.value) and e.value.code not in (0, None)
    for flags, flag in ((['--warmup_updates', '-1'], '--warmup_updates'), (['--lr_decay_every', '0'], '--lr_decay_every'),
                        (['--lr_gamma', '1.5'], '--lr_gamma'), (['--lr_gamma', '-0.1'], '--lr_gamma'), (['--lr_min_ratio', '1.1'], '--lr_min_ratio'),
                        (['--lr_min_ratio', '-0.5'], '--lr_min_ratio'), (['--weight_decay=-1e-4'], '--weight_decay'),
                        (['--weight_decay', 'inf'], '--weight_decay'), (['--weight_decay', 'nan'], '--weight_decay')):
        with pytest.raises(SystemExit) as e:
            train.main(BASE + ['--fused_step'] + flags)
        assert flag in str(e.value) and e.value.code not in (0, None), flags
    assert not started
    train.main(BASE + ['--lr_D', '3e-4'])                                  # --lr_D alone needs no --fused_step
    assert len(started) == 1 and started[0].lr_D == 3e-4
    # the environment: the same words
    for kw, flag in ((dict(lr_schedule=COSINE), '--lr_schedule cosine'), (dict(lr_schedule=Schedule(warmup_updates=3)), '--warmup_updates'),
                     (dict(weight_decay=1e-3), '--weight_decay')):
        with pytest.raises(ValueError) as e:
            _make(tmp_path, 'x', **kw)
        assert flag in str(e.value) and '--fused_step' in str(e.value)
        assert str(e.value) == fused_step.needs_fused_step(kw.get('lr_schedule'), kw.get('weight_decay', 0.0))
    for kw, flag in ((dict(lr_schedule=Schedule(warmup_updates=-1)), '--warmup_updates'), (dict(lr_schedule=Schedule('step', 0, 0)), '--lr_decay_every'),
                     (dict(lr_schedule=Schedule('step', gamma=2.0)), '--lr_gamma'), (dict(lr_schedule=Schedule('cosine', min_ratio=-1.0)), '--lr_min_ratio'),
                     (dict(weight_decay=float('nan')), '--weight_decay'), (dict(weight_decay=-1.0), '--weight_decay')):
        with pytest.raises(ValueError, match=flag):
            _make(tmp_path, 'x', fused_step=True, **kw)
    plain = _make(tmp_path, 'd', lr_D=3e-4)                                # without the fused step: another number for the second optimizer
    assert plain.fused is None and plain.optimizer_D.param_groups[0]['lr'] == 3e-4 and plain.optimizer_G.param_groups[0]['lr'] == LR
    assert _make(tmp_path, 'e').optimizer_D.param_groups[0]['lr'] == LR


# ---------------------------------------------------------------------------------------------------------------- exact resume

FLAGS = dict(fused_step=True, ema_decay=0.99, lr_schedule=Schedule('cosine', 2, min_ratio=0.05), weight_decay=1e-2, lr_D=5e-4)


def _train_state(env):
    out = dict(('G.' + k, v.clone()) for k, v in env.generator.state_dict().items())
    out.update(('D.' + k, v.clone()) for k, v in env.discriminator.state_dict().items())
    for tag, opt in (('oG', env.optimizer_G), ('oD', env.optimizer_D)):
        for i, p in enumerate(opt.param_groups[0]['params']):
            out.update(('%s.%d.%s' % (tag, i, k), torch.as_tensor(v).clone()) for k, v in opt.state.get(p, {}).items())
    out.update(('E.' + k, v.clone()) for k, v in env.fused.ema.items())
    return out


def _resume_leg(_, root, name, first, last, out):
    env = _make(root, name, resumable=True, guard=grad_guard.GradGuard(clip_grad_norm=1.0, patience=4), seed=first + 11, max_iter=6, **FLAGS)
    order = np.random.RandomState(9)
    if first:
        assert env.exact_resume and env.start_update == first
        order.set_state(run_state.numpy_state(env.restored_data_state['order']))
    env.data_state_source = lambda: {'kind': 'synthetic', 'order': order.get_state()}
    for _u in range(first, last):
        _step(env, _CLIPS[order.randint(0, 6, 2)])
    env.save('model_latest.ckpt', last, 0, 0)
    torch.save({'state': _train_state(env), 'digest': run_state.digest(env), 'suffix': env.fused.rates_suffix()}, out)


def test_three_plus_three_updates_equal_six_and_other_settings_are_refused(tmp_path):
    root = str(tmp_path)
    mp.spawn(_resume_leg, args=(root, 'straight', 0, 6, os.path.join(root, 'a.pt')), nprocs=1, join=True)
    mp.spawn(_resume_leg, args=(root, 'split', 0, 3, os.path.join(root, 'b.pt')), nprocs=1, join=True)
    mp.spawn(_resume_leg, args=(root, 'split', 3, 6, os.path.join(root, 'c.pt')), nprocs=1, join=True)
    a, c = torch.load(os.path.join(root, 'a.pt'), weights_only=False), torch.load(os.path.join(root, 'c.pt'), weights_only=False)
    assert set(a['state']) == set(c['state']) and all(torch.equal(a['state'][k], c['state'][k]) for k in a['state'])
    assert a['digest'] == c['digest'] and a['suffix'] == c['suffix'] and 'lr_G=' in a['suffix']
    snap = torch.load(os.path.join(root, 'split', 'model_latest.ckpt'), weights_only=False)
    assert snap['run_state']['lr_schedule'] == {'lr': LR, 'lr_D': 5e-4, 'lr_schedule': 'cosine', 'warmup_updates': 2, 'lr_decay_every': 10000,
                                                'lr_gamma': 0.5, 'lr_min_ratio': 0.05, 'weight_decay': 1e-2, 'max_iter': 6}
    assert snap['run_state']['digest'] == a['digest']
    guard = lambda: grad_guard.GradGuard(clip_grad_norm=1.0, patience=4)
    for change, named in ((dict(max_iter=8), '--max_iter 8'), (dict(weight_decay=2e-2), '--weight_decay 0.02'),
                          (dict(lr_schedule=None, weight_decay=0.0), 'no schedule')):
        with pytest.raises(ValueError) as e:
            _make(root, 'split', resumable=True, guard=guard(), **dict(dict(FLAGS, max_iter=6), **change))
        assert named in str(e.value) and '--max_iter 6' in str(e.value) and '--weight_decay 0.01' in str(e.value), str(e.value)
    with pytest.raises(ValueError, match='--weight_decay 0.01'):
        _make(root, 'split', resumable=True, guard=guard())                # ... and a run without the fused step


def test_a_run_without_the_flags_saves_what_it_saved_before(tmp_path):
    plain = _make(tmp_path, 'plain', resumable=True, fused_step=True)
    only_d = _make(tmp_path, 'lrd', resumable=True, fused_step=True, lr_D=LR, lr_schedule=Schedule(), weight_decay=0.0)
    flagged = _make(tmp_path, 'fl', resumable=True, fused_step=True, max_iter=10, lr_schedule=COSINE)
    for env in (plain, only_d, flagged):
        torch.manual_seed(1)                                               # (the spectral-norm vectors are drawn in the first forward)
        _step(env)
    today = {'version', 'world_size', 'u', 'ktf', 'ranks', 'digest'}
    assert set(run_state.capture(plain)) == set(run_state.capture(only_d)) == today
    assert set(run_state.capture(flagged)) == today | {'lr_schedule'}
    assert run_state.digest(plain) == run_state.digest(only_d)             # the same state, the same digest: nothing enters the table
    a, b = _train_state(plain), _train_state(only_d)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert plain.fused.settings() is None and plain.fused.rates_suffix() == '' and plain.fused._opt['G'].decay is None
    plain.save('model_latest.ckpt', 1, 0, 0)
    snap = torch.load(str(tmp_path / 'plain' / 'model_latest.ckpt'), weights_only=False)
    assert set(snap) == {'updates', 'sum_avg_psnr_err', 'sum_avg_ssim_err', 'generator', 'optimizer_G', 'discriminator', 'optimizer_D', 'run_state'}
    assert set(snap['run_state']) == today


# ---------------------------------------------------------------------------------------------------------------- library

ASM = os.path.join(os.path.dirname(_native.HEADER), '..', 'build', 'sepconv_capi-hip-amdgcn-amd-amdhsa-gfx950.s')

_CHILD = r'''
import ctypes, json, sys
sys.path.insert(0, %r)
import importlib
_native = importlib.import_module('video-frame-inpainting_amd._native')
L = ctypes.CDLL(_native.LIB_PATH)
for name, (restype, argtypes) in _native.signatures().items():
    getattr(L, name).restype, getattr(L, name).argtypes = restype, argtypes
P = 16
i64 = lambda *v: (ctypes.c_longlong * len(v))(*v)
ROW = i64(16, 16, 16, 16, 16, 0, 4, 0)
def call(table=P, table_host=ROW, flags=P, flags_host=i64(1), n=1, segs=1, scalars=P, table_len=1, record=P, which=0, blocks=0):
    cast = lambda a: a if a is None or isinstance(a, int) else ctypes.cast(a, ctypes.c_void_p)
    rc = L.tai_fused_step_decay(cast(table), cast(table_host), cast(flags), cast(flags_host), n, segs, scalars, table_len, 0.5, 0.999, 0.001, 1e-8,
                                0.0, record, which, blocks, None, None)
    return [rc, L.tai_sepconv_last_error().decode()]
print(json.dumps({'null table': call(table=None), 'null flags': call(flags=None), 'flag 2': call(flags_host=i64(2)), 'flag -1': call(flags_host=i64(-1)),
                  'no entries': call(n=0), 'record': call(record=12), 'flags address': call(flags=12), 'segments': call(segs=2),
                  'row': call(table_host=i64(16, 16, 16, 0, 16, 0, 4, 0)), 'which': call(which=2), 'blocks': call(blocks=65537),
                  'table_len': call(table_len=0)}))
'''


def test_header_declares_and_library_exports_the_entry_points_and_they_refuse_without_a_device():
    names = ['tai_fused_step_decay', 'tai_fused_step_decay_workspace_bytes']
    assert all(n in _native.declared_symbols() for n in names)
    _native.verify(_native.LIB_PATH)
    L = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(L, n) for n in names)
    L.tai_sepconv_version.restype = ctypes.c_int
    assert L.tai_sepconv_version() >= 870
    L.tai_fused_step_decay_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_longlong]
    L.tai_fused_step_decay_workspace_bytes.restype = ctypes.c_longlong
    assert L.tai_fused_step_decay_workspace_bytes(3, 10) == 0 and L.tai_fused_step_decay_workspace_bytes(0, 10) < 0
    assert len(_native.signatures()['tai_fused_step_decay'][1]) == 18
    header = open(_native.HEADER).read()
    for line in ("p1 = p - (decay[t'] * p)", "p' = p1 - step_size[t'] * (m' / s)", "lr(t')    = (L * warm(t')) * s(t')",
                 "decay[t']     = f32(lr(t') * wd)", "s(t') = g ** ((t' - 1) // E)"):
        assert line in header
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, '-c', _CHILD % root], env=dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1'),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout)
    assert all(rc == -1 and msg.startswith('fused_step_decay: ') for rc, msg in got.values()), got
    assert 'null pointer' in got['null table'][1] and 'null pointer' in got['null flags'][1]
    assert 'flag word must be 0 or 1' in got['flag 2'][1] and got['flag -1'] == got['flag 2']
    assert 'n_entries > 0' in got['no entries'][1] and got['which'] == got['blocks'] == got['table_len'] == got['no entries']
    assert '8-byte aligned' in got['record'][1] and got['flags address'] == got['record']
    assert 'the table has 1 segments, not 2' in got['segments'][1] and 'row 0 is not' in got['row'][1]


def test_the_decay_kernel_is_compiled_as_written():
    asm = open(ASM).read()
    assert len(_isa_check.kernels(asm, '_ZN5fstep19step_segments_decay')) == 1
    assert len(_isa_check.kernels(asm, '_ZN5fstep13step_segments')) == 2                  # ... beside the two there were, not among them
    assert _isa_check.check_fused_step_decay(asm) == [] and _isa_check.check(asm) == []
    at = asm.index('\tv_div_fixup_f32', re.search(r'^_ZN5fstep19step_segments_decay\w*:', asm, re.M).start())
    doctored = asm[:at] + '\tv_fma_f32 v1, v2, v3, v4\n' + asm[at:]
    found = _isa_check.check_fused_step_decay(doctored)
    assert len(found) == 1 and 'fused multiply-adds' in found[0] and 'step_segments_decay' in found[0]
    assert any('step_segments_decay' in v for v in _isa_check.check(doctored))             # check() runs it
    assert _isa_check.check_fused_step(doctored) == []
    assert 'expected one' in _isa_check.check_fused_step_decay(asm.replace('_ZN5fstep19step_segments_decay', '_ZN5fstep19step_segments_gone'))[0]
