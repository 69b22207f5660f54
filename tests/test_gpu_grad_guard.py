"""train.py --guard on the GPU: tai_grad_stats / tai_grad_scale against the numpy restatement of their definition, the guarded update of
the training environment (clean, poisoned, clipped, a poisoned state, patience), and a clipped --resumable run cut in two against the
same run made in one.  Every comparison is bit equality or an exact integer unless stated.  NaN and Inf here are data in tensors."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_stats_ref as ref  # noqa: E402
import test_gpu_exact_resume as resume  # noqa: E402  (its helpers: the arguments of a reduced-width run, straight against split)

import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import environments, grad_guard, synthetic, tai  # noqa: E402
from video_frame_inpainting_amd.environments import create_training_environment  # noqa: E402

pytestmark = pytest.mark.gpu

SPEC, K, T, F, SIZE, DEV = resume.SPEC, resume.K, resume.T, resume.F, resume.SIZE, resume.DEV


# ---------------------------------------------------------------------------------------------------------------- the kernels

SIZES = (1, 3, 4, 5, 63, 64, 65, 16383, 16384, 16385, 1000003)


def _values(n, seed):
    """float32 over the whole range: normal draws times 2^-149 .. 2^127 (denormals, magnitudes whose square overflows fp32), +-0."""
    rng = np.random.RandomState(seed)
    with np.errstate(over='ignore'):
        x = (rng.standard_normal(n) * np.exp2(rng.randint(-149, 128, n).astype(np.float64))).astype(np.float32)
    x[~np.isfinite(x)] = np.float32(-3.0e38)
    x[rng.randint(0, n, max(1, n // 50))] = np.float32(0.0)
    x[rng.randint(0, n, max(1, n // 50))] = np.float32(-0.0)
    return x


def _table(seed=0, plant=True):
    table = [_values(n, seed + n) for n in SIZES]
    table.insert(5, np.zeros(0, np.float32))
    if plant:
        big = table[-1]
        big[[0, 4097, 16384, 500000, 1000002]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
        table[9][[100, 16383]] = [-np.inf, np.nan]                         # the entry of 16384 elements: one full segment
        table[4][62] = np.inf                                              # the entry of 63
    return table


def _on_device(table, behind=(1, 0)):
    """The same values on the GPU; entry i starts ``behind[i % len(behind)]`` words behind a 16-byte boundary."""
    out = []
    for i, a in enumerate(table):
        words = behind[i % len(behind)]
        buf = torch.empty(a.size + 8, device=DEV)
        first = (16 - buf.data_ptr() % 16) % 16 // 4 + words
        view = buf[first:first + a.size]
        assert a.size == 0 or view.data_ptr() % 16 == 4 * words
        view.copy_(torch.from_numpy(a))
        out.append(view)
    return out


def _bits64(values):
    return [float(v).hex() for v in values]


def _assert_equal(have, want):
    (sumsq, maxabs, bad), totals = have
    per, total = want
    assert _bits64(sumsq) == _bits64(p[0] for p in per)
    assert [np.float32(v).tobytes() for v in maxabs] == [np.float32(p[1]).tobytes() for p in per]
    assert [int(v) for v in bad] == [p[2] for p in per]
    assert float(totals[0]).hex() == float(total[0]).hex() and np.float32(totals[1]) == total[1] and totals[2] == total[2]


def test_grad_stats_kernel_equals_the_numpy_restatement():
    table = _table()
    want = ref.table_stats(table)
    assert want[1][2] == 8 and want[0][5] == (0.0, 0.0, 0) and np.isfinite(want[1][0])
    dev = _on_device(table)
    assert any(t.data_ptr() % 16 == 4 for t in dev if t.numel()) and any(t.numel() == 0 for t in dev)
    have = grad_guard.grad_stats(dev)
    print('total sumsq %r (restated %r), maxabs %r, nonfinite %d' % (have[1][0], float(want[1][0]), have[1][1], have[1][2]))
    _assert_equal(have, want)
    _assert_equal(grad_guard.grad_stats(dev), want)                                        # a second launch
    for behind in ((0,), (2, 3), (0, 1, 2, 3)):                                            # other addresses, other alignments
        _assert_equal(grad_guard.grad_stats(_on_device(table, behind)), want)
    for blocks in (1, 7, 300):                                                             # other grids
        _assert_equal(grad_guard.grad_stats(dev, blocks=blocks), want)
    # per entry, what else is in the table does not matter
    other = _table(seed=5, plant=False)
    for i in (0, 4, 9, 11):
        mixed = list(other)
        mixed[i] = table[i]
        (sumsq, maxabs, bad), _ = grad_guard.grad_stats(_on_device(mixed))
        assert float(sumsq[i]).hex() == float(want[0][i][0]).hex() and np.float32(maxabs[i]) == want[0][i][1] and bad[i] == want[0][i][2]
    (sumsq, _, _), _ = grad_guard.grad_stats(dev[11:12])
    assert float(sumsq[0]).hex() == float(want[0][11][0]).hex()
    # the clean table: a norm
    clean = _table(plant=False)
    _assert_equal(grad_guard.grad_stats(_on_device(clean)), ref.table_stats(clean))
    gauss = [np.random.RandomState(n).standard_normal(n).astype(np.float32) for n in (7, 16384, 49152, 300001)]
    _assert_equal(grad_guard.grad_stats(_on_device(gauss)), ref.table_stats(gauss))


def test_grad_stats_refuses_a_bad_table_before_launching():
    from video_frame_inpainting_amd import _native
    L = _native.lib()
    x = torch.zeros(40000, device=DEV)
    rows = np.array([[x.data_ptr(), 40000, 0, 0]], dtype=np.int64)
    table = torch.from_numpy(rows).to(DEV)
    ws = torch.zeros(64, dtype=torch.int64, device=DEV)
    out = torch.zeros(16, dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda r, nseg: L.tai_grad_stats(table.data_ptr(), r.ctypes.data, 1, nseg, 0, ws.data_ptr(), out.data_ptr(), out.data_ptr() + 32,
                                            out.data_ptr() + 64, stream)
    assert call(rows, 3) == 0
    assert call(rows, 2) != 0 and b'segments' in L.tai_sepconv_last_error()
    for bad in ([x.data_ptr() + 2, 40000, 0, 0], [x.data_ptr(), -1, 0, 0], [0, 40000, 0, 0], [x.data_ptr(), 40000, 0, 1]):
        assert call(np.array([bad], dtype=np.int64), 3) != 0 and b'row 0' in L.tai_sepconv_last_error()
    assert L.tai_grad_scale(table.data_ptr(), rows.ctypes.data, 1, 3, float('nan'), 0, None, stream) != 0
    assert L.tai_grad_scale(table.data_ptr(), rows.ctypes.data, 1, 2, 0.5, 0, None, stream) != 0
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0 and L.tai_grad_scale_workspace_bytes(1, 3) == 0


def test_grad_scale_kernel_is_one_fp32_product_per_element():
    """Finite values and +-Inf (the guard never scales a table that holds a NaN, and a NaN's payload is not part of the definition)."""
    table = _table(seed=3, plant=False)
    table[-1][[5, 70000]] = [np.inf, -np.inf]
    for c in (np.float32(0.3), np.float32(1.0 / 3.0e5), np.float32(0.99999994)):
        for behind in ((1, 0), (0,), (3, 2)):
            dev = _on_device(table, behind)
            grad_guard.scale_(dev, c)
            for a, t in zip(table, dev):
                assert np.array_equal(t.cpu().numpy().view(np.uint32), (a * c).view(np.uint32))
    # nothing outside [address, address + 4 n) is written
    for n in (5, 16385):
        buf = torch.full((n + 16,), 7.0, device=DEV)
        first = (16 - buf.data_ptr() % 16) % 16 // 4 + 1
        grad_guard.scale_([buf[first:first + n]], np.float32(0.5))
        got = buf.cpu().numpy()
        assert np.all(got[:first] == 7.0) and np.all(got[first + n:] == 7.0) and np.all(got[first:first + n] == 3.5)


# ---------------------------------------------------------------------------------------------------------------- the training environment

@pytest.fixture
def reproducible():
    previous = (tai.set_reproducible_backward(True), torch.backends.cudnn.deterministic)
    torch.backends.cudnn.deterministic = True
    yield
    tai.set_reproducible_backward(previous[0])
    torch.backends.cudnn.deterministic = previous[1]


def _env(tmp_path, name, guard, seed=0):
    torch.manual_seed(seed)
    np.random.seed(seed)
    return create_training_environment(vfi.create_model(SPEC), 1, str(tmp_path / 'ckpt'), name, K, T, F, [SIZE, SIZE], 1.0, 0.02, 1e-4, 0.5, 8,
                                       3, 3, [0, 0], device=DEV, guard=guard)


_CLIPS = torch.from_numpy(synthetic.make_clips(6, K + T + F, 1, SIZE, SIZE, 1002))


def _poisoned(clips):
    bad = clips.clone()
    bad[0, K, 0, 5, 7] = float('inf')                                       # one Inf in a ground-truth frame
    return bad


def _update(env, i=0, clips=None):
    clips = _CLIPS[2 * i:2 * i + 2] if clips is None else clips
    env.K, env.T, env.F = K, T, F
    env.train()
    env.train_step(clips[:, :K], clips[:, K + T:], clips[:, K:K + T])


def _state(env, parts=('G', 'D', 'oG', 'oD')):
    out = {}
    if 'G' in parts:
        out.update(('G.' + k, v.clone()) for k, v in env.generator.state_dict().items())
    if 'D' in parts:
        out.update(('D.' + k, v.clone()) for k, v in env.discriminator.state_dict().items())
    for tag, opt in (('oG', env.optimizer_G), ('oD', env.optimizer_D)):
        if tag in parts:
            for i, st in opt.state_dict()['state'].items():
                assert set(st) == {'step', 'exp_avg', 'exp_avg_sq'}
                out.update(('%s.%s.%s' % (tag, i, k), torch.as_tensor(v).clone()) for k, v in st.items())
    return out


def _same(a, b):
    assert set(a) == set(b)
    different = [k for k in a if not torch.equal(a[k].cpu(), b[k].cpu())]
    assert not different, 'first of %d differing tensors: %s' % (len(different), different[0])


def test_clean_guarded_updates_are_the_unguarded_ones(tmp_path, reproducible):
    plain, env = _env(tmp_path, 'plain', None), _env(tmp_path, 'guarded', grad_guard.GradGuard())
    for e in (plain, env):
        torch.manual_seed(1)                                               # the spectral-norm vectors are drawn in the first forward
        for i in range(3):
            _update(e, i)
    _same(_state(plain), _state(env))
    g = env.guard
    assert g.counters() == {'skipped_G': 0, 'skipped_D': 0, 'consecutive': 0} and g.verdict == {'G': grad_guard.OK, 'D': grad_guard.OK}
    # the norms it reports are the restated ones of the gradients still in place
    for which, module in (('G', env.generator), ('D', env.discriminator)):
        grads = [p.grad for p in module.parameters() if p.grad is not None]
        assert g.norm[which] == math.sqrt(float(ref.table_stats(grads)[1][0])) and g.norm[which] > 0
    assert any(p.grad is None for p in env.generator.parameters())          # merge_residual1 never gets one: left out of the table


def test_poisoned_batch_skips_both_steps_and_the_next_clean_update_steps(tmp_path, reproducible):
    env = _env(tmp_path, 'poison', grad_guard.GradGuard())
    _update(env, 0)                                                        # Adam's state exists
    before = _state(env)
    _update(env, 1, _poisoned(_CLIPS[2:4]))
    after = _state(env)
    _same({k: v for k, v in before.items() if not k.startswith('D.')}, {k: v for k, v in after.items() if not k.startswith('D.')})
    assert all(bool(torch.isfinite(v).all()) for k, v in after.items() if k.startswith('D.'))
    g = env.guard
    assert (g.skipped_G, g.skipped_D, g.consecutive) == (1, 1, 1) and g.verdict == {'G': grad_guard.SKIPPED, 'D': grad_guard.SKIPPED}
    names = [n for n, _ in env.discriminator.named_parameters()]
    print(g.message)
    assert 'non-finite' in g.message and any(' in %s ' % n in g.message for n in names)
    _update(env, 2)
    later = _state(env)
    assert (g.skipped_G, g.skipped_D, g.consecutive) == (1, 1, 0)
    steps = [k for k in later if k.endswith('.step')]
    assert steps and all(float(later[k]) == float(before[k]) + 1 for k in steps)
    assert any(not torch.equal(before[k], later[k]) for k in before if k.startswith('G.'))
    assert all(bool(torch.isfinite(v).all()) for v in later.values())


def test_clipping_scales_every_gradient_by_the_restated_coefficient(tmp_path, reproducible):
    twin = _env(tmp_path, 'twin', grad_guard.GradGuard())
    torch.manual_seed(1)
    _update(twin, 0)
    X = 0.5 * min(twin.guard.norm['G'], twin.guard.norm['D'])              # both optimizers clip
    env = _env(tmp_path, 'clipped', grad_guard.GradGuard(clip_grad_norm=X))
    torch.manual_seed(1)
    _update(env, 0)
    assert env.guard.verdict == {'G': grad_guard.CLIPPED, 'D': grad_guard.CLIPPED} and env.guard.norm == twin.guard.norm
    for which, mine, theirs in (('G', env.generator, twin.generator), ('D', env.discriminator, twin.discriminator)):
        raw = [p.grad.cpu().numpy() for p in theirs.parameters() if p.grad is not None]
        total, _, bad = ref.table_stats(raw)[1]
        c = ref.coefficient(float(total), bad, X)
        assert isinstance(c, np.float32) and c < 1 and env.guard.coefficient[which] == c
        scaled = [p.grad.cpu().numpy() for p in mine.parameters() if p.grad is not None]
        assert len(scaled) == len(raw)
        for a, b in zip(scaled, raw):
            assert np.array_equal(a.view(np.uint32), (b * c).view(np.uint32))
        norm = math.sqrt(float(ref.table_stats(scaled)[1][0]))
        print('%s: norm %.9g -> %.9g, X = %.9g, c = %r' % (which, math.sqrt(float(total)), norm, X, c))
        assert norm <= X * (1 + 2.0 ** -20)                                # fp32 rounding of c and of the products


def test_poisoned_state_is_not_written_over_a_snapshot(tmp_path, reproducible):
    env = _env(tmp_path, 'refuse', grad_guard.GradGuard())
    _update(env, 0)
    env.save('model_latest.ckpt', 1, 0, 0)
    path = tmp_path / 'ckpt' / 'refuse' / 'model_latest.ckpt'
    healthy = path.read_bytes()
    name, weight = next((n, p) for n, p in env.generator.named_parameters() if p.numel() > 10)
    weight.data.view(-1)[3] = float('inf')
    with pytest.raises(environments.SnapshotRefused, match=re.escape('generator.' + name)):
        env.save('model_latest.ckpt', 2, 0, 0)
    assert path.read_bytes() == healthy and sorted(os.listdir(path.parent)) == ['model_latest.ckpt']


def test_patience_ends_the_run_and_leaves_the_healthy_snapshot(tmp_path, reproducible, monkeypatch, capsys):
    env = _env(tmp_path, 'patience', grad_guard.GradGuard(patience=2))
    _update(env, 0)
    env.save('model_latest.ckpt', 1, 0, 0)
    path = tmp_path / 'ckpt' / 'patience' / 'model_latest.ckpt'
    healthy = path.read_bytes()
    _update(env, 1, _poisoned(_CLIPS[2:4]))
    with pytest.raises(grad_guard.GuardGaveUp, match='non-finite'):
        _update(env, 2, _poisoned(_CLIPS[4:6]))
    assert env.guard.consecutive == 2 and path.read_bytes() == healthy

    # train.py: every clip holds an Inf -> non-zero exit after N updates, nothing written
    real = synthetic.make_clips

    def poisoned_clips(*a, **k):
        clips = real(*a, **k)
        clips[:, K, 0, 5, 7] = np.inf
        return clips
    monkeypatch.setattr(synthetic, 'make_clips', poisoned_clips)
    monkeypatch.chdir(tmp_path)
    import train
    args = ['--name', 'dead', '--K', str(K), '--T', str(T), '--F', str(F), '--c_dim', '1', '--image_size', str(SIZE), '--model_key', SPEC,
            '--checkpoints_dir', str(tmp_path / 'ckpt'), '--batch_size', '2', '--max_iter', '6', '--print_freq', '1', '--df_dim', '8',
            '--synthetic', '4', '--guard', '--guard_patience', '3']
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        train.main(args)
    out = capsys.readouterr().out
    assert e.value.code not in (0, None) and 'iter 3' in str(e.value.code) and 'gives up' in str(e.value.code)
    assert re.findall(r'^iter (\d+) ', out, re.M) == ['1', '2'] and 'skipped=4' in out and 'Done.' not in out
    assert not os.path.exists(tmp_path / 'ckpt' / 'dead' / 'model_latest.ckpt')


# ---------------------------------------------------------------------------------------------------------------- train.py, straight against split

def test_clipped_resumable_run_straight_against_split(tmp_path, capsys, monkeypatch):
    """X = 1e-3 is far below the gradient norm of an untrained network on these losses, so updates clip -- asserted from the log."""
    monkeypatch.chdir(tmp_path)
    X = 1e-3
    extra = ['--synthetic', '4', '--guard', '--clip_grad_norm', repr(X)]
    seen = []
    real = resume._train

    def train_and_keep(*a, **k):
        seen.append(real(*a, **k))
        return seen[-1]
    monkeypatch.setattr(resume, '_train', train_and_keep)
    a = resume._straight_and_split(tmp_path, capsys, 'clip', extra)
    b = resume._latest(tmp_path, 'clipB')
    lines = re.findall(r'^iter (\d+) .* gnorm_G=(\S+) gnorm_D=(\S+) skipped=(\d+) state=[0-9a-f]{16}$', seen[0], re.M)
    assert [int(l[0]) for l in lines] == [1, 2, 3, 4] and all(l[3] == '0' for l in lines)
    print(lines)
    assert any(float(l[1]) > X for l in lines) and any(float(l[2]) > X for l in lines)          # it did clip
    assert a['run_state']['guard'] == b['run_state']['guard'] == {'skipped_G': 0, 'skipped_D': 0, 'consecutive': 0}
    # the straight and the split log carry the same norms, digit for digit
    split = re.findall(r'gnorm_G=(\S+) gnorm_D=(\S+)', seen[1] + seen[2])
    assert [(l[1], l[2]) for l in lines] == split
