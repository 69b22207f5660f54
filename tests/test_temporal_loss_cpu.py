"""The temporal-difference loss without a GPU (train.py --temporal_weight; losses.TemporalLoss; include/tai_sepconv.h tai_temporal_loss):
the numpy restatement of the definition (temporal_loss_ref.py) against float64 autograd of the plain composition, the module's CPU path
against the restatement, T = 1, every refusal of the C ABI (argument checks run before any runtime call, so they need no device), the
flags, one CPU update, and the header / library / launch constants."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))          # (for the child process of the refusal test)
import temporal_loss_ref as ref  # noqa: E402

import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import _native, synthetic  # noqa: E402
from video_frame_inpainting_amd.ablations import BidirectionalSimpleAverageFillInModel  # noqa: E402
from video_frame_inpainting_amd.environments import create_training_environment  # noqa: E402
from video_frame_inpainting_amd.losses import TemporalLoss, _block_strides  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-3
SHAPES = [(2, 1, 1, 2, 2), (1, 2, 3, 5, 7), (3, 5, 1, 17, 66)]
U = 2.0 ** -24                   # fp32 unit roundoff


def _delta_bound(pred, gt):
    """What the restatement's fp32 d can be away from the exact difference of the same fp32 inputs: d carries four fp32 roundings (of
    pred + 1 and gt + 1 -- the halving is exact --, of e and of d) of values up to 2 m, m = the largest magnitude among the inputs
    (1 for nominal frames)."""
    m = max(1.0, float(np.abs(pred).max()), float(np.abs(gt).max()))
    return 4 * U * 2 * m


def _grad_bound(kind, pred, gt):
    """On grad / ct = rho'(d_t) - rho'(d_{t+1}): two rho' values.  kind 0: rho' = 2 d doubles d's error exactly.  kind 2: the slope of
    d / sqrt(d^2 + eps^2) is at most 1 / eps, so d's error grows by that (its own few roundings of a value below 1 are far below
    that).  kind 1: sgn is exact wherever d is further from 0 than its error, and is compared only there."""
    return {0: 4 * _delta_bound(pred, gt), 1: 0.0, 2: 4 * _delta_bound(pred, gt) / EPS}[kind]


def _composition(pred32, gt32, kind):
    """float64 torch composition on the same fp32 values -> (loss, grad, d), numpy float64."""
    p = torch.from_numpy(pred32).double().requires_grad_()
    e = (p + 1) / 2 - (torch.from_numpy(gt32).double() + 1) / 2
    zero = torch.zeros_like(e[:, :1])
    e = torch.cat([zero, e, zero], dim=1)
    d = e[:, 1:] - e[:, :-1]
    if kind == 0:
        rho = d * d
    elif kind == 1:
        rho = d.abs()
    else:
        e2 = float(np.float32(EPS) * np.float32(EPS))       # the definition's constant: eps * eps in fp32
        rho = torch.sqrt(d * d + e2)
    loss = rho.mean()
    loss.backward()
    return float(loss.detach()), p.grad.numpy(), d.detach().numpy()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', [0, 1, 2], ids=ref.KIND_NAMES)
def test_restatement_matches_float64_autograd_and_the_cpu_module_matches_the_restatement(kind, shape):
    B, T, C, H, W = shape
    for inputs in ref.KINDS:
        pred, gt = ref.make_pair(inputs, shape, 31 + W)
        loss64, grad64, d64 = _composition(pred, gt, kind)
        want = ref.temporal_loss_ref(pred, gt, kind, EPS)
        assert want['grad'].dtype == np.float32 and want['grad'].shape == pred.shape and want['seq_terms'].shape == (B * C, T + 1)
        assert want['count'] == B * C * (T + 1) * H * W and want['ct'] == 0.5 / want['count']
        # ---- the restatement against float64 autograd, on grad / ct
        bound = _grad_bound(kind, pred, gt)
        diff = np.abs(want['grad64'] - grad64) / want['ct']
        if kind == 1:                                                           # away from d = 0 only
            far = np.abs(d64) > _delta_bound(pred, gt)
            diff = np.where(far[:, :-1] & far[:, 1:], diff, 0.0)
            bound = 1e-9                                                        # equal: autograd multiplies by 0.5 / count in its own order
        print('restatement %s %s kind %d: grad / ct off by %.3e (bound %.3e); loss %.9e rel %.2e' % (
            inputs, shape, kind, diff.max(), bound, want['loss'], abs(want['loss'] - loss64) / max(abs(loss64), 1e-300)))
        assert diff.max() <= bound
        # rho's own error: kind 0 2 |d| Dd, kinds 1 and 2 Dd (slope at most 1), plus rho's fp32 roundings
        dd = _delta_bound(pred, gt)
        assert abs(want['loss'] - loss64) <= (2 * np.abs(d64).max() if kind == 0 else 1.0) * dd + 4 * U * max(abs(loss64), EPS)
        assert np.allclose(want['terms'].sum() / (T + 1), want['loss'], rtol=1e-13, atol=0)
        # ---- the module's CPU path against the restatement: the same fp32 terms by torch ops, float64 sums, fp32 autograd
        p = torch.from_numpy(pred).requires_grad_()
        module = TemporalLoss(ref.KIND_NAMES[kind], EPS)
        loss = module(p, torch.from_numpy(gt))
        assert loss.dtype == torch.float32 and loss.dim() == 0
        loss.backward()
        seqs, terms = module.seq_terms.numpy(), module.last_terms.numpy()
        assert seqs.shape == (1, B * C, T + 1) and seqs.dtype == np.float64 and terms.shape == (1, T + 1) and terms.dtype == np.float32
        assert not module.seq_terms.requires_grad and not module.last_terms.requires_grad
        m_loss = seqs[0].sum() / want['count']
        rel = abs(m_loss - want['loss']) / max(abs(want['loss']), 1e-300)
        # the gradient: the module multiplies rho' by fp32(1 / count) and subtracts in fp32 where the definition subtracts and scales in
        # float64 and rounds once: per rho' the cast of 1 / count, the products of the chain rule (kind 0: d g + d g, three roundings; kind
        # 1: none; kind 2: those, the division by 2 s and torch's own square root and division, which may be an ulp off numpy's: nine) and
        # the fp32 subtraction
        n_roundings = {0: 5, 1: 2, 2: 11}[kind]
        g_bound = n_roundings * U * (np.abs(want['drho'][:, :-1]) + np.abs(want['drho'][:, 1:])).astype(np.float64) * want['ct']
        g_diff = np.abs(p.grad.numpy().astype(np.float64) - want['grad64'])
        print('module %s %s kind %d: loss rel %.2e; gradient off by %.2f of its bound' % (
            inputs, shape, kind, rel, float((g_diff / np.maximum(g_bound, 1e-300)).max())))
        assert rel <= 1e-12
        assert (g_diff <= g_bound).all()
        assert abs(float(loss.detach()) - want['loss']) <= 2.0 ** -23 * abs(want['loss'])       # the fp32 scalar
        np.testing.assert_allclose(terms[0], want['terms'], rtol=2.0 ** -23, atol=0)
        if inputs == 'equal':                                                   # sgn(0) = 0: every d is 0
            assert not want['grad'].any() and not p.grad.numpy().any()
            assert want['loss'] == 0.0 if kind < 2 else abs(want['loss'] - EPS) <= 2.0 ** -22 * EPS          # rho(0) = sqrt(eps * eps)


def test_one_frame_has_both_seams_and_a_constant_error_is_counted_at_the_seams_only():
    for kind in (0, 1, 2):
        pred, gt = ref.make_pair('uniform', (2, 1, 3, 5, 7), 3)
        want = ref.temporal_loss_ref(pred, gt, kind, EPS)
        e = (pred + np.float32(1)) / np.float32(2) - (gt + np.float32(1)) / np.float32(2)
        rho = {0: e * e, 1: np.abs(e), 2: np.sqrt(e * e + np.float32(EPS) * np.float32(EPS))}[kind][:, 0]
        assert np.array_equal(want['rho'][:, 0], rho) and np.array_equal(want['rho'][:, 1], rho)          # d_1 = -d_0
        per_pixel = want['rho'].astype(np.float64).sum(axis=1)
        assert np.array_equal(per_pixel, 2.0 * rho.astype(np.float64))
        assert np.array_equal(want['seq_terms'][:, 0], want['seq_terms'][:, 1])
        assert np.array_equal(want['grad64'][:, 0], (want['drho'][:, 0].astype(np.float64) - want['drho'][:, 1].astype(np.float64)) * want['ct'])
    # an error that is the same in every frame: the inner positions see d = 0
    gt = ref.make_pair('grid', (2, 4, 1, 6, 8), 5)[1]
    pred = gt + np.float32(0.25)
    want = ref.temporal_loss_ref(pred, gt, 1)
    assert np.array_equal(want['terms'], [0.125, 0.0, 0.0, 0.0, 0.125])
    assert not want['grad'][:, 1:-1].any() and (want['grad'][:, 0] > 0).all() and (want['grad'][:, -1] > 0).all()


def test_grid_sums_do_not_depend_on_their_order():
    """On grid inputs every d is a multiple of 2^-7 of size at most 2: every term is a multiple of 2^-33 below 4, and float64 sums of up to
    2^18 of them are exact, whatever the order."""
    shape = (4, 5, 3, 17, 66)
    pred, gt = ref.make_pair('grid', shape, 5)
    rs = np.random.RandomState(1)
    for kind in (0, 1, 2):
        want = ref.temporal_loss_ref(pred, gt, kind, EPS)
        d = want['delta'].astype(np.float64)
        assert np.all(np.abs(d) < 2.0) and np.all(d * 128.0 == np.round(d * 128.0)) and (d == 0).mean() > 0.05
        t = want['rho'].astype(np.float64).ravel()
        assert t.size <= 1 << 18 and np.all(t < 4.0) and np.all(t * 2.0 ** 33 == np.round(t * 2.0 ** 33))
        assert t.sum() == t[::-1].sum() == np.sort(t).sum() == t[rs.permutation(t.size)].sum() == float(sum(float(c.sum()) for c in np.array_split(t, 37)))


def test_three_predictions_a_time_major_view_and_float64():
    shape = (2, 3, 2, 9, 11)
    preds = [ref.make_pair('uniform', shape, s)[0] for s in (1, 2, 3)]
    gt = ref.make_pair('uniform', shape, 4)[1]
    module = TemporalLoss('charbonnier', EPS)
    ts = tuple(torch.from_numpy(p).requires_grad_() for p in preds)
    losses = module(ts, torch.from_numpy(gt))
    assert isinstance(losses, tuple) and len(losses) == 3 and module.last_terms.shape == (3, 4) and module.seq_terms.shape == (3, 4, 4)
    sum(losses).backward()
    for t, p, loss in zip(ts, preds, losses):
        want = ref.temporal_loss_ref(p, gt, 2, EPS)
        assert abs(float(loss.detach()) - want['loss']) <= 2.0 ** -23 * want['loss']
        assert np.abs(t.grad.numpy() - want['grad64']).max() <= 2.0 ** -20 * np.abs(want['grad64']).max()
    # the time-major storage of tai.py's ``pred``: a transposed view; the gradient comes back in the view's shape
    stored = torch.from_numpy(preds[0]).transpose(0, 1).contiguous()          # [T, B, C, H, W]
    view = stored.transpose(0, 1).requires_grad_()
    assert not view.is_contiguous() and _block_strides(view) == (2 * 99, 2 * 2 * 99)
    loss = TemporalLoss('l1')(view, torch.from_numpy(gt))
    loss.backward()
    want = ref.temporal_loss_ref(preds[0], gt, 1)
    assert view.grad.shape == view.shape and np.abs(view.grad.numpy() - want['grad64']).max() <= 2.0 ** -21 * np.abs(want['grad64']).max()
    # float64 tensors: the same definition in float64
    p64 = torch.from_numpy(preds[0]).double().requires_grad_()
    loss64 = TemporalLoss('l2')(p64, torch.from_numpy(gt).double())
    assert loss64.dtype == torch.float64
    assert abs(float(loss64.detach()) - _composition(preds[0], gt, 0)[0]) <= 1e-14
    # (Charbonnier: e2 is the definition's constant, eps * eps in fp32, in either precision)
    c64 = TemporalLoss('charbonnier', EPS)(torch.from_numpy(preds[0]).double(), torch.from_numpy(gt).double())
    assert abs(float(c64) - _composition(preds[0], gt, 2)[0]) <= 1e-14


def test_which_tensors_are_read_where_they_lie():
    x = torch.zeros(3, 4, 2, 5, 8)
    assert _block_strides(x) == (320, 80)
    assert _block_strides(x.transpose(0, 1).contiguous().transpose(0, 1)) == (80, 240)
    assert _block_strides(x[:, 1:3]) == (320, 80) and _block_strides(x[1:]) == (320, 80)
    assert _block_strides(x[..., ::2]) is None and _block_strides(x[..., 1:]) is None and _block_strides(x[:, :, :1]) == (320, 80)
    assert _block_strides(x[:, :, :, 1:]) is None and _block_strides(x.permute(0, 2, 1, 3, 4)) is None
    assert _block_strides(x[:1].expand(3, 4, 2, 5, 8)) is None                # a stride of 0: the blocks overlap
    assert _block_strides(x[:, :1]) == (320, 960) and _block_strides(x[:1]) == (320, 80) and _block_strides(x[:1, :1]) == (80, 80)


def test_the_module_refuses_what_it_cannot_take_and_carries_no_state():
    assert not TemporalLoss().state_dict() and not list(TemporalLoss().parameters()) and not list(TemporalLoss().buffers())
    assert TemporalLoss().kind == 'charbonnier' and TemporalLoss().eps == 1e-3
    with pytest.raises(ValueError):
        TemporalLoss()(torch.zeros(1, 2, 1, 8, 8), torch.zeros(1, 2, 1, 8, 9))
    with pytest.raises(ValueError):
        TemporalLoss()(torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 8, 8))
    with pytest.raises(ValueError):
        TemporalLoss()(torch.zeros(0, 2, 1, 8, 8), torch.zeros(0, 2, 1, 8, 8))
    with pytest.raises(ValueError):
        TemporalLoss()((torch.zeros(1, 1, 1, 8, 8),) * 4, torch.zeros(1, 1, 1, 8, 8))
    with pytest.raises(ValueError):
        TemporalLoss('huber')
    for eps in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            TemporalLoss('charbonnier', eps)


# ---------------------------------------------------------------------------------------------------------------- the C ABI's refusals

P = 16                          # a pointer that is never followed: a refused call reads none of its device buffers
CHW = 64                        # C H W of the calls below: (B, T, C, H, W) = (2, 3, 1, 8, 8)
DIMS = (2, 3, 1, 8, 8)
BT = (3 * CHW, CHW)             # [B, T, ...] storage
TB = (CHW, 2 * CHW)             # time-major storage


def _call(preds=(P,), npred=1, gt=P, strides=BT + BT, kind=0, eps=0.0, seq_terms=P, totals=P, grads=None, workspace=P, dims=DIMS):
    return [preds, npred, gt, strides, kind, eps, seq_terms, totals, grads, workspace] + list(dims)


# (arguments, a word of the message)
REFUSALS = [
    (_call(preds=None), 'null pointer'), (_call(gt=None), 'null pointer'), (_call(strides=None), 'null pointer'),
    (_call(seq_terms=None), 'null pointer'), (_call(totals=None), 'null pointer'), (_call(workspace=None), 'null pointer'),
    (_call(preds=(P, None), npred=2, strides=BT * 3), 'null prediction pointer'),
    (_call(npred=0), 'npred'), (_call(npred=4, preds=(P,) * 4, strides=BT * 5), 'npred'), (_call(npred=-1), 'npred'),
    (_call(kind=-1), 'kind'), (_call(kind=3), 'kind'),
    (_call(kind=2, eps=0.0), 'eps'), (_call(kind=2, eps=-1.0), 'eps'), (_call(kind=2, eps='nan'), 'eps'), (_call(kind=2, eps='inf'), 'eps'),
    (_call(dims=(0, 3, 1, 8, 8)), '>= 1'), (_call(dims=(2, 0, 1, 8, 8)), '>= 1'), (_call(dims=(2, 3, 0, 8, 8)), '>= 1'),
    (_call(dims=(2, 3, 1, 0, 8)), '>= 1'), (_call(dims=(2, 3, 1, 8, -1)), '>= 1'),
    (_call(dims=(1, 1, 1, 1 << 16, 1 << 15)), 'too large'), (_call(dims=(1 << 20, 1, 1 << 10, 1 << 5, 1 << 5)), 'too large'),
    (_call(dims=(1 << 10, 1 << 20, 1 << 10, 1, 1)), 'too large'),
    (_call(dims=(1 << 20, 1, 1, 1 << 19, 1)), 'chunks'), (_call(dims=(1 << 30, 1, 2, 1, 1)), 'sequence positions'), (_call(dims=(1 << 15, 1 << 16, 1, 1, 1)), 'sequence positions'),
    (_call(strides=(0, CHW) + BT), 'positive'), (_call(strides=BT + (3 * CHW, -CHW)), 'positive'),
    (_call(strides=(1 << 40, CHW) + BT), '2^40'), (_call(strides=BT + (3 * CHW, 1 << 39)), '2^40'),
    (_call(strides=(3 * CHW, CHW - 1) + BT), 'overlap'), (_call(strides=(3 * CHW - 1, CHW) + BT), 'overlap'),
    (_call(strides=BT + (CHW, 2 * CHW - 1)), 'overlap'), (_call(strides=BT + (CHW - 1, 2 * CHW)), 'overlap'),
    (_call(strides=BT + (CHW, CHW)), 'overlap'), (_call(strides=(5 * CHW, 2 * CHW + 32) + BT), 'overlap'),
    (_call(seq_terms=P + 4), 'aligned'), (_call(totals=P + 4), 'aligned'), (_call(workspace=P + 4), 'aligned'),
]
# what must get past every check: asked of the checks alone, in a stand-alone host program (nothing is launched for these)
ACCEPTED = [_call(), _call(strides=TB + BT), _call(strides=BT + TB), _call(kind=2, eps=1e-3), _call(kind=0, eps='nan'),
            _call(strides=(3 * CHW, 2 * CHW) + (3 * CHW + 5, CHW + 1)),            # interleaved batches; padded blocks
            _call(preds=(P, P, P), npred=3, strides=TB + BT * 3, grads=(P, None, P)),
            _call(dims=(2, 3, 1, 1, 1), strides=(1, 2, 3, 1))]
EINVAL = -1


def _answers(lib_path):
    """Run in a child process that sees no device: [(return code, message)] for REFUSALS: calls that end before any launch."""
    L = ctypes.CDLL(lib_path)
    for name, (restype, argtypes) in _native.signatures().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    out = []
    for args in [r[0] for r in REFUSALS]:
        preds, npred, gt, strides, kind, eps, seq_terms, totals, grads, workspace = args[:10]
        keep = [None if a is None else (ctypes.c_void_p * len(a))(*a) for a in (preds, grads)]
        table = None if strides is None else (ctypes.c_longlong * len(strides))(*strides)
        cast = lambda a: None if a is None else ctypes.cast(a, ctypes.c_void_p)
        rc = L.tai_temporal_loss(cast(keep[0]), npred, gt, cast(table), kind, float(eps), seq_terms, totals, cast(keep[1]), workspace,
                                 *args[10:], None)
        out.append([rc, L.tai_sepconv_last_error().decode()])
    return out


def _library_refusals():
    """The library's message for each of REFUSALS, replayed in a child process that sees no device; each is checked on the way."""
    _native.verify(_native.LIB_PATH)
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1')
    child = subprocess.run([sys.executable, os.path.abspath(__file__), '--answers', _native.LIB_PATH], env=env, capture_output=True, text=True,
                           timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    got = json.loads(child.stdout)
    assert len(got) == len(REFUSALS)
    for (args, word), (rc, message) in zip(REFUSALS, got):
        assert rc == EINVAL and message.startswith('temporal_loss: ') and word in message, (args, rc, message)
    # every message the launcher can give is reached
    source = open(os.path.join(_native.CSRC, 'temporal_loss.hip.inc')).read()
    said = {m for _, m in got[:len(REFUSALS)]}
    assert len(said) == 13 and set(re.findall(r'return "(temporal_loss: [^"]*)";', source)) == said
    return [m for _, m in got]


def test_every_refusal_returns_the_error_and_its_message_without_a_device():
    assert len(_library_refusals()) == len(REFUSALS)


def _cpp(v, kind='ptr'):
    if kind == 'ptr':
        return 'nullptr' if v is None else 'P(%d)' % v
    if kind == 'eps':
        return {'nan': 'NAN', 'inf': 'INFINITY'}.get(v, '%rf' % float(v) if not isinstance(v, str) else v)
    return '%dLL' % v


def test_the_checks_alone_take_what_they_should_and_refuse_the_rest(tmp_path):
    """temploss::call_refusal in a stand-alone host program: the launcher's whole argument check, with no launch behind it.  The refused
    calls give the library's messages word for word; the accepted ones, every layout in use among them, come back null."""
    hipcc = shutil.which('hipcc')
    assert hipcc, 'hipcc builds the library, so it is there wherever this suite runs'
    rows = []
    for args in [r[0] for r in REFUSALS] + ACCEPTED:
        preds, npred, gt, strides, kind, eps, seq_terms, totals, grads, workspace = args[:10]
        pa = 'nullptr' if preds is None else 'std::vector<const float*>{%s}.data()' % ', '.join(_cpp(v) for v in preds)
        sa = 'nullptr' if strides is None else 'std::vector<long long>{%s}.data()' % ', '.join(_cpp(v, 'll') for v in strides)
        rows.append('    say(temploss::call_refusal(%s, %d, %s, %s, %d, %s, (const double*)%s, (const double*)%s, %s, %s));' % (
            pa, npred, _cpp(gt), sa, kind, _cpp(eps, 'eps'), _cpp(seq_terms), _cpp(totals), _cpp(workspace), ', '.join('%d' % d for d in args[10:])))
    src = tmp_path / 'checks.cpp'
    src.write_text('#include <hip/hip_runtime.h>\n#include <cmath>\n#include <cstdint>\n#include <cstdio>\n#include <vector>\n'
                   '#include "temporal_loss.hip.inc"\n'
                   'static const float* P(long long v) { return reinterpret_cast<const float*>(v); }\n'
                   'static void say(const char* why) { std::printf("%s\\n", why ? why : "accepted"); }\n'
                   'int main() {\n' + '\n'.join(rows) + '\n    return 0;\n}\n')
    exe = tmp_path / 'checks'
    subprocess.check_call([hipcc, '-x', 'hip', '--offload-arch=gfx950', '-O1', '-std=c++17', '-w', '-I' + _native.CSRC, '-o', str(exe), str(src)])
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1')
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split('\n')[:-1]
    assert len(lines) == len(REFUSALS) + len(ACCEPTED)
    assert lines[:len(REFUSALS)] == _library_refusals()
    assert lines[len(REFUSALS):] == ['accepted'] * len(ACCEPTED), list(zip(ACCEPTED, lines[len(REFUSALS):]))


def test_the_workspace_query_refuses_the_same_dimensions():
    L = _native.lib()
    q = L.tai_temporal_loss_workspace_bytes
    for args, _ in REFUSALS:
        dims = tuple(args[10:])
        if dims != DIMS:
            assert q(1, *dims) == EINVAL, dims
    assert q(0, *DIMS) == EINVAL and q(4, *DIMS) == EINVAL
    # one float64 per prediction, chunk of 256 four-pixel runs, position and wave
    assert q(1, *DIMS) == 2 * 1 * 4 * 4 * 8 and q(3, 32, 5, 1, 128, 128) == 3 * 32 * 16 * 6 * 4 * 8
    assert q(1, 1, 1, 1, 1, 1) == 2 * 4 * 8 and q(2, 3, 5, 1, 17, 66) == 2 * 3 * 2 * 6 * 4 * 8


# ---------------------------------------------------------------------------------------------------------------- flags, environment

def _main(extra):
    import train
    return train.main(['--name', 'x', '--K', '3', '--T', '2', '--F', '3', '--c_dim', '1', '--image_size', '32', '--batch_size', '2',
                       '--model_key', 'MCNet_gray'] + extra)


def test_the_flags_parse_and_bad_values_are_refused_before_anything_runs(monkeypatch, tmp_path):
    import train
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)         # the option parser's own check; nothing else is reached
    seen = []
    monkeypatch.setattr(train, '_run', lambda opt, stop: seen.append((opt.temporal_weight, opt.temporal_kind, opt.temporal_eps)))
    _main([])
    _main(['--temporal_weight', '0.5'])
    _main(['--temporal_weight', '2', '--temporal_kind', 'l1'])
    _main(['--temporal_weight', '1', '--temporal_kind', 'l2', '--temporal_eps', '0.01'])
    assert seen == [(0.0, 'charbonnier', 1e-3), (0.5, 'charbonnier', 1e-3), (2.0, 'l1', 1e-3), (1.0, 'l2', 0.01)]
    monkeypatch.setattr(train, '_run', lambda *a, **k: pytest.fail('the run was started'))
    for extra in (['--temporal_kind', 'huber'], ['--temporal_weight', '-1'], ['--temporal_weight', 'nan'], ['--temporal_eps', '0'],
                  ['--temporal_eps', 'nan'], ['--temporal_eps', '-1'], ['--temporal_eps', 'inf'],
                  ['--temporal_weight', '0.5', '--temporal_eps', '0', '--resumable']):
        with pytest.raises(SystemExit) as e:
            _main(extra)
        assert e.value.code not in (0, None), extra
    with pytest.raises(ValueError, match='temporal_weight'):
        _env(tmp_path, 'unused', temporal_weight=-0.5)
    with pytest.raises(ValueError, match='temporal_kind'):
        _env(tmp_path, 'unused', temporal_weight=0.5, temporal_kind='huber')
    with pytest.raises(ValueError, match='temporal_eps'):
        _env(tmp_path, 'unused', temporal_weight=0.5, temporal_eps=0.0)


K, T, F = 3, 2, 3
_CLIPS = torch.from_numpy(synthetic.make_clips(2, K + T + F, 1, 32, 32, 77))


def _env(root, name, model='mcnet', **kw):
    torch.manual_seed(0)
    np.random.seed(0)
    net = vfi.MCNetFillInModel(4, 1, 3) if model == 'mcnet' else BidirectionalSimpleAverageFillInModel(4, 1, 3)
    return create_training_environment(net, 1, str(root), name, K, T, F, [32, 32], 1.0, 0.02, 1e-3, 0.5, 4, 2, 3, [0, 0], device='cpu', **kw)


def _update(env):
    env.K, env.T, env.F = K, T, F
    env.train()
    env.set_train_inputs(_CLIPS[:, :K], _CLIPS[:, K + T:], _CLIPS[:, K:K + T])
    env.forward_train()
    env.optimize_parameters()


@pytest.mark.parametrize('model', ['mcnet', 'bidirectional'])
def test_one_cpu_update_with_the_term_and_nothing_without_it(tmp_path, model):
    """The separable convolution exists on the GPU only, so the three-prediction environment is driven here by the bidirectional average
    model (the same TAITrainingEnvironment, the same three outputs) and the one-prediction environment by MC-Net."""
    plain, env = _env(tmp_path, 'plain', model), _env(tmp_path, 'temporal', model, temporal_weight=0.5, temporal_kind='l1')
    assert plain.loss_temporal is None and plain.temporal_weight == 0.0 and isinstance(env.loss_temporal, TemporalLoss)
    assert env.loss_temporal.kind == 'l1' and _env(tmp_path, 'd', model, temporal_weight=1.0).loss_temporal.kind == 'charbonnier'
    _update(plain)
    _update(env)
    a, b = plain.get_current_errors(), env.get_current_errors()
    keys = ['G_temporal'] + (['G_temporal_forward', 'G_temporal_backward'] if model == 'bidirectional' else [])
    print({k: b[k] for k in keys})
    assert sorted(b) == sorted(list(a) + keys) and not any(k.startswith('G_temporal') for k in a)
    assert all(np.isfinite(b[k]) and b[k] > 0 for k in keys)
    # the two environments started from the same weights and saw the same clips: the image terms are the same, and the loss gained 0.5 x
    # each temporal term (the discriminator's spectral-norm vectors are drawn per environment: beta G_GAN moves a little)
    assert all(a[k] == b[k] for k in a if k.startswith(('G_Lp', 'G_gdl')))
    gained = 0.5 * sum(b[k] for k in keys) + 0.02 * (b['G_GAN'] - a['G_GAN'])
    assert abs(b['G_loss'] - (a['G_loss'] + gained)) <= 1e-5 * abs(b['G_loss'])
    gt = _CLIPS[:, K:K + T].numpy()
    for key, out in zip(keys, ('pred', 'pred_forward', 'pred_backward')):
        want = ref.temporal_loss_ref(env.gen_output[out].detach().numpy(), gt, 1)
        assert abs(b[key] - want['loss']) <= 2.0 ** -23 * want['loss']
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in env.generator.parameters() if p.requires_grad)


# ---------------------------------------------------------------------------------------------------------------- header, library

def test_the_header_declares_the_entry_points_and_the_launch_constants_are_the_sources():
    header = open(os.path.join(ROOT, 'include', 'tai_sepconv.h')).read()
    assert {'tai_temporal_loss', 'tai_temporal_loss_workspace_bytes'} <= set(_native.declared_symbols())
    flat = re.sub(r'\s+', ' ', re.sub(r'\s*\n \*\s*', ' ', header))
    for line in ('x = (pred + 1) / 2, y = (gt + 1) / 2, in that operation order (util.inverse_transform);',
                 'e_t = x_t - y_t for t = 0..T-1; e_{-1} = e_T = +0 (the known frames);',
                 'd_j = e_j - e_{j-1} for j = 0..T',
                 'kind 2 (Charbonnier): s = sqrt(d * d + e2) with e2 = eps * eps computed once in fp32; rho = s; rho\' = d / s;',
                 'grad[b,t,c,r,col] = fp32( ((double)rho\'(d_t) - (double)rho\'(d_{t+1})) * ct ), ct = 0.5 / count;',
                 'count = (double)S * (T+1) * H * W;'):
        assert line in flat, line
    assert 'long long tai_temporal_loss_workspace_bytes(int npred, int B, int T, int C, int H, int W);' in header
    V, I, LL, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    sigs = _native.signatures()
    assert sigs['tai_temporal_loss'] == (I, [V, I, V, V, I, Fl, V, V, V, V, I, I, I, I, I, V])
    assert sigs['tai_temporal_loss_workspace_bytes'] == (LL, [I] * 6)
    L = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(L, 'tai_temporal_loss') and hasattr(L, 'tai_temporal_loss_workspace_bytes')
    L.tai_sepconv_version.restype = ctypes.c_int
    assert L.tai_sepconv_version() >= 840
    # the source hash covers the new file, and the GPU tests' constants are the kernel's
    assert os.path.join(_native.CSRC, 'temporal_loss.hip.inc') in _native.sources()
    source = open(os.path.join(_native.CSRC, 'temporal_loss.hip.inc')).read()
    assert 'constexpr int THREADS = 256;' in source and 'constexpr long long GRID_CAP = 1LL << 20;' in source
    assert 'constexpr int WAVES = THREADS / 64;' in source and 'constexpr int MAXP = 3;' in source
    assert '#pragma clang fp contract(off)' in source and 'atomic' not in source.replace('No atomics', '')
    assert '#include "temporal_loss.hip.inc"' in open(_native.MAIN_SOURCE).read()


if __name__ == '__main__':
    if sys.argv[1:2] == ['--answers'] and len(sys.argv) == 3:
        assert os.environ.get('HIP_VISIBLE_DEVICES') == '-1' and os.environ.get('ROCR_VISIBLE_DEVICES') == '-1'
        print(json.dumps(_answers(sys.argv[2])))
