"""The SSIM training loss on the GPU (csrc/ssim_loss.hip.inc through the C ABI and losses.SSIMLoss) against the numpy restatement of its
definition (ssim_loss_ref.py): gradient bit for bit, plane values and loss to 1e-12 relative (the interior mean's order is the kernel's);
reproducible, batch-independent, isolated from a non-finite plane, capturable; and train.py --ssim_weight with the other run options.
The tile is 16 x 16 pixels: sizes below run from a single window over one below / at / one above the tile to three tiles each way."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssim_loss_ref as ref  # noqa: E402
import loss_kit as kit  # noqa: E402
from loss_kit import _bits, _generator, _rel, _states, _train  # noqa: E402

from video_frame_inpainting_amd import _native  # noqa: E402
from video_frame_inpainting_amd.losses import SSIMLoss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TILE = 16

# H and W from {7, 8, 13, TILE - 1, TILE, TILE + 1, 41 (three tiles, not a multiple: the pixel (18, 18) has windows in four), 128};
# (N, C) from {(1, 1), (5, 3), (2, 1)}
CASES = [(1, 1, 7, 7), (2, 1, 8, 7), (1, 1, 8, 13), (5, 3, 13, 15), (2, 1, 15, 17), (1, 1, 16, 16), (5, 3, 17, 16), (2, 1, 16, 41),
         (1, 1, 41, 41), (5, 3, 41, 8), (2, 1, 7, 128), (2, 1, 128, 17), (1, 1, 128, 128)]


@functools.lru_cache(maxsize=None)
def _case(kind, shape, seed=0):
    """(pred, gt, restatement) for a seeded input; computed once, shared, never written to."""
    pred, gt = ref.make_pair(kind, shape, 101 + seed + 7 * shape[-1] + shape[-2])
    want = ref.ssim_loss_ref(pred, gt)
    for a in (pred, gt, want['grad'], want['plane_ssim']):
        a.setflags(write=False)
    return pred, gt, want


def _launch(pred, gt, with_grad=True):
    """tai_ssim_loss through the C ABI -> (plane_ssim [N*C] float64, totals [2] float64, grad float32 or None), numpy."""
    L = _native.lib()
    C, H, W = pred.shape[-3:]
    N = pred.size // (C * H * W)
    nbytes = L.tai_ssim_loss_workspace_bytes(N, C, H, W)
    assert nbytes > 0 and nbytes % 8 == 0
    p, g = torch.from_numpy(np.array(pred)).to(DEV), torch.from_numpy(np.array(gt)).to(DEV)
    ws = torch.full((nbytes // 8,), float('nan'), dtype=torch.float64, device=DEV)
    planes = torch.full((N * C,), -7.0, dtype=torch.float64, device=DEV)
    totals = torch.full((2,), -7.0, dtype=torch.float64, device=DEV)
    grad = torch.full(pred.shape, float('nan'), dtype=torch.float32, device=DEV) if with_grad else None
    rc = L.tai_ssim_loss(p.data_ptr(), g.data_ptr(), planes.data_ptr(), totals.data_ptr(), grad.data_ptr() if with_grad else None,
                         ws.data_ptr(), N, C, H, W, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.tai_sepconv_last_error()
    torch.cuda.synchronize()
    return planes.cpu().numpy(), totals.cpu().numpy(), grad.cpu().numpy() if with_grad else None


@pytest.mark.parametrize('shape', CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_and_module_match_the_restatement(shape):
    N, C, H, W = shape
    for kind in ref.KINDS:
        pred, gt, want = _case(kind, shape)
        planes, totals, grad = _launch(pred, gt)
        wrong = int(np.count_nonzero(_bits(grad) != _bits(want['grad'])))
        d_plane = _rel(planes, want['plane_ssim'])
        d_loss = abs(totals[1] - want['loss']) / max(abs(want['loss']), 1e-300) if want['loss'] != 0 else abs(totals[1])
        print('%s %s: %d of %d gradient words differ; plane_ssim rel %.2e; loss %.15f rel %.2e'
              % (kind, shape, wrong, grad.size, d_plane, totals[1], d_loss))
        assert wrong == 0
        assert d_plane <= 1e-12 and d_loss <= 1e-12 and abs(totals[0] - want['mean_ssim']) <= 1e-12
        assert totals[1] == 1.0 - totals[0]
        # the module: the same launch behind autograd
        p = torch.from_numpy(np.array(pred)).to(DEV).requires_grad_()
        module = SSIMLoss()
        loss = module(p, torch.from_numpy(np.array(gt)).to(DEV))
        assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
        loss.backward()
        assert float(loss.detach()) == float(np.float32(totals[1]))
        assert np.array_equal(_bits(p.grad.cpu().numpy()), _bits(grad))
        assert np.array_equal(_bits(module.plane_ssim.cpu().numpy()), _bits(planes))


def test_two_launches_give_identical_bits_and_the_evaluation_form_the_same_values():
    for kind, shape in (('smooth', (5, 3, 41, 17)), ('uniform', (2, 1, 128, 128))):
        pred, gt, _ = _case(kind, shape)
        a, b, ev = _launch(pred, gt), _launch(pred, gt), _launch(pred, gt, with_grad=False)
        for x, y in zip(a, b):
            assert np.array_equal(_bits(x), _bits(y))
        assert ev[2] is None
        assert np.array_equal(_bits(ev[0]), _bits(a[0])) and np.array_equal(_bits(ev[1]), _bits(a[1]))
        with torch.no_grad():                                                         # the module asks for no gradient map here
            module = SSIMLoss()
            loss = module(torch.from_numpy(np.array(pred)).to(DEV), torch.from_numpy(np.array(gt)).to(DEV))
        assert float(loss) == float(np.float32(a[1][1])) and not loss.requires_grad


def test_a_plane_does_not_depend_on_its_batch():
    shape5 = (5, 1, 41, 17)
    pred5, gt5, want5 = _case('smooth', shape5)
    planes5, _, grad5 = _launch(pred5, gt5)
    assert np.array_equal(_bits(grad5), _bits(want5['grad']))
    for n in (0, 3):
        pred1, gt1 = pred5[n:n + 1], gt5[n:n + 1]
        want1 = ref.ssim_loss_ref(pred1, gt1)
        planes1, _, grad1 = _launch(pred1, gt1)
        assert np.array_equal(_bits(grad1), _bits(want1['grad']))                     # each N through the restatement, bit for bit
        assert _bits(planes1)[0] == _bits(planes5)[n]
        # ... and directly: the two differ by the divisor's factor 5 and one fp32 rounding each
        g1, g5 = grad1.astype(np.float64), grad5[n:n + 1].astype(np.float64) * 5.0
        assert np.all(np.abs(g5 - g1) <= 2.0 ** -22 * np.abs(g1))


def test_a_nan_stays_in_its_plane():
    shape = (5, 3, 17, 41)
    pred, gt, _ = _case('uniform', shape)
    clean_planes, _, clean_grad = _launch(pred, gt)
    dirty = np.array(pred)
    dirty[2, 1, 9, 20] = np.nan                                                       # plane 7
    planes, totals, grad = _launch(dirty, gt)
    keep = np.ones(15, bool)
    keep[7] = False
    assert np.array_equal(_bits(planes[keep]), _bits(clean_planes[keep]))
    assert np.isnan(planes[7]) and not np.isfinite(totals).any()
    g = grad.reshape(15, 17, 41)
    assert np.isfinite(g[keep]).all() and np.array_equal(_bits(g[keep]), _bits(clean_grad.reshape(15, 17, 41)[keep]))
    assert np.isnan(g[7]).any()


@pytest.mark.parametrize('H,W', [(6, 32), (32, 6)])
def test_planes_below_the_window_are_refused(H, W):
    L = _native.lib()
    assert L.tai_ssim_loss_workspace_bytes(2, 1, H, W) < 0
    assert L.tai_ssim_loss_workspace_bytes(0, 1, 32, 32) < 0 and L.tai_ssim_loss_workspace_bytes(1, 0, 32, 32) < 0
    x = torch.zeros(2, 1, H, W, device=DEV)
    with pytest.raises(ValueError):
        SSIMLoss()(x, x)
    out = torch.empty(4, dtype=torch.float64, device=DEV)
    rc = L.tai_ssim_loss(x.data_ptr(), x.data_ptr(), out.data_ptr(), out[2:].data_ptr(), None, out.data_ptr(), 2, 1, H, W,
                         torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b'7' in L.tai_sepconv_last_error()


def test_autograd_scales_the_map_and_takes_a_permuted_view():
    pred, gt, want = _case('smooth', (2, 3, 17, 41))
    p = torch.from_numpy(np.array(pred)).to(DEV).requires_grad_()
    g = torch.from_numpy(np.array(gt)).to(DEV)
    (0.2 * SSIMLoss()(p, g)).backward()
    assert np.array_equal(_bits(p.grad.cpu().numpy()), _bits(np.float32(0.2) * want['grad']))      # one fp32 product
    assert g.grad is None
    # a permuted view [3, 2, H, W] of a [2, 3, H, W] tensor against its contiguous copy
    base = torch.from_numpy(np.array(pred)).to(DEV)
    view = base.permute(1, 0, 2, 3).requires_grad_()
    copy = base.permute(1, 0, 2, 3).contiguous().requires_grad_()
    assert not view.is_contiguous()
    gv = g.permute(1, 0, 2, 3)
    lv, lc = SSIMLoss()(view, gv), SSIMLoss()(copy, gv.contiguous())
    lv.backward()
    lc.backward()
    assert float(lv.detach()) == float(lc.detach())
    assert torch.equal(view.grad.view(torch.int32), copy.grad.view(torch.int32)) and view.grad.shape == view.shape


def test_forward_and_backward_replay_inside_one_graph():
    shape = (2, 1, 32, 32)
    p1, g1, _ = _case('smooth', shape, seed=1)
    p2, g2, want2 = _case('uniform', shape, seed=2)
    sp = torch.from_numpy(np.array(p1)).to(DEV).requires_grad_()
    sg = torch.from_numpy(np.array(g1)).to(DEV)
    kit.check_graph_replay(SSIMLoss, [sp], sg, [p2], g2, [want2['grad']], single=True)


# ---------------------------------------------------------------------------------------------------------------- drivers

def _terms(out, n):
    """{key: [value per printed update]} of the three SSIM terms; asserts each is printed on every line, finite, inside (0, 2)."""
    return kit._terms(out, n, ('G_ssim', 'G_ssim_forward', 'G_ssim_backward'), 0.0, 2.0)


def test_the_flag_adds_its_terms_and_weight_zero_is_the_run_without_it(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    plain = _train(tmp_path, capsys, 'plain', 3, ['--resumable'])
    zero = _train(tmp_path, capsys, 'zero', 3, ['--resumable', '--ssim_weight', '0'])
    on = _train(tmp_path, capsys, 'on', 3, ['--ssim_weight', '0.2'])
    assert 'G_ssim' not in plain and 'G_ssim' not in zero
    assert len(_states(plain)) == 3 and _states(plain) == _states(zero)
    print(_terms(on, 3))
    a, b = _generator(tmp_path, 'plain'), _generator(tmp_path, 'on')
    assert list(a) == list(b)
    assert any(not torch.equal(a[k], b[k]) for k in a)
    assert all(torch.isfinite(v).all() for v in b.values() if v.is_floating_point())


@pytest.mark.parametrize('extra', [[], ['--guard', '--clip_grad_norm', '1', '--fused_step', '--ema_decay', '0.99']],
                         ids=['resumable', 'guard_fused_ema'])
def test_straight_against_split_with_the_term(tmp_path, capsys, monkeypatch, extra):
    monkeypatch.chdir(tmp_path)
    kit.check_straight_against_split(tmp_path, capsys, ['--resumable', '--ssim_weight', '0.2'] + extra, _terms)


def test_graph_step_with_the_term(tmp_path, capsys, monkeypatch):
    """Updates 1-2 eager, 3 captured and replayed, 4 replayed: the launch is part of the captured update."""
    monkeypatch.chdir(tmp_path)
    kit.check_graph_step(tmp_path, capsys, ['--ssim_weight', '0.2'], _terms, changing=('G_ssim',))
