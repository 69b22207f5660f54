"""The census (soft ternary) loss on the GPU (csrc/census_loss.hip.inc through the C ABI and losses.CensusLoss) against the numpy
restatement of its definition (census_loss_ref.py): gradient bit for bit, frame terms within (H-6)(W-6) 2^-53 relative and totals to
1e-12 (the order of the sum over a frame is the kernel's); the same bits from either storage layout, for any npred, batch and neighbour;
isolated from a non-finite frame, capturable; and train.py --census_weight with the other run options.  A workgroup owns a 32 x 32 tile of
the PLANE (not of the interior: border pixels have gradients too) and a lane four consecutive pixels of a row: the shapes below run from
one interior pixel over one-row and one-column interiors, odd planes (no 16-byte alignment, rows that end inside a run), exactly one
tile, a one-pixel second tile each way and three tiles across with outliers on every seam to a base one element off alignment and one
tile past the grid cap."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import census_loss_ref as ref  # noqa: E402
import loss_kit as kit  # noqa: E402
from loss_kit import MCNET, _bits, _generator, _rel, _states, _train  # noqa: E402

from video_frame_inpainting_amd import _native  # noqa: E402
from video_frame_inpainting_amd.losses import CensusLoss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TH = TW = 32                    # the kernel's tile of the plane (csrc/census_loss.hip.inc; test_census_loss_cpu.py holds them to the source)
GRID_CAP = 1 << 14              # workgroups per launch; past it a workgroup strides over the tiles

# (B, T, C, H, W): one interior pixel (48 pixels get their gradient through the neighbour term alone); a one-row and a one-column interior;
# the first size with a pixel whose 48 neighbours are all interior; the gray path on an odd plane with W % 4 != 0; exactly one tile; a
# one-pixel second tile each way; the same two for a tiling of the interior (th + 6, th + 7)
CASES = [(1, 1, 1, 7, 7), (1, 2, 1, 7, 12), (1, 1, 1, 12, 7), (2, 2, 1, 13, 13), (1, 2, 3, 9, 11), (1, 1, 1, TH, TW), (1, 1, 3, TH + 1, TW + 1),
         (1, 1, 1, TH + 6, TW + 6), (1, 1, 1, TH + 7, TW + 7)]
SEAMS = (1, 1, 1, TH + 8, 3 * TW)          # three tiles across, two down


@functools.lru_cache(maxsize=None)
def _case(inputs, shape, seed=0, outliers=False):
    """(pred, gt, restatement) for a seeded input; computed once, shared, never written to.  ``outliers``: +-4 in both tensors on both
    sides of every tile seam."""
    pred, gt = ref.make_pair(inputs, shape, 523 + seed + 7 * shape[-1] + shape[-2] + 3 * shape[1])
    if outliers:
        H, W = shape[-2:]
        for a, sign in ((pred, 1.0), (gt, -1.0)):
            for c in range(TW, W, TW):
                a[..., 1::3, c - 1] = 4.0 * sign
                a[..., 2::3, c] = -4.0 * sign
            for r in range(TH, H, TH):
                a[..., r - 1, 1::3] = -4.0 * sign
                a[..., r, 0::3] = 4.0 * sign
    want = ref.census_loss_ref(pred, gt)
    for a in (pred, gt, want['grad'], want['frame_terms']):
        a.setflags(write=False)
    return pred, gt, want


def _store(a, layout, fill=None):
    """A device tensor that reads as ``a`` [B, T, C, H, W] (or, with ``fill``, holds that value), stored as ``layout`` says: 'bt' =
    contiguous, 'tb' = time-major (a transposed view, what tai.py returns for ``pred``), 'off' = contiguous inside a buffer, one element
    past its 16-byte aligned base.  -> (view, (batch stride, time stride))."""
    B, T, C, H, W = a.shape
    chw = C * H * W
    src = torch.from_numpy(np.array(a))
    if layout == 'bt':
        t, strides = torch.empty(a.shape, device=DEV), (T * chw, chw)
    elif layout == 'tb':
        t, strides = torch.empty((T, B, C, H, W), device=DEV).transpose(0, 1), (chw, B * chw)
    else:
        buf = torch.empty(a.size + 4, device=DEV)
        assert buf.data_ptr() % 16 == 0
        t, strides = buf[1:1 + a.size].view(a.shape), (T * chw, chw)
        assert t.data_ptr() % 16 == 4
    if fill is None:
        t.copy_(src)
    else:
        t.fill_(fill)
    return t, strides


def _launch(preds, gt, grads=True, layouts=None, gt_layout='bt'):
    """tai_census_loss through the C ABI -> (frame_terms [n, B * T] float64, totals [n] float64, [grad float32 [B, T, C, H, W] or None
    per prediction]), numpy.  ``grads``: True, False (a NULL table) or one bool per prediction (NULL entries); ``layouts``: one of 'bt',
    'tb', 'off' per prediction.  Every output is pre-filled and the workspace is NaN."""
    L = _native.lib()
    n = len(preds)
    B, T, C, H, W = gt.shape
    layouts = layouts or ['bt'] * n
    nbytes = L.tai_census_loss_workspace_bytes(n, B, T, C, H, W)
    assert nbytes == n * B * T * (-(-H // TH)) * (-(-W // TW)) * 8
    stored = [_store(p, l) for p, l in zip(preds, layouts)]
    g, g_strides = _store(gt, gt_layout)
    ws = torch.full((nbytes // 8,), float('nan'), dtype=torch.float64, device=DEV)
    frames = torch.full((n, B * T), -7.0, dtype=torch.float64, device=DEV)
    totals = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
    mask = [bool(grads)] * n if isinstance(grads, bool) else list(grads)
    maps = [_store(p, l, fill=float('nan'))[0] if m else None for p, l, m in zip(preds, layouts, mask)]
    pred_ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t, _ in stored])
    map_ptrs = (ctypes.c_void_p * n)(*[m.data_ptr() if m is not None else None for m in maps]) if grads is not False else None
    table = (ctypes.c_longlong * (2 * n + 2))(*([v for _, st in stored for v in st] + list(g_strides)))
    rc = L.tai_census_loss(pred_ptrs, n, g.data_ptr(), table, frames.data_ptr(), totals.data_ptr(), map_ptrs, ws.data_ptr(),
                           B, T, C, H, W, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.tai_sepconv_last_error()
    torch.cuda.synchronize()
    return frames.cpu().numpy(), totals.cpu().numpy(), [m.cpu().contiguous().numpy() if m is not None else None for m in maps]


def _compare(frames, total, grad, want, what):
    """One prediction's outputs against the restatement."""
    H, W = want['grad'].shape[-2:]
    wrong = int(np.count_nonzero(_bits(grad) != _bits(want['grad'])))
    bound = (H - 6) * (W - 6) * 2.0 ** -53
    d_frames, d_total = _rel(frames, want['frame_terms']), _rel(total, want['loss'])
    print('%s: %d of %d gradient words differ; frame_terms rel %.2e (bound %.2e); total rel %.2e' % (what, wrong, grad.size, d_frames, bound, d_total))
    assert wrong == 0
    assert d_frames <= bound and d_total <= 1e-12


def _module_matches(p, g, frames, totals, grad, want):
    """losses.CensusLoss on the device tensors ``p``, ``g`` (in whatever layout they lie) against one launch's outputs and the
    restatement: the fp32 scalar, the gradient map and frame_terms, bit for bit."""
    p = p.requires_grad_()
    module = CensusLoss()
    loss = module(p, g)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    loss.backward()
    got = float(loss.detach())
    assert got == float(np.float32(totals[0])) or (np.isnan(got) and np.isnan(totals[0]))
    assert abs(got - want['loss']) <= 2.0 ** -23 * abs(want['loss'])                  # one rounding of a value within 1e-12 of it
    assert np.array_equal(_bits(p.grad.cpu().contiguous().numpy()), _bits(grad)) and np.array_equal(_bits(grad), _bits(want['grad']))
    assert np.array_equal(_bits(module.frame_terms.cpu().numpy()), _bits(frames)) and not module.frame_terms.requires_grad


@pytest.mark.parametrize('shape', CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_and_module_match_the_restatement(shape):
    for inputs in ref.KINDS:
        pred, gt, want = _case(inputs, shape)
        frames, totals, (grad,) = _launch([pred], gt)
        _compare(frames[0], totals[0], grad, want, '%s %s' % (inputs, shape))
        if inputs in ('equal', 'flat'):
            assert not grad.any() and totals[0] == 0.0 and not frames.any()
        _module_matches(torch.from_numpy(np.array(pred)).to(DEV), torch.from_numpy(np.array(gt)).to(DEV), frames, totals, grad, want)


def test_three_tiles_across_with_outliers_on_every_seam():
    for inputs in ('uniform', 'smooth'):
        pred, gt, want = _case(inputs, SEAMS, outliers=True)
        assert np.abs(pred).max() == 4.0 and np.abs(gt).max() == 4.0
        frames, totals, (grad,) = _launch([pred], gt)
        _compare(frames[0], totals[0], grad, want, '%s %s with outliers' % (inputs, SEAMS))


def test_a_base_one_element_off_alignment(monkeypatch):
    """W % 4 == 0, but no run of the tensor starts at a multiple of 16 bytes: single words for that tensor alone.  Kernel and module; the
    module gets the slice itself (a spy sees its pointer: no copy was made to realign it)."""
    L = _native.lib()
    seen = []
    real = L.tai_census_loss
    monkeypatch.setattr(L, 'tai_census_loss', lambda preds, n, gt_, *rest: seen.append((preds[0], gt_)) or real(preds, n, gt_, *rest))
    for shape, inputs in (((2, 2, 3, 16, 40), 'uniform'), ((1, 2, 1, 40, 36), 'smooth')):
        pred, gt, want = _case(inputs, shape)
        aligned = _launch([pred], gt)
        for layouts, gt_layout in ((['off'], 'bt'), (['bt'], 'off'), (['off'], 'off')):
            frames, totals, (grad,) = _launch([pred], gt, layouts=layouts, gt_layout=gt_layout)
            _compare(frames[0], totals[0], grad, want, '%s pred %s gt %s' % (inputs, layouts[0], gt_layout))
            assert np.array_equal(_bits(frames), _bits(aligned[0])) and np.array_equal(_bits(totals), _bits(aligned[1]))
        p, g = _store(pred, 'off')[0], _store(gt, 'off')[0]
        _module_matches(p, g, aligned[0], aligned[1], aligned[2][0], want)
        assert seen[-1] == (p.data_ptr(), g.data_ptr())


def test_one_tile_past_the_grid_cap_makes_a_second_pass():
    shape = (GRID_CAP + 1, 1, 1, 7, 7)                            # one tile per frame: the first workgroup takes a second tile
    pred, gt, want = _case('uniform', shape)
    frames, totals, (grad,) = _launch([pred], gt)
    _compare(frames[0], totals[0], grad, want, 'uniform %s' % (shape,))


def test_either_storage_gives_the_same_bits_and_the_view_is_read_where_it_lies(monkeypatch):
    shape = (3, 4, 1, 17, 38)
    pred, gt, want = _case('smooth', shape)
    bt = _launch([pred], gt)
    for layouts, gt_layout in ((['tb'], 'bt'), (['bt'], 'tb'), (['tb'], 'tb')):
        frames, totals, (grad,) = _launch([pred], gt, layouts=layouts, gt_layout=gt_layout)
        _compare(frames[0], totals[0], grad, want, 'pred %s gt %s' % (layouts[0], gt_layout))
        assert np.array_equal(_bits(frames), _bits(bt[0])) and np.array_equal(_bits(totals), _bits(bt[1]))
    # the module: tai.py's ``pred`` is a transposed view of a [T * B, ...] buffer; its data_ptr and strides are what the launch gets
    B, T, C, H, W = shape
    chw = C * H * W
    stored = torch.from_numpy(np.array(pred)).to(DEV).transpose(0, 1).contiguous().view(T * B, C, H, W)
    view = stored.view(T, B, C, H, W).transpose(0, 1).requires_grad_()
    copy = view.detach().contiguous().requires_grad_()
    g = torch.from_numpy(np.array(gt)).to(DEV)
    assert not view.is_contiguous() and view.data_ptr() == stored.data_ptr()
    L = _native.lib()
    seen = []
    real = L.tai_census_loss

    def spy(preds, n, gt_, strides, frames, totals, grads, *rest):
        seen.append(([preds[i] for i in range(n)], gt_, [strides[i] for i in range(2 * n + 2)], [grads[i] for i in range(n)]))
        return real(preds, n, gt_, strides, frames, totals, grads, *rest)
    monkeypatch.setattr(L, 'tai_census_loss', spy)
    lv = CensusLoss()(view, g)
    lc = CensusLoss()(copy, g)
    assert seen[0][0] == [stored.data_ptr()] and seen[0][1] == g.data_ptr() and seen[0][2] == [chw, B * chw, T * chw, chw]
    assert seen[1][0] == [copy.data_ptr()] and seen[1][2] == [T * chw, chw, T * chw, chw]
    (3.0 * lv).backward()
    (3.0 * lc).backward()
    assert float(lv.detach()) == float(lc.detach()) == float(np.float32(bt[1][0]))
    assert view.grad.shape == view.shape and view.grad.stride() == view.stride()              # the map in the view's own layout
    assert torch.equal(view.grad.view(torch.int32), copy.grad.view(torch.int32))
    assert np.array_equal(_bits(copy.grad.cpu().numpy()), _bits(np.float32(3.0) * want['grad']))          # backward scales the map: one fp32 product
    # a tensor whose blocks are not dense is made contiguous first; no_grad and a detached prediction get no map
    wide = torch.zeros(B, T, C, H, W + 2, device=DEV)
    wide[..., :W] = view.detach()
    seen.clear()
    with torch.no_grad():
        quiet = CensusLoss()((wide[..., :W], view), g)
    assert seen[0][0][0] != wide.data_ptr() and seen[0][0][1] == stored.data_ptr() and seen[0][3] == [None, None]
    assert seen[0][2] == [T * chw, chw, chw, B * chw, T * chw, chw]
    assert float(quiet[0]) == float(quiet[1]) == float(lv.detach()) and not quiet[0].requires_grad
    CensusLoss()((view, copy.detach()), g)
    assert seen[1][3][0] is not None and seen[1][3][1] is None


def test_a_launch_of_three_gives_each_prediction_the_bits_of_its_own_launch():
    shape = (2, 3, 3, 9, 37)
    cases = [_case(inputs, shape, seed) for seed, inputs in enumerate(('uniform', 'smooth', 'wide'))]
    gt = cases[0][1]
    preds = [c[0] for c in cases]
    alone = [_launch([p], gt) for p in preds]
    for i, p in enumerate(preds):                                       # (each against the restatement with the shared gt)
        _compare(alone[i][0][0], alone[i][1][0], alone[i][2][0], ref.census_loss_ref(p, gt), 'alone %d' % i)
    together = _launch(preds, gt, layouts=['tb', 'bt', 'bt'])
    swapped = _launch([preds[0], preds[0], preds[2]], gt)               # other neighbours
    some = _launch(preds, gt, grads=[False, True, False])
    none = _launch(preds, gt, grads=False)
    for i in range(3):
        for run in (together, some, none):
            assert np.array_equal(_bits(run[0][i]), _bits(alone[i][0][0])) and np.array_equal(_bits(run[1][i]), _bits(alone[i][1][0]))
        assert np.array_equal(_bits(together[2][i]), _bits(alone[i][2][0]))
    for i in (0, 2):
        assert np.array_equal(_bits(swapped[2][i]), _bits(alone[i][2][0])) and np.array_equal(_bits(swapped[0][i]), _bits(alone[i][0][0]))
    assert some[2][0] is None and some[2][2] is None and np.array_equal(_bits(some[2][1]), _bits(alone[1][2][0]))
    assert none[2] == [None, None, None]
    two = _launch(preds[:2], gt)
    assert all(np.array_equal(_bits(two[2][i]), _bits(alone[i][2][0])) and np.array_equal(_bits(two[0][i]), _bits(alone[i][0][0]))
               for i in range(2))


def test_a_frame_depends_on_its_own_pixels_and_a_nan_stays_in_its_frame():
    shape = (3, 2, 1, 35, 13)                                     # frames of two tiles
    pred, gt, want = _case('smooth', shape)
    frames, totals, (grad, _) = _launch([pred, pred], gt, grads=[True, False])
    assert np.array_equal(_bits(grad), _bits(want['grad']))
    # a frame launched alone: count differs (kappa), so the restatement is asked again; its frame term keeps its bits
    one_p, one_g = pred[1:2, 1:2], gt[1:2, 1:2]
    f1, _, (g1,) = _launch([one_p], one_g)
    assert np.array_equal(_bits(g1), _bits(ref.census_loss_ref(one_p, one_g)['grad']))
    assert np.array_equal(_bits(f1[0]), _bits(frames[0][3:4]))
    # a NaN in frame (b, t) = (1, 1), number 3: only its terms, its gradients and the totals are non-finite
    dirty = np.array(pred)
    dirty[1, 1, 0, 20, 6] = np.nan
    d_frames, d_totals, (d_grad, _) = _launch([dirty, pred], gt, grads=[True, False])
    keep = np.ones(6, bool)
    keep[3] = False
    assert np.array_equal(_bits(d_frames[0][keep]), _bits(frames[0][keep])) and np.isnan(d_frames[0][3]) and np.isnan(d_totals[0])
    assert np.array_equal(_bits(d_frames[1]), _bits(frames[1])) and d_totals[1] == totals[1]              # the other prediction
    bad = np.isnan(d_grad)
    assert bad[1, 1].any() and not np.delete(bad.reshape(6, -1), 3, axis=0).any()
    assert np.array_equal(_bits(d_grad[~bad]), _bits(grad[~bad]))
    rows, cols = np.nonzero(bad[1, 1, 0])
    assert rows.min() == 17 and rows.max() == 23 and cols.min() == 3 and cols.max() == 9               # the pixel's own window
    # the other way round: every other frame of the batch is NaN, and frame 3 keeps its bits
    lonely = np.full_like(pred, np.nan)
    lonely[1, 1] = pred[1, 1]
    l_frames, l_totals, (l_grad,) = _launch([lonely], gt)
    assert np.array_equal(_bits(l_frames[0][3]), _bits(frames[0][3])) and np.isnan(l_frames[0][keep]).all() and np.isnan(l_totals[0])
    assert np.array_equal(_bits(l_grad[1, 1]), _bits(grad[1, 1])) and np.isnan(np.delete(l_grad.reshape(6, -1), 3, axis=0)).all()


def test_forward_and_backward_replay_inside_one_graph():
    shape = (2, 3, 1, 32, 40)
    first = [_case(inputs, shape, 1 + i) for i, inputs in enumerate(('smooth', 'uniform', 'wide'))]
    second = [_case(inputs, shape, 5 + i) for i, inputs in enumerate(('uniform', 'dyadic', 'smooth'))]
    sp = [_store(first[0][0], 'tb')[0].requires_grad_()] + [torch.from_numpy(np.array(c[0])).to(DEV).requires_grad_() for c in first[1:]]
    sg = torch.from_numpy(np.array(first[0][1])).to(DEV)
    gt2 = second[0][1]
    kit.check_graph_replay(CensusLoss, sp, sg, [c[0] for c in second], gt2, [ref.census_loss_ref(c[0], gt2)['grad'] for c in second])


# ---------------------------------------------------------------------------------------------------------------- drivers

TAI_KEYS = ('G_census', 'G_census_forward', 'G_census_backward')
EVERYTHING = ['--guard', '--clip_grad_norm', '1', '--fused_step', '--ema_decay', '0.99', '--ssim_weight', '0.2', '--image_loss', 'charbonnier',
              '--lap_weight', '0.5', '--temporal_weight', '0.5']


def _terms(out, n, keys=TAI_KEYS):
    """{key: [value per printed update]}; asserts each key is printed on every line, finite and inside (0, 1): phi < 1."""
    return kit._terms(out, n, keys, 0.0, 1.0)


def _spy(monkeypatch):
    L = _native.lib()
    seen = []
    real = L.tai_census_loss
    monkeypatch.setattr(L, 'tai_census_loss', lambda preds, n, *rest: seen.append(n) or real(preds, n, *rest))
    return seen


def test_the_keys_come_with_the_weight_and_weight_zero_is_the_run_without_the_flag(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    seen = _spy(monkeypatch)
    plain = _train(tmp_path, capsys, 'plain', 3, ['--resumable'])
    zero = _train(tmp_path, capsys, 'zero', 3, ['--resumable', '--census_weight', '0'])
    assert len(_states(plain)) == 3 and _states(plain) == _states(zero)
    assert 'G_census' not in plain and 'G_census' not in zero and seen == []
    out = _train(tmp_path, capsys, 'on', 3, ['--census_weight', '0.5'])
    found = _terms(out, 3)
    print(found)
    assert all(len(set(v)) > 1 for v in found.values())
    assert seen == [3, 3, 3]                                                          # bi-TAI: one launch per update for its three predictions
    a, b = _generator(tmp_path, 'plain'), _generator(tmp_path, 'on')
    assert list(a) == list(b) and any(not torch.equal(a[k], b[k]) for k in a)
    assert all(torch.isfinite(v).all() for v in b.values() if v.is_floating_point())


@pytest.mark.parametrize('extra', [[], EVERYTHING], ids=['resumable', 'guard_fused_ema_all_terms'])
def test_straight_against_split_with_the_census_term(tmp_path, capsys, monkeypatch, extra):
    monkeypatch.chdir(tmp_path)
    kit.check_straight_against_split(tmp_path, capsys, ['--resumable', '--census_weight', '0.5'] + extra, _terms)


def test_graph_step_with_the_census_term(tmp_path, capsys, monkeypatch):
    """Updates 1-2 eager, 3 captured and replayed, 4 replayed: the launch is part of the captured update."""
    monkeypatch.chdir(tmp_path)
    kit.check_graph_step(tmp_path, capsys, ['--census_weight', '0.5'], _terms, replays_differ=True)


def test_mcnet_runs_with_one_prediction(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    seen = _spy(monkeypatch)
    out = _train(tmp_path, capsys, 'm', 3, ['--census_weight', '0.5'], model=MCNET)
    print(_terms(out, 3, ('G_census',)))
    assert 'G_census_forward' not in out and seen == [1, 1, 1]
