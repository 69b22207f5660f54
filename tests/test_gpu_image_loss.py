"""The L2 / L1 / Charbonnier + gradient-difference image loss on the GPU (csrc/image_loss.hip.inc through the C ABI and losses.ImageLoss)
against the numpy restatement of its definition (image_loss_ref.py): gradient bit for bit, plane sums and totals to 1e-12 relative (the
order of the sums is the kernel's) and bit for bit on grid inputs (every order is exact there); independent of npred, of the other
predictions, of the batch; reproducible, isolated from a non-finite plane, capturable; and train.py --image_loss with the other run options.
The tile is TH x TW = 16 x 64 pixels, a lane owns four of a row: sizes below run from 2 over one below / at / one above the tile to two
tiles and one pixel each way, with widths that are no multiple of 4 and planes of odd H * W (no 16-byte alignment)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_loss_ref as ref  # noqa: E402
import loss_kit as kit  # noqa: E402
from loss_kit import MCNET, _bits, _generator, _rel, _states, _train  # noqa: E402

from video_frame_inpainting_amd import _native  # noqa: E402
from video_frame_inpainting_amd.losses import ImageLoss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TH, TW = 16, 64                 # csrc/image_loss.hip.inc
GRID_CAP = 1 << 20              # workgroups per launch; past it a workgroup strides over the tiles
EPS = 1e-3

# (P, H, W): H from {2, 3, TH - 1, TH, TH + 1, 2 TH + 1}, W from {2, 3, TW - 1, TW, TW + 1, 2 TW + 1}, P from {1, 3, 15}; 41 x 17 (odd H * W);
# 128 x 128
CASES = [(1, 2, 2), (3, 3, 3), (15, 2, TW - 1), (1, TH - 1, TW), (3, TH, TW + 1), (15, TH + 1, 2 * TW + 1), (1, 2 * TH + 1, 2), (3, 2 * TH + 1, TW - 1),
         (15, TH, 3), (1, TH + 1, TW), (3, 2, 2 * TW + 1), (1, 3, TW + 1), (3, TH - 1, 3), (1, 2 * TH + 1, 2 * TW + 1), (15, 41, 17), (3, 128, 128)]


@functools.lru_cache(maxsize=None)
def _case(inputs, shape, kind, seed=0):
    """(pred, gt, restatement) for a seeded input; computed once, shared, never written to."""
    pred, gt = ref.make_pair(inputs, shape, 211 + seed + 7 * shape[-1] + shape[-2])
    want = ref.image_loss_ref(pred, gt, kind, EPS)
    for a in (pred, gt, want['grad'], want['plane_terms']):
        a.setflags(write=False)
    return pred, gt, want


def _launch(preds, gt, kind, eps=EPS, grads=True):
    """tai_image_loss through the C ABI -> (plane_terms [n, P, 2] float64, totals [n, 3] float64, [grad float32 or None per prediction]),
    numpy.  ``grads``: True, False (a NULL table) or one bool per prediction (NULL entries).  Every output is pre-filled."""
    L = _native.lib()
    n = len(preds)
    H, W = gt.shape[-2:]
    P = gt.size // (H * W)
    nbytes = L.tai_image_loss_workspace_bytes(n, P, H, W)
    assert nbytes > 0 and nbytes % 16 == 0
    ps = [torch.from_numpy(np.array(p)).to(DEV) for p in preds]
    g = torch.from_numpy(np.array(gt)).to(DEV)
    ws = torch.full((nbytes // 8,), float('nan'), dtype=torch.float64, device=DEV)
    planes = torch.full((n, P, 2), -7.0, dtype=torch.float64, device=DEV)
    totals = torch.full((n, 3), -7.0, dtype=torch.float64, device=DEV)
    mask = [bool(grads)] * n if isinstance(grads, bool) else list(grads)
    maps = [torch.full(gt.shape, float('nan'), dtype=torch.float32, device=DEV) if m else None for m in mask]
    pred_ptrs = (ctypes.c_void_p * n)(*[p.data_ptr() for p in ps])
    map_ptrs = (ctypes.c_void_p * n)(*[m.data_ptr() if m is not None else None for m in maps]) if grads is not False else None
    rc = L.tai_image_loss(pred_ptrs, n, g.data_ptr(), kind, eps, planes.data_ptr(), totals.data_ptr(), map_ptrs, ws.data_ptr(), P, H, W,
                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.tai_sepconv_last_error()
    torch.cuda.synchronize()
    return planes.cpu().numpy(), totals.cpu().numpy(), [m.cpu().numpy() if m is not None else None for m in maps]


def _compare(planes, totals, grad, want, exact, what):
    """One prediction's outputs against the restatement; ``exact``: the sums are order-independent (grid inputs, P H W <= 2^18)."""
    wrong = int(np.count_nonzero(_bits(grad) != _bits(want['grad'])))
    d_plane = _rel(planes, want['plane_terms'])
    d_tot = _rel(totals, [want['point'], want['gdl'], want['loss']])
    print('%s: %d of %d gradient words differ; plane_terms rel %.2e; totals %s rel %.2e' % (what, wrong, grad.size, d_plane, totals, d_tot))
    assert wrong == 0
    assert d_plane <= 1e-12 and d_tot <= 1e-12
    if exact:
        assert np.array_equal(_bits(planes), _bits(want['plane_terms']))
        assert np.array_equal(_bits(totals), _bits(np.array([want['point'], want['gdl'], want['loss']])))
    assert totals[2] == totals[0] + totals[1]


@pytest.mark.parametrize('kind', [0, 1, 2], ids=ref.KIND_NAMES)
@pytest.mark.parametrize('shape', CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_and_module_match_the_restatement(shape, kind):
    assert shape[0] * shape[1] * shape[2] <= 1 << 18
    for inputs in ref.KINDS:
        pred, gt, want = _case(inputs, shape, kind)
        planes, totals, (grad,) = _launch([pred], gt, kind)
        _compare(planes[0], totals[0], grad, want, inputs == 'grid', '%s %s kind %d' % (inputs, shape, kind))
    # the module: the same launch behind autograd (the last input kind: grid)
    p = torch.from_numpy(np.array(pred)).to(DEV).requires_grad_()
    module = ImageLoss(ref.KIND_NAMES[kind], EPS)
    loss = module(p, torch.from_numpy(np.array(gt)).to(DEV))
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    loss.backward()
    assert float(loss.detach()) == float(np.float32(totals[0][2]))
    assert np.array_equal(_bits(p.grad.cpu().numpy()), _bits(grad))
    assert np.array_equal(_bits(module.plane_terms.cpu().numpy()), _bits(planes))
    (point, gdl), = module.last_terms
    assert float(point) == float(np.float32(totals[0][0])) and float(gdl) == float(np.float32(totals[0][1])) and not point.requires_grad


def test_one_tile_past_the_grid_cap_makes_a_second_pass():
    shape = (GRID_CAP + 1, 2, 2)                                  # one tile per plane: the first workgroup takes a second tile
    pred, gt, want = _case('uniform', shape, 2)
    planes, totals, (grad,) = _launch([pred], gt, 2)
    _compare(planes[0], totals[0], grad, want, False, 'uniform %s' % (shape,))
    assert np.array_equal(_bits(planes[0][[0, -1]]), _bits(want['plane_terms'][[0, -1]]))          # four terms each: any order is exact


def test_a_launch_of_three_gives_each_prediction_the_bits_of_its_own_launch():
    shape = (3, 41, 17)
    for kind in (0, 1, 2):
        cases = [_case(inputs, shape, kind, seed) for seed, inputs in enumerate(('uniform', 'smooth', 'wide'))]
        gt = cases[0][1]
        preds = [c[0] for c in cases]
        alone = [_launch([p], gt, kind) for p in preds]
        for i, p in enumerate(preds):                                   # (each against the restatement with the shared gt)
            _compare(alone[i][0][0], alone[i][1][0], alone[i][2][0], ref.image_loss_ref(p, gt, kind, EPS), False, 'alone %d' % i)
        together = _launch(preds, gt, kind)
        again = _launch(preds, gt, kind)
        some = _launch(preds, gt, kind, grads=[False, True, False])
        none = _launch(preds, gt, kind, grads=False)
        for i in range(3):
            for run in (together, again, some, none):
                assert np.array_equal(_bits(run[0][i]), _bits(alone[i][0][0])) and np.array_equal(_bits(run[1][i]), _bits(alone[i][1][0]))
            assert np.array_equal(_bits(together[2][i]), _bits(alone[i][2][0])) and np.array_equal(_bits(again[2][i]), _bits(alone[i][2][0]))
        assert some[2][0] is None and some[2][2] is None and np.array_equal(_bits(some[2][1]), _bits(alone[1][2][0]))
        two = _launch(preds[:2], gt, kind)
        assert all(np.array_equal(_bits(two[2][i]), _bits(alone[i][2][0])) and np.array_equal(_bits(two[0][i]), _bits(alone[i][0][0]))
                   for i in range(2))


def test_a_plane_does_not_depend_on_its_batch():
    shape5 = (5, 41, 17)
    for kind in (0, 2):
        pred5, gt5, want5 = _case('smooth', shape5, kind)
        planes5, _, (grad5,) = _launch([pred5], gt5, kind)
        assert np.array_equal(_bits(grad5), _bits(want5['grad']))
        for n in (0, 3):
            pred1, gt1 = pred5[n:n + 1], gt5[n:n + 1]
            want1 = ref.image_loss_ref(pred1, gt1, kind, EPS)
            planes1, _, (grad1,) = _launch([pred1], gt1, kind)
            assert np.array_equal(_bits(grad1), _bits(want1['grad']))                 # each P through the restatement, bit for bit
            assert np.array_equal(_bits(planes1[0, 0]), _bits(planes5[0, n]))


def test_a_nan_stays_in_its_plane():
    shape = (15, 17, 65)
    for kind in (0, 1, 2):
        pred, gt, _ = _case('uniform', shape, kind)
        clean_planes, _, (clean_grad, _) = _launch([pred, pred], gt, kind, grads=[True, False])
        dirty = np.array(pred)
        dirty[7, 9, 63] = np.nan                                                      # the last column of a tile: its neighbour is the next tile's
        planes, totals, (grad, _) = _launch([dirty, pred], gt, kind, grads=[True, False])
        keep = np.ones(15, bool)
        keep[7] = False
        assert np.array_equal(_bits(planes[0][keep]), _bits(clean_planes[0][keep]))
        assert np.isnan(planes[0][7]).all() and not np.isfinite(totals[0]).any()
        assert np.array_equal(_bits(planes[1]), _bits(clean_planes[1])) and np.isfinite(totals[1]).all()      # the other prediction
        assert np.isfinite(grad[keep]).all() and np.array_equal(_bits(grad[keep]), _bits(clean_grad[keep]))
        bad = np.argwhere(np.isnan(grad[7]))
        assert sorted(map(tuple, bad)) == [(8, 63), (9, 62), (9, 63), (9, 64), (10, 63)]                    # the pixel and its four neighbours


def _refused(L, *args):
    rc = L.tai_image_loss(*args)
    message = L.tai_sepconv_last_error()
    assert rc != 0 and message.startswith(b'image_loss:'), (rc, message)
    return message


def test_every_refusal_returns_an_error_and_launches_nothing():
    L = _native.lib()
    x = torch.zeros(2, 8, 8, device=DEV)
    out = torch.full((64,), -7.0, dtype=torch.float64, device=DEV)
    ws = torch.full((64,), -7.0, dtype=torch.float64, device=DEV)
    ptrs = (ctypes.c_void_p * 3)(x.data_ptr(), x.data_ptr(), x.data_ptr())
    hole = (ctypes.c_void_p * 3)(x.data_ptr(), None, x.data_ptr())
    s = torch.cuda.current_stream().cuda_stream
    xp, planes, totals, w = x.data_ptr(), out.data_ptr(), out[32:].data_ptr(), ws.data_ptr()
    assert L.tai_image_loss(ptrs, 1, xp, 2, EPS, planes, totals, None, w, 2, 8, 8, s) == 0
    torch.cuda.synchronize()
    out.fill_(-7.0)
    ws.fill_(-7.0)
    assert b'null' in _refused(L, None, 1, xp, 0, EPS, planes, totals, None, w, 2, 8, 8, s)
    assert b'null' in _refused(L, hole, 3, xp, 0, EPS, planes, totals, None, w, 2, 8, 8, s)
    assert b'null' in _refused(L, ptrs, 1, None, 0, EPS, planes, totals, None, w, 2, 8, 8, s)
    assert b'null' in _refused(L, ptrs, 1, xp, 0, EPS, None, totals, None, w, 2, 8, 8, s)
    assert b'null' in _refused(L, ptrs, 1, xp, 0, EPS, planes, None, None, w, 2, 8, 8, s)
    assert b'null' in _refused(L, ptrs, 1, xp, 0, EPS, planes, totals, None, None, 2, 8, 8, s)
    for npred in (0, 4, -1):
        assert b'npred' in _refused(L, ptrs, npred, xp, 0, EPS, planes, totals, None, w, 2, 8, 8, s)
        assert L.tai_image_loss_workspace_bytes(npred, 2, 8, 8) < 0
    for kind in (-1, 3):
        assert b'kind' in _refused(L, ptrs, 1, xp, kind, EPS, planes, totals, None, w, 2, 8, 8, s)
    for eps in (0.0, -1.0, float('nan'), float('inf')):
        assert b'eps' in _refused(L, ptrs, 1, xp, 2, eps, planes, totals, None, w, 2, 8, 8, s)
        assert L.tai_image_loss(ptrs, 1, xp, 0, eps, planes, totals, None, w, 2, 8, 8, s) == 0          # only Charbonnier reads it
    torch.cuda.synchronize()
    out.fill_(-7.0)
    ws.fill_(-7.0)
    for P, H, W, word in ((0, 8, 8, b'plane'), (2, 1, 8, b'H, W >= 2'), (2, 8, 1, b'H, W >= 2'), (1 << 38, 2, 2, b'too large'),
                          (1, 1 << 16, 1 << 15, b'too large'), (1 << 31, 2, 2, b'tiles')):
        assert word in _refused(L, ptrs, 1, xp, 0, EPS, planes, totals, None, w, P, H, W, s)
        assert L.tai_image_loss_workspace_bytes(1, P, H, W) < 0
    assert b'aligned' in _refused(L, ptrs, 1, xp, 0, EPS, planes + 4, totals, None, w, 2, 8, 8, s)
    assert b'aligned' in _refused(L, ptrs, 1, xp, 0, EPS, planes, totals + 4, None, w, 2, 8, 8, s)
    assert b'aligned' in _refused(L, ptrs, 1, xp, 0, EPS, planes, totals, None, w + 4, 2, 8, 8, s)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((ws == -7.0).all())                                     # nothing was launched
    # the module
    for shape in ((2, 1, 8), (2, 8, 1)):
        z = torch.zeros(shape, device=DEV)
        with pytest.raises(ValueError):
            ImageLoss()(z, z)
    with pytest.raises(ValueError):
        ImageLoss()(torch.zeros(2, 8, 8, device=DEV), torch.zeros(2, 8, 9, device=DEV))
    with pytest.raises(ValueError):
        ImageLoss()((x, torch.zeros(2, 8, 9, device=DEV)), x)


def test_autograd_scales_the_maps_takes_a_permuted_view_and_writes_nothing_under_no_grad(monkeypatch):
    shape = (2, 3, 17, 41)
    cases = [_case(inputs, shape, 2, seed) for seed, inputs in enumerate(('smooth', 'uniform', 'grid'))]
    gt = cases[0][1]
    wants = [ref.image_loss_ref(c[0], gt, 2, EPS) for c in cases]
    ps = tuple(torch.from_numpy(np.array(c[0])).to(DEV).requires_grad_() for c in cases)
    g = torch.from_numpy(np.array(gt)).to(DEV).requires_grad_()
    module = ImageLoss('charbonnier', EPS)
    a, b, c = module(ps, g)
    assert module.plane_terms.shape == (3, 6, 2) and len(module.last_terms) == 3
    (0.2 * a + 3.0 * b + c).backward()
    for p, want, scale in zip(ps, wants, (0.2, 3.0, 1.0)):
        assert np.array_equal(_bits(p.grad.cpu().numpy()), _bits(np.float32(scale) * want['grad']))      # one fp32 product
        assert p.grad.shape == p.shape
    assert g.grad is None
    # a permuted view [3, 2, H, W] of a [2, 3, H, W] tensor against its contiguous copy
    base = torch.from_numpy(np.array(cases[0][0])).to(DEV)
    view = base.permute(1, 0, 2, 3).requires_grad_()
    copy = base.permute(1, 0, 2, 3).contiguous().requires_grad_()
    assert not view.is_contiguous()
    gv = g.detach().permute(1, 0, 2, 3)
    lv, lc = ImageLoss('l1')(view, gv), ImageLoss('l1')(copy, gv.contiguous())
    lv.backward()
    lc.backward()
    assert float(lv.detach()) == float(lc.detach())
    assert torch.equal(view.grad.view(torch.int32), copy.grad.view(torch.int32)) and view.grad.shape == view.shape
    # under no_grad (and for a prediction that asks for no gradient) the launch gets no gradient buffer
    L = _native.lib()
    seen = []
    real = L.tai_image_loss

    def spy(preds, n, gt_, kind, eps, planes, totals, grads, *rest):
        seen.append([grads[i] for i in range(n)])
        return real(preds, n, gt_, kind, eps, planes, totals, grads, *rest)
    monkeypatch.setattr(L, 'tai_image_loss', spy)
    with torch.no_grad():
        quiet = ImageLoss('charbonnier', EPS)(ps, g)
    assert seen[-1] == [None, None, None] and not any(q.requires_grad for q in quiet)
    assert [float(q) for q in quiet] == [float(a.detach()), float(b.detach()), float(c.detach())]
    ImageLoss('charbonnier', EPS)((ps[0], ps[1].detach()), g)
    assert seen[-1][0] is not None and seen[-1][1] is None


def test_forward_and_backward_replay_inside_one_graph():
    shape = (2, 1, 32, 32)
    first = [_case(inputs, shape, 2, 1 + i) for i, inputs in enumerate(('smooth', 'uniform', 'wide'))]
    second = [_case(inputs, shape, 2, 5 + i) for i, inputs in enumerate(('uniform', 'grid', 'smooth'))]
    sp = [torch.from_numpy(np.array(c[0])).to(DEV).requires_grad_() for c in first]
    sg = torch.from_numpy(np.array(first[0][1])).to(DEV)
    gt2 = second[0][1]
    kit.check_graph_replay(lambda: ImageLoss('charbonnier', EPS), sp, sg, [c[0] for c in second], gt2,
                           [ref.image_loss_ref(c[0], gt2, 2, EPS)['grad'] for c in second])


# ---------------------------------------------------------------------------------------------------------------- drivers

TAI_KEYS = ('G_Lp', 'G_gdl', 'G_Lp_forward', 'G_gdl_forward', 'G_Lp_backward', 'G_gdl_backward')


def _terms(out, n, keys=TAI_KEYS):
    """{key: [value per printed update]}; asserts each key is printed on every line, finite and positive."""
    return kit._terms(out, n, keys, 0.0, float('inf'))


def test_l2_is_the_run_without_the_flag_and_the_other_kinds_train_on_their_terms(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    plain = _train(tmp_path, capsys, 'plain', 3, ['--resumable'])
    l2 = _train(tmp_path, capsys, 'l2', 3, ['--resumable', '--image_loss', 'l2'])
    assert len(_states(plain)) == 3 and _states(plain) == _states(l2)
    assert _terms(plain, 3) == _terms(l2, 3)
    a = _generator(tmp_path, 'plain')
    for kind in ('charbonnier', 'l1'):
        out = _train(tmp_path, capsys, kind, 3, ['--image_loss', kind])
        terms = _terms(out, 3)
        print(kind, terms)
        assert terms['G_Lp'] != _terms(plain, 3)['G_Lp']
        b = _generator(tmp_path, kind)
        assert list(a) == list(b)
        assert any(not torch.equal(a[k], b[k]) for k in a)
        assert all(torch.isfinite(v).all() for v in b.values() if v.is_floating_point())


@pytest.mark.parametrize('extra', [[], ['--guard', '--clip_grad_norm', '1', '--fused_step', '--ema_decay', '0.99', '--ssim_weight', '0.2']],
                         ids=['resumable', 'guard_fused_ema_ssim'])
def test_straight_against_split_with_the_charbonnier_term(tmp_path, capsys, monkeypatch, extra):
    monkeypatch.chdir(tmp_path)
    kit.check_straight_against_split(tmp_path, capsys, ['--resumable', '--image_loss', 'charbonnier'] + extra, _terms)


def test_graph_step_with_the_charbonnier_term(tmp_path, capsys, monkeypatch):
    """Updates 1-2 eager, 3 captured and replayed, 4 replayed: the launch is part of the captured update."""
    monkeypatch.chdir(tmp_path)
    kit.check_graph_step(tmp_path, capsys, ['--image_loss', 'charbonnier'], _terms, replays_differ=True)


def test_mcnet_runs_with_one_prediction(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    L = _native.lib()
    seen = []
    real = L.tai_image_loss
    monkeypatch.setattr(L, 'tai_image_loss', lambda preds, n, *rest: seen.append(n) or real(preds, n, *rest))
    out = _train(tmp_path, capsys, 'm', 3, ['--image_loss', 'l1'], model=MCNET)
    print(_terms(out, 3, ('G_Lp', 'G_gdl')))
    assert 'G_Lp_forward' not in out and seen == [1, 1, 1]
    seen.clear()
    _train(tmp_path, capsys, 't', 2, ['--image_loss', 'l1'])
    assert seen == [3, 3]                                                             # bi-TAI: one launch per update for its three predictions
