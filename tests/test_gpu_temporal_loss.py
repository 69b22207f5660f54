"""The temporal-difference loss on the GPU (csrc/temporal_loss.hip.inc through the C ABI and losses.TemporalLoss) against the numpy
restatement of its definition (temporal_loss_ref.py): gradient bit for bit, sequence sums within H W 2^-53 relative and totals to 1e-12
(the order of the sums is the kernel's), everything bit for bit on grid inputs (every order is exact there); the same bits from either
storage layout, for any npred, batch and neighbour; reproducible, isolated from a non-finite sequence, capturable; and train.py
--temporal_weight with the other run options.  A lane owns a run of four pixels of a row and a workgroup a chunk of 256 runs of one
sequence: the shapes below run from one pixel over odd planes (no 16-byte alignment, rows that end inside a run) and more than one chunk
per sequence to a plane whose base is one element off alignment."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_loss_ref as ref  # noqa: E402
import loss_kit as kit  # noqa: E402
from loss_kit import MCNET, _bits, _generator, _rel, _states, _train  # noqa: E402

from video_frame_inpainting_amd import _native  # noqa: E402
from video_frame_inpainting_amd.losses import TemporalLoss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
THREADS = 256                   # runs of four pixels per chunk (csrc/temporal_loss.hip.inc; test_temporal_loss_cpu.py holds them to the source)
GRID_CAP = 1 << 20              # workgroups per launch; past it a workgroup strides over the chunks
EPS = 1e-3

# (B, T, C, H, W): one pixel; T = 1 (both seams on one frame); an odd plane (single-word loads and stores); ragged runs and two chunks per
# sequence (17 rows of 17 runs); whole 16-byte runs, C > 1; a long gap
CASES = [(1, 1, 1, 1, 1), (2, 1, 1, 2, 2), (1, 2, 3, 5, 7), (3, 5, 1, 17, 66), (2, 3, 3, 16, 64), (2, 10, 1, 8, 12)]


@functools.lru_cache(maxsize=None)
def _case(inputs, shape, kind, seed=0):
    """(pred, gt, restatement) for a seeded input; computed once, shared, never written to."""
    pred, gt = ref.make_pair(inputs, shape, 311 + seed + 7 * shape[-1] + shape[-2] + 3 * shape[1])
    want = ref.temporal_loss_ref(pred, gt, kind, EPS)
    for a in (pred, gt, want['grad'], want['seq_terms'], want['terms']):
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


def _launch(preds, gt, kind, eps=EPS, grads=True, layouts=None, gt_layout='bt'):
    """tai_temporal_loss through the C ABI -> (seq_terms [n, S, T + 1] float64, totals [n, T + 2] float64, [grad float32 [B, T, C, H, W] or
    None per prediction]), numpy.  ``grads``: True, False (a NULL table) or one bool per prediction (NULL entries); ``layouts``: one of
    'bt', 'tb', 'off' per prediction.  Every output is pre-filled."""
    L = _native.lib()
    n = len(preds)
    B, T, C, H, W = gt.shape
    S = B * C
    layouts = layouts or ['bt'] * n
    nbytes = L.tai_temporal_loss_workspace_bytes(n, B, T, C, H, W)
    assert nbytes > 0 and nbytes % 32 == 0
    stored = [_store(p, l) for p, l in zip(preds, layouts)]
    g, g_strides = _store(gt, gt_layout)
    ws = torch.full((nbytes // 8,), float('nan'), dtype=torch.float64, device=DEV)
    seqs = torch.full((n, S, T + 1), -7.0, dtype=torch.float64, device=DEV)
    totals = torch.full((n, T + 2), -7.0, dtype=torch.float64, device=DEV)
    mask = [bool(grads)] * n if isinstance(grads, bool) else list(grads)
    maps = [_store(p, l, fill=float('nan'))[0] if m else None for p, l, m in zip(preds, layouts, mask)]
    pred_ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t, _ in stored])
    map_ptrs = (ctypes.c_void_p * n)(*[m.data_ptr() if m is not None else None for m in maps]) if grads is not False else None
    table = (ctypes.c_longlong * (2 * n + 2))(*([v for _, st in stored for v in st] + list(g_strides)))
    rc = L.tai_temporal_loss(pred_ptrs, n, g.data_ptr(), table, kind, eps, seqs.data_ptr(), totals.data_ptr(), map_ptrs, ws.data_ptr(),
                             B, T, C, H, W, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.tai_sepconv_last_error()
    torch.cuda.synchronize()
    return seqs.cpu().numpy(), totals.cpu().numpy(), [m.cpu().contiguous().numpy() if m is not None else None for m in maps]


def _want_totals(want):
    return np.concatenate([want['terms'], [want['loss']]])


def _compare(seqs, totals, grad, want, exact, what):
    """One prediction's outputs against the restatement; ``exact``: the sums are order-independent (grid inputs, at most 2^18 terms)."""
    H, W = want['grad'].shape[-2:]
    wrong = int(np.count_nonzero(_bits(grad) != _bits(want['grad'])))
    d_seq, d_tot = _rel(seqs, want['seq_terms']), _rel(totals, _want_totals(want))
    print('%s: %d of %d gradient words differ; seq_terms rel %.2e (H W 2^-53 = %.2e); totals rel %.2e' % (
        what, wrong, grad.size, d_seq, H * W * 2.0 ** -53, d_tot))
    assert wrong == 0
    assert d_seq <= H * W * 2.0 ** -53 and d_tot <= 1e-12
    if exact:
        assert np.array_equal(_bits(seqs), _bits(want['seq_terms']))
        assert np.array_equal(_bits(totals), _bits(_want_totals(want)))


@pytest.mark.parametrize('kind', [0, 1, 2], ids=ref.KIND_NAMES)
@pytest.mark.parametrize('shape', CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_and_module_match_the_restatement(shape, kind):
    assert int(np.prod(shape)) // shape[1] * (shape[1] + 1) <= 1 << 18
    for inputs in ref.KINDS:
        pred, gt, want = _case(inputs, shape, kind)
        seqs, totals, (grad,) = _launch([pred], gt, kind)
        _compare(seqs[0], totals[0], grad, want, inputs == 'grid', '%s %s kind %d' % (inputs, shape, kind))
        # the module: the same launch behind autograd
        _module_matches(torch.from_numpy(np.array(pred)).to(DEV), torch.from_numpy(np.array(gt)).to(DEV), kind, seqs, totals, grad, want)


def _module_matches(p, g, kind, seqs, totals, grad, want):
    """losses.TemporalLoss on the device tensors ``p``, ``g`` (in whatever layout they lie) against one launch's outputs and the
    restatement: the fp32 scalar, the gradient map, seq_terms and last_terms, bit for bit."""
    p = p.requires_grad_()
    module = TemporalLoss(ref.KIND_NAMES[kind], EPS)
    loss = module(p, g)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    loss.backward()
    got = float(loss.detach())
    assert got == float(np.float32(totals[0][-1])) or (np.isnan(got) and np.isnan(totals[0][-1]))
    assert abs(got - want['loss']) <= 2.0 ** -23 * abs(want['loss'])                  # one rounding of a value within 1e-12 of it
    assert np.array_equal(_bits(p.grad.cpu().contiguous().numpy()), _bits(grad)) and np.array_equal(_bits(grad), _bits(want['grad']))
    assert np.array_equal(_bits(module.seq_terms.cpu().numpy()), _bits(seqs))
    assert np.array_equal(_bits(module.last_terms.cpu().numpy()), _bits(totals[:, :-1].astype(np.float32)))
    assert not module.last_terms.requires_grad and not module.seq_terms.requires_grad


@pytest.mark.parametrize('kind', [0, 1, 2], ids=ref.KIND_NAMES)
def test_a_base_one_element_off_alignment(kind, monkeypatch):
    """W % 4 == 0, but no run of the tensor starts at a multiple of 16 bytes: single words for that tensor alone.  Kernel and module, every
    input kind; the module gets the slice itself (a spy sees its pointer: no copy was made to realign it)."""
    shape = (2, 3, 3, 16, 64)
    L = _native.lib()
    seen = []
    real = L.tai_temporal_loss
    monkeypatch.setattr(L, 'tai_temporal_loss', lambda preds, n, gt_, *rest: seen.append((preds[0], gt_)) or real(preds, n, gt_, *rest))
    for inputs in ref.KINDS:
        pred, gt, want = _case(inputs, shape, kind)
        aligned = _launch([pred], gt, kind)
        for layouts, gt_layout in ((['off'], 'bt'), (['bt'], 'off'), (['off'], 'off')):
            seqs, totals, (grad,) = _launch([pred], gt, kind, layouts=layouts, gt_layout=gt_layout)
            _compare(seqs[0], totals[0], grad, want, inputs == 'grid', '%s pred %s gt %s' % (inputs, layouts[0], gt_layout))
            assert np.array_equal(_bits(seqs), _bits(aligned[0])) and np.array_equal(_bits(totals), _bits(aligned[1]))
        for p_layout, g_layout in (('off', 'bt'), ('off', 'off')):
            p, g = _store(pred, p_layout)[0], _store(gt, g_layout)[0]
            assert p.data_ptr() % 16 == 4
            _module_matches(p, g, kind, aligned[0], aligned[1], aligned[2][0], want)
            assert seen[-1] == (p.data_ptr(), g.data_ptr())


def test_one_chunk_past_the_grid_cap_makes_a_second_pass():
    shape = (GRID_CAP + 1, 1, 1, 2, 2)                            # one chunk per sequence: the first workgroup takes a second chunk
    pred, gt, want = _case('uniform', shape, 2)
    seqs, totals, (grad,) = _launch([pred], gt, 2)
    _compare(seqs[0], totals[0], grad, want, False, 'uniform %s' % (shape,))
    assert np.array_equal(_bits(seqs[0][[0, -1]]), _bits(want['seq_terms'][[0, -1]]))          # four terms each: any order is exact


def test_either_storage_gives_the_same_bits_and_the_view_is_read_where_it_lies(monkeypatch):
    shape = (3, 5, 1, 17, 66)
    for kind in (0, 1, 2):
        pred, gt, want = _case('smooth', shape, kind)
        bt = _launch([pred], gt, kind)
        for layouts, gt_layout in ((['tb'], 'bt'), (['bt'], 'tb'), (['tb'], 'tb')):
            seqs, totals, (grad,) = _launch([pred], gt, kind, layouts=layouts, gt_layout=gt_layout)
            _compare(seqs[0], totals[0], grad, want, False, 'pred %s gt %s kind %d' % (layouts[0], gt_layout, kind))
            assert np.array_equal(_bits(seqs), _bits(bt[0])) and np.array_equal(_bits(totals), _bits(bt[1]))
    # the module: tai.py's ``pred`` is a transposed view of a [T * B, ...] buffer; its data_ptr and strides are what the launch gets
    B, T, C, H, W = shape
    chw = C * H * W
    pred, gt, want = _case('smooth', shape, 2)
    stored = torch.from_numpy(np.array(pred)).to(DEV).transpose(0, 1).contiguous().view(T * B, C, H, W)
    view = stored.view(T, B, C, H, W).transpose(0, 1).requires_grad_()
    copy = view.detach().contiguous().requires_grad_()
    g = torch.from_numpy(np.array(gt)).to(DEV)
    assert not view.is_contiguous() and view.data_ptr() == stored.data_ptr()
    L = _native.lib()
    seen = []
    real = L.tai_temporal_loss

    def spy(preds, n, gt_, strides, kind, eps, seqs, totals, grads, *rest):
        seen.append(([preds[i] for i in range(n)], gt_, [strides[i] for i in range(2 * n + 2)], [grads[i] for i in range(n)]))
        return real(preds, n, gt_, strides, kind, eps, seqs, totals, grads, *rest)
    monkeypatch.setattr(L, 'tai_temporal_loss', spy)
    lv = TemporalLoss('charbonnier', EPS)(view, g)
    lc = TemporalLoss('charbonnier', EPS)(copy, g)
    assert seen[0][0] == [stored.data_ptr()] and seen[0][1] == g.data_ptr() and seen[0][2] == [chw, B * chw, T * chw, chw]
    assert seen[1][0] == [copy.data_ptr()] and seen[1][2] == [T * chw, chw, T * chw, chw]
    (3.0 * lv).backward()
    (3.0 * lc).backward()
    assert float(lv.detach()) == float(lc.detach()) == float(np.float32(want['loss']))
    assert view.grad.shape == view.shape and view.grad.stride() == view.stride()              # the map in the view's own layout
    assert torch.equal(view.grad.view(torch.int32), copy.grad.view(torch.int32))
    assert np.array_equal(_bits(copy.grad.cpu().numpy()), _bits(np.float32(3.0) * want['grad']))          # one fp32 product
    # a tensor whose blocks are not dense is made contiguous first; no_grad and a detached prediction get no map
    wide = torch.zeros(B, T, C, H, W + 2, device=DEV)
    wide[..., :W] = view.detach()
    seen.clear()
    with torch.no_grad():
        quiet = TemporalLoss('charbonnier', EPS)((wide[..., :W], view), g)
    assert seen[0][0][0] != wide.data_ptr() and seen[0][0][1] == stored.data_ptr() and seen[0][3] == [None, None]
    assert seen[0][2] == [T * chw, chw, chw, B * chw, T * chw, chw]
    assert float(quiet[0]) == float(quiet[1]) == float(lv.detach()) and not quiet[0].requires_grad
    TemporalLoss('charbonnier', EPS)((view, copy.detach()), g)
    assert seen[1][3][0] is not None and seen[1][3][1] is None


def test_a_launch_of_three_gives_each_prediction_the_bits_of_its_own_launch():
    shape = (2, 3, 2, 9, 13)
    for kind in (0, 1, 2):
        cases = [_case(inputs, shape, kind, seed) for seed, inputs in enumerate(('uniform', 'smooth', 'wide'))]
        gt = cases[0][1]
        preds = [c[0] for c in cases]
        alone = [_launch([p], gt, kind) for p in preds]
        for i, p in enumerate(preds):                                   # (each against the restatement with the shared gt)
            _compare(alone[i][0][0], alone[i][1][0], alone[i][2][0], ref.temporal_loss_ref(p, gt, kind, EPS), False, 'alone %d' % i)
        together = _launch(preds, gt, kind, layouts=['tb', 'bt', 'bt'])
        again = _launch(preds, gt, kind, layouts=['tb', 'bt', 'bt'])
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


def test_a_sequence_does_not_depend_on_its_batch():
    shape5 = (5, 3, 2, 9, 13)
    for kind in (0, 2):
        pred5, gt5, want5 = _case('smooth', shape5, kind)
        seqs5, _, (grad5,) = _launch([pred5], gt5, kind)
        assert np.array_equal(_bits(grad5), _bits(want5['grad']))
        for b in (0, 3):
            pred1, gt1 = pred5[b:b + 1], gt5[b:b + 1]
            want1 = ref.temporal_loss_ref(pred1, gt1, kind, EPS)
            seqs1, _, (grad1,) = _launch([pred1], gt1, kind)
            assert np.array_equal(_bits(grad1), _bits(want1['grad']))                 # each B through the restatement, bit for bit
            assert np.array_equal(_bits(seqs1[0]), _bits(seqs5[0, 2 * b:2 * b + 2]))  # the sums know nothing of (S, T, H, W) but their own pixels


def test_a_nan_stays_in_its_sequence():
    shape = (3, 4, 2, 9, 13)
    for kind in (0, 1, 2):
        pred, gt, _ = _case('uniform', shape, kind)
        clean_seqs, _, (clean_grad, _) = _launch([pred, pred], gt, kind, grads=[True, False])
        dirty = np.array(pred)
        dirty[1, 2, 1, 4, 7] = np.nan                                                 # sequence b = 1, c = 1: number 3; frame 2
        seqs, totals, (grad, _) = _launch([dirty, pred], gt, kind, grads=[True, False])
        keep = np.ones(6, bool)
        keep[3] = False
        assert np.array_equal(_bits(seqs[0][keep]), _bits(clean_seqs[0][keep]))
        assert np.isnan(seqs[0][3][2:4]).all() and np.array_equal(_bits(seqs[0][3][[0, 1, 4]]), _bits(clean_seqs[0][3][[0, 1, 4]]))
        assert np.isnan(totals[0][[2, 3, 5]]).all() and np.isfinite(totals[0][[0, 1, 4]]).all()
        assert np.array_equal(_bits(seqs[1]), _bits(clean_seqs[1])) and np.isfinite(totals[1]).all()      # the other prediction
        bad = np.argwhere(np.isnan(grad))
        assert sorted(map(tuple, bad)) == [(1, 1, 1, 4, 7), (1, 2, 1, 4, 7), (1, 3, 1, 4, 7)]              # the pixel, and its two neighbours in time
        ok = ~np.isnan(grad)
        assert np.array_equal(_bits(grad[ok]), _bits(clean_grad[ok]))


def test_forward_and_backward_replay_inside_one_graph():
    shape = (2, 3, 1, 32, 32)
    first = [_case(inputs, shape, 2, 1 + i) for i, inputs in enumerate(('smooth', 'uniform', 'wide'))]
    second = [_case(inputs, shape, 2, 5 + i) for i, inputs in enumerate(('uniform', 'grid', 'smooth'))]
    sp = [_store(first[0][0], 'tb')[0].requires_grad_()] + [torch.from_numpy(np.array(c[0])).to(DEV).requires_grad_() for c in first[1:]]
    sg = torch.from_numpy(np.array(first[0][1])).to(DEV)
    gt2 = second[0][1]
    kit.check_graph_replay(lambda: TemporalLoss('charbonnier', EPS), sp, sg, [c[0] for c in second], gt2,
                           [ref.temporal_loss_ref(c[0], gt2, 2, EPS)['grad'] for c in second])


# ---------------------------------------------------------------------------------------------------------------- drivers

TAI_KEYS = ('G_temporal', 'G_temporal_forward', 'G_temporal_backward')


def _terms(out, n, keys=TAI_KEYS):
    """{key: [value per printed update]}; asserts each key is printed on every line, finite and positive."""
    return kit._terms(out, n, keys, 0.0, float('inf'))


def test_the_keys_come_with_the_weight_and_weight_zero_is_the_run_without_the_flag(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    L = _native.lib()
    seen = []
    real = L.tai_temporal_loss
    monkeypatch.setattr(L, 'tai_temporal_loss', lambda preds, n, *rest: seen.append(n) or real(preds, n, *rest))
    plain = _train(tmp_path, capsys, 'plain', 3, ['--resumable'])
    zero = _train(tmp_path, capsys, 'zero', 3, ['--resumable', '--temporal_weight', '0', '--temporal_kind', 'l1'])
    assert len(_states(plain)) == 3 and _states(plain) == _states(zero)
    assert 'G_temporal' not in plain and 'G_temporal' not in zero and seen == []
    out = _train(tmp_path, capsys, 'on', 3, ['--temporal_weight', '0.5'])
    print(_terms(out, 3))
    assert seen == [3, 3, 3]                                                          # bi-TAI: one launch per update for its three predictions
    a, b = _generator(tmp_path, 'plain'), _generator(tmp_path, 'on')
    assert list(a) == list(b) and any(not torch.equal(a[k], b[k]) for k in a)
    assert all(torch.isfinite(v).all() for v in b.values() if v.is_floating_point())


@pytest.mark.parametrize('extra', [[], ['--guard', '--clip_grad_norm', '1', '--fused_step', '--ema_decay', '0.99', '--ssim_weight', '0.2',
                                        '--image_loss', 'charbonnier', '--lap_weight', '0.5']], ids=['resumable', 'guard_fused_ema_all_terms'])
def test_straight_against_split_with_the_temporal_term(tmp_path, capsys, monkeypatch, extra):
    monkeypatch.chdir(tmp_path)
    kit.check_straight_against_split(tmp_path, capsys, ['--resumable', '--temporal_weight', '0.5'] + extra, _terms)


def test_graph_step_with_the_temporal_term(tmp_path, capsys, monkeypatch):
    """Updates 1-2 eager, 3 captured and replayed, 4 replayed: the launch is part of the captured update."""
    monkeypatch.chdir(tmp_path)
    kit.check_graph_step(tmp_path, capsys, ['--temporal_weight', '0.5', '--temporal_kind', 'l1'], _terms, replays_differ=True)


def test_mcnet_runs_with_one_prediction(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    L = _native.lib()
    seen = []
    real = L.tai_temporal_loss
    monkeypatch.setattr(L, 'tai_temporal_loss', lambda preds, n, *rest: seen.append(n) or real(preds, n, *rest))
    out = _train(tmp_path, capsys, 'm', 3, ['--temporal_weight', '0.5', '--temporal_kind', 'l2'], model=MCNET)
    print(_terms(out, 3, ('G_temporal',)))
    assert 'G_temporal_forward' not in out and seen == [1, 1, 1]
