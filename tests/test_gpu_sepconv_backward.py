"""The three gradients of the separable convolution (tai_sepconv_backward: gI, gV, gH) against the CPU oracle accumulated
in fp64, on ragged tiles and on every route of the launcher.

Integer-exact cases (tests/sepconv_cases.py: small integers with +-512 outliers on the tile seams; every partial sum an
integer below 2^24, asserted in tests/test_sepconv_cases_cpu.py) are compared with torch.equal: any fp32 summation order
gives exactly the oracle's value, the atomic routes included, so one missing, doubled or misplaced term fails.  Float cases
(test_gpu_sepconv.py's generator) are held to that module's BWD_TOL = 2e-5 of 1 + |ref| and guard the rounding.

Branch of tai_sepconv_backward -> test that holds it:
  gI strips, slabs in the borrowed gV      test_every_route_matches_the_oracle_exactly (variants 0 / 3 / 4), test_request_subsets
  gI strips, slabs in the borrowed gH      test_request_subsets {I, H}, test_nothing_is_written_outside_the_outputs {I, H}
  gI strips, atomics: nothing to borrow    test_request_subsets {I}, test_nothing_is_written_outside_the_outputs {I}
  gI strips, atomics: slabs do not fit     test_every_route... at 1x1x2x104, 1x3x5x124, 1x3x11x132
  sepconv_grad_i_rows                      test_every_route... (grad-input variant 2)
  gI gather, triples and singles           test_generic_routes_match_the_oracle_exactly (C = 4, 5, 2, 1), variant 1 everywhere
  sepconv_grad_vh_ab, four forms           test_every_route... (tap variants 0, 2, 3, 4 at C = 1)
  sepconv_grad_vh_ab, gV or gH null        test_request_subsets at 1x1x9x132 and 1x1x2x108 (tap variants 0, 2)
  tiled gV / gH, C = 1, either one null    test_request_subsets at 1x1x9x132 and 1x1x2x108 (tap variant 1); both: test_every_route...
  tiled gV / gH, C = 3, either one null    test_every_route... at C = 3, test_request_subsets at 1x3x9x132
  generic gV / gH                          test_generic_routes_match_the_oracle_exactly, test_request_subsets at 1x4x5x8
"""
import itertools

import numpy as np
import pytest
import torch

import video_frame_inpainting_amd as vfi
from video_frame_inpainting_amd import _native
from oracle import sepconv_oracle as so

import sepconv_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
BWD_TOL = 2e-5              # tests/test_gpu_sepconv.py's gradient tolerance, relative to 1 + |ref|
DEV = 'cuda:0'
SENTINEL = -1234.5          # finite and no integer: an output element the kernels never wrote cannot equal the oracle
GI_VARIANTS = TAP_VARIANTS = (0, 1, 2, 3, 4)


def _rel(a, b):
    return float(np.max(np.abs(a.astype(np.float64) - b) / (1 + np.abs(b))))


def _dev(ts):
    return tuple((torch.tensor(t) if isinstance(t, np.ndarray) else t).to(DEV) for t in ts)


_ORACLE = {}


def _oracle(kind, shape, seed):
    """(case on the host, (rI, rV, rH) of the fp64 oracle as numpy): computed once per case, shared, never written to."""
    key = (kind, shape, seed)
    if key not in _ORACLE:
        case = (sc.int_case if kind == 'int' else sc.float_case)(*shape, seed)
        inp, v, h, gO = case
        ref = so.backward(gO.numpy(), inp.numpy(), v.numpy(), h.numpy(), shape[4], f64=True)
        for r in ref:
            r.setflags(write=False)
        _ORACLE[key] = (case, ref)
    return _ORACLE[key]


def _backward(gO, inp, v, h, ks, need=(True, True, True)):
    """tai_sepconv_backward through the C ABI on device tensors -> [gI, gV, gH] (None where not requested).  The outputs are
    filled with SENTINEL first: torch.empty would hand back the block that held the previous call's (correct) gradient."""
    B, C = inp.shape[:2]
    H, W = v.shape[2:]
    outs = [torch.full_like(t, SENTINEL) if n else None for t, n in zip((inp, v, h), need)]
    ptr = lambda t: t.data_ptr() if t is not None else None
    _native.check(_native.lib().tai_sepconv_backward(gO.data_ptr(), inp.data_ptr(), v.data_ptr(), h.data_ptr(), ptr(outs[0]),
                                                     ptr(outs[1]), ptr(outs[2]), B, C, H, W, ks,
                                                     torch.cuda.current_stream().cuda_stream), 'tai_sepconv_backward')
    return outs


class _Variants(object):
    """Select (grad-input variant, tap-gradient variant) for the block; both selectors are restored on the way out."""

    def __init__(self, gi, taps):
        self.want = (gi, taps)

    def __enter__(self):
        L = _native.lib()
        self.prev_gi = L.tai_sepconv_set_grad_input_variant(self.want[0])
        self.prev_taps = L.tai_sepconv_set_grad_taps_variant(self.want[1])

    def __exit__(self, *exc):
        L = _native.lib()
        L.tai_sepconv_set_grad_input_variant(self.prev_gi)
        L.tai_sepconv_set_grad_taps_variant(self.prev_taps)


def _assert_equal(got, want, what):
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        first = tuple(int(i) for i in bad[0])
        raise AssertionError('%s: %d of %d elements differ, first at %r: got %r, want %r'
                             % (what, bad.shape[0], want.numel(), first, float(got[first]), float(want[first])))


# ---- every route at every ragged shape, integer-exact -------------------------------------------------------------------

@pytest.mark.parametrize('shape', sc.TILEABLE_SHAPES, ids=sc.shape_id)
def test_every_route_matches_the_oracle_exactly(shape):
    """Grad-input variants 0-4 x tap-gradient variants 0-4: strips with the assembly and the C++ row loop (slabs in the
    borrowed gV where they fit, atomics where they do not), the gather, the row-scatter with atomics; the fused
    sepconv_grad_vh_ab in its four forms and the two tiled kernels.  Integer-exact data: torch.equal for every pair."""
    ks = shape[4]
    case, ref = _oracle('int', shape, 21)
    inp, v, h, gO = _dev(case)
    want = _dev(ref)
    for gi, taps in itertools.product(GI_VARIANTS, TAP_VARIANTS):
        with _Variants(gi, taps):
            got = _backward(gO, inp, v, h, ks)
        for name, g, w in zip(('gI', 'gV', 'gH'), got, want):
            _assert_equal(g, w, '%s, grad-input variant %d, tap variant %d' % (name, gi, taps))


@pytest.mark.parametrize('shape', sc.GENERIC_SHAPES, ids=sc.shape_id)
def test_generic_routes_match_the_oracle_exactly(shape):
    """C not in {1, 3}, W % 4 != 0, ks != 51: the gather in channel triples and singles, the generic gV / gH."""
    ks = shape[4]
    case, ref = _oracle('int', shape, 22)
    inp, v, h, gO = _dev(case)
    got = _backward(gO, inp, v, h, ks)
    for name, g, r in zip(('gI', 'gV', 'gH'), got, ref):
        _assert_equal(g, _dev([r])[0], name)


# ---- the same shapes on float data --------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', sc.ALL_SHAPES, ids=sc.shape_id)
def test_default_route_matches_the_oracle_on_float_data(shape):
    ks = shape[4]
    case, ref = _oracle('float', shape, 23)
    inp, v, h, gO = _dev(case)
    got = _backward(gO, inp, v, h, ks)
    errs = {name: _rel(g.cpu().numpy(), r) for name, g, r in zip(('gI', 'gV', 'gH'), got, ref)}
    print(sc.shape_id(shape), errs)
    assert max(errs.values()) < BWD_TOL, errs


@pytest.mark.parametrize('shape', [(1, 1, 9, 132, 51), (1, 3, 9, 132, 51)], ids=sc.shape_id)
def test_every_route_matches_the_oracle_on_float_data(shape):
    ks = shape[4]
    case, ref = _oracle('float', shape, 23)
    inp, v, h, gO = _dev(case)
    worst = {}
    for gi, taps in itertools.product(GI_VARIANTS, TAP_VARIANTS):
        with _Variants(gi, taps):
            got = _backward(gO, inp, v, h, ks)
        for name, g, r in zip(('gI', 'gV', 'gH'), got, ref):
            worst[(name, gi, taps)] = _rel(g.cpu().numpy(), r)
    bad = {k: e for k, e in worst.items() if not e < BWD_TOL}
    print(sc.shape_id(shape), 'largest error', max(worst.values()))
    assert not bad, bad


# ---- request subsets ----------------------------------------------------------------------------------------------------

def _autograd_subset(case_dev, ks, need):
    """The gradients torch.autograd.grad asks the op for -> [gI, gV, gH] (None where not requested)."""
    inp, v, h, gO = case_dev
    leaves = [t.detach().clone().requires_grad_(n) for t, n in zip((inp, v, h), need)]
    out = vfi.SeparableConvolution.apply(leaves[0], leaves[1], leaves[2], ks)
    grads = iter(torch.autograd.grad(out, [t for t, n in zip(leaves, need) if n], gO))
    return [next(grads) if n else None for n in need]


def _spoil(grads):
    """The op allocates its outputs with torch.empty, and the allocator hands the next call the block that held this call's
    (correct) gradient: overwrite it, so that an element the next call does not write cannot pass."""
    for g in grads:
        if g is not None:
            g.fill_(SENTINEL)


@pytest.mark.parametrize('shape', sc.SUBSET_SHAPES, ids=sc.shape_id)
def test_request_subsets(shape):
    """All seven non-empty subsets of (gI, gV, gH), with the fused tap-gradient kernel (tap variants 0 and 2, with and without
    the early tap loads: at C = 1 the waves of a gradient that was not requested leave before their row loop) and with the two
    separate kernels (variant 1: either output null).
    Integer-exact data: whatever is returned equals the oracle.  Float data: gV and gH carry the bits of the all-three call
    whatever else was asked for; gI does too where a tap buffer was there to borrow and the slabs fit (the fixed-order slab
    sum), and is within BWD_TOL otherwise.  The operands are never written."""
    B, C, H, W, ks = shape
    names = ('gI', 'gV', 'gH')
    slab_route = sc.tileable(C, W, ks) and sc.slabs_fit(B, C, H, W, ks)
    icase, iref = _oracle('int', shape, 24)
    fcase, fref = _oracle('float', shape, 25)
    idev, fdev, want = _dev(icase), _dev(fcase), _dev(iref)
    for taps in (0, 1, 2):
        with _Variants(0, taps):
            for need in sc.SUBSETS:
                got = _autograd_subset(idev, ks, need)
                for name, g, w, n in zip(names, got, want, need):
                    assert (g is not None) == n
                    if n:
                        _assert_equal(g, w, '%s of subset %r, tap variant %d' % (name, need, taps))
                _spoil(got)
            full = _autograd_subset(fdev, ks, (True, True, True))
            for need in sc.SUBSETS[1:]:
                got = _autograd_subset(fdev, ks, need)
                for k in (1, 2):
                    if need[k]:
                        _assert_equal(got[k], full[k], '%s of subset %r against the all-three call, tap variant %d' % (names[k], need, taps))
                if need[0] and slab_route and (need[1] or need[2]):
                    _assert_equal(got[0], full[0], 'gI of subset %r against the all-three call' % (need,))
                elif need[0]:
                    assert _rel(got[0].cpu().numpy(), fref[0]) < BWD_TOL, need
                _spoil(got)
    # input, vertical, horizontal, grad_output: bit-unchanged after all of these calls
    for dev, case in ((idev, icase), (fdev, fcase)):
        for t, t0 in zip(dev, case):
            assert torch.equal(t.cpu(), t0)


# ---- nothing outside the outputs ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('need', [(True, True, True), (True, False, True), (True, False, False)], ids=['IVH', 'IH', 'I'])
@pytest.mark.parametrize('shape', sc.BAND_SHAPES, ids=sc.shape_id)
def test_nothing_is_written_outside_the_outputs(shape, need):
    """Each output is a 16-byte-aligned view in the middle of a larger allocation filled with a sentinel, with a band of at
    least one tile slab (and of everything the strips kernel would write, fit or not) on either side: the bands are
    untouched, the outputs equal the oracle.  The slabs go to gV ({I,V,H}), to gH ({I,H}) or nowhere ({I}: atomics)."""
    B, C, H, W, ks = shape
    case, ref = _oracle('int', shape, 26)
    inp, v, h, gO = _dev(case)
    band = max(sc.GI_SLAB, sc.slab_floats(B, C, H, W))
    assert band % 4 == 0 and band >= 10800
    fill = 7.5
    bufs, views = [], []
    for t, n in zip((inp, v, h), need):
        buf = torch.full((band + t.numel() + band,), fill, device=DEV) if n else None
        view = buf[band:band + t.numel()].view(t.shape) if n else None
        assert view is None or (view.data_ptr() % 16 == 0 and view.is_contiguous())
        bufs.append(buf); views.append(view)
    ptr = lambda t: t.data_ptr() if t is not None else None
    _native.check(_native.lib().tai_sepconv_backward(gO.data_ptr(), inp.data_ptr(), v.data_ptr(), h.data_ptr(), ptr(views[0]),
                                                     ptr(views[1]), ptr(views[2]), B, C, H, W, ks,
                                                     torch.cuda.current_stream().cuda_stream), 'tai_sepconv_backward')
    torch.cuda.synchronize()
    for name, buf, view, r in zip(('gI', 'gV', 'gH'), bufs, views, ref):
        if buf is None:
            continue
        assert bool((buf[:band] == fill).all()), 'band in front of %s was written' % name
        assert bool((buf[band + view.numel():] == fill).all()), 'band behind %s was written' % name
        _assert_equal(view, _dev([r])[0], name)


# ---- reproducible bits, stale LDS ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', sc.REPEAT_SHAPES, ids=sc.shape_id)
def test_all_three_gradients_are_bit_reproducible(shape):
    ks = shape[4]
    assert sc.slabs_fit(*shape)                       # gI on the slab route: a fixed-order sum
    case, _ = _oracle('float', shape, 27)
    inp, v, h, gO = _dev(case)
    first = _backward(gO, inp, v, h, ks)
    for _ in range(3):
        again = _backward(gO, inp, v, h, ks)
        for name, a, b in zip(('gI', 'gV', 'gH'), first, again):
            _assert_equal(b, a, name + ' of a repeated call')


@pytest.mark.parametrize('shape', sc.REPEAT_SHAPES, ids=sc.shape_id)
def test_no_state_survives_in_lds_between_launches(shape):
    """LDS keeps its contents from launch to launch: the `ready` counter, the tap ring, the three-buffer DMA ring reused
    across channels, the accumulator strips.  Alternate gO with its exact negation: on the deterministic routes all three
    gradients alternate between g and exactly -g; anything read before it was written this launch is the previous launch's
    value and shows.  The same with the frame and its negation for gV and gH (gI does not read the frame)."""
    ks = shape[4]
    assert sc.slabs_fit(*shape)
    case, ref = _oracle('float', shape, 28)
    inp, v, h, gO = _dev(case)
    ngO, ninp = -gO, -inp
    pos = _backward(gO, inp, v, h, ks)
    for name, g, r in zip(('gI', 'gV', 'gH'), pos, ref):
        assert _rel(g.cpu().numpy(), r) < BWD_TOL, name
    for _ in range(5):
        for name, g, p in zip(('gI', 'gV', 'gH'), _backward(ngO, inp, v, h, ks), pos):
            _assert_equal(g, -p, name + ' of -gO')
        for name, g, p in zip(('gI', 'gV', 'gH'), _backward(gO, inp, v, h, ks), pos):
            _assert_equal(g, p, name + ' of gO')
    for _ in range(5):
        for name, g, p in zip(('gV', 'gH'), _backward(gO, ninp, v, h, ks, (False, True, True))[1:], pos[1:]):
            _assert_equal(g, -p, name + ' of -input')
        for name, g, p in zip(('gV', 'gH'), _backward(gO, inp, v, h, ks, (False, True, True))[1:], pos[1:]):
            _assert_equal(g, p, name + ' of input')
