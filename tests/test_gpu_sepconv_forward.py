"""The forward of the separable convolution (tai_sepconv_forward) against the CPU oracle accumulated in fp64, on ragged tiles,
at C > 1 and on every route of the launcher.

Integer-exact cases (tests/sepconv_cases.py, fwd_int_case: small integers with +-512 outliers on the forward's seams -- the
row and column tile seams, the last patch row and column, the two padded columns the LDS-DMA staging writes separately; the
sum of the absolute terms of every output below 2^24, asserted in tests/test_sepconv_cases_cpu.py) are compared with
torch.equal: any fp32 summation order, rows first or accumulators folded last, gives exactly the oracle's value, so one
missing, doubled or misplaced term fails.  Float cases (sepconv_cases.float_case) are held to test_gpu_sepconv.py's
FWD_TOL = 1e-5 of 1 + |ref| and guard the rounding.

The persistent kernel's cases take their batch size from the CU count of the device that runs them (sepconv_cases.
persistent_batch), and every claim "this shape runs that kernel" is asserted through tai_sepconv_forward_route, the launcher's
own decision: a case that fell back to another kernel fails instead of testing that kernel twice.

Branch of tai_sepconv_forward -> test that holds it:
  case 1, generic kernel                        test_every_variant_matches_the_oracle_exactly at 1x1x6x10, 1x2x5x9-ks7, 1x1x4x6-ks1
                                                (variants 0 and 1), variant 1 at every other shape
  refusal: tiled variant, shape not tileable    test_every_variant... at the same three shapes (variants 2-27: EINVAL, nothing written)
  cases 2-4 (tiled, split, packed)              test_every_variant... (triples and singles at C = 2, 4, 5, 6, 7; 8-row tiles at H % 8 = 1)
  cases 5-9 (sepconv_forward_asm)               test_every_variant... (8-row tiles for 5 / 6, 16-row for 7-9)
  cases 10-13, 16, 18 (sepconv_forward_ab)      test_every_variant..., test_persistent_kernel_on_ragged_planes (16, 18 as controls)
  cases 14, 15 (sepconv_forward_asm_channels)   test_every_variant... (the in-kernel channel loop at C = 2-7)
  cases 17, 19: channel triples                 test_every_variant... at C = 3, 6 (c0 = 3), test_channel_offsets
  cases 17, 19: leftover channels on kernel 16  test_every_variant... and test_channel_offsets at C = 4, 5, 7
  17 / 19 -> 16: C < 3, no triple               test_every_variant... and test_channel_offsets at 2x2x9x132, every C = 1 shape
  cases 21-27, persistent kernel                test_persistent_kernel_on_ragged_planes (three tiles per workgroup: both patch buffers
                                                reused), test_persistent_fallbacks 'few' (by number: one tile per workgroup)
  20 / automatic -> 21 or 26 by footprint       test_persistent_kernel_on_ragged_planes (variants 0 and 20)
  persistent fallback: tile count % 8 != 0      test_persistent_fallbacks 'ragged' (variants 0, 20-27 -> 18)
  persistent fallback: tiles <= workgroups      test_persistent_fallbacks 'few' (variant 0 -> 18)
  persistent fallback: C != 1                   test_every_variant... at C >= 2 (variants 20-27 -> 18)
  default: unknown variant                      test_route_query_refuses_what_the_launcher_refuses
"""
import numpy as np
import pytest
import torch

import video_frame_inpainting_amd as vfi
from video_frame_inpainting_amd import _native
from video_frame_inpainting_amd import separable_convolution as sepconv
from oracle import sepconv_oracle as so

import sepconv_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
FWD_TOL = 1e-5              # tests/test_gpu_sepconv.py's forward tolerance, relative to 1 + |ref|
DEV = 'cuda:0'
SENTINEL = -1234.5          # finite and no integer: an output element the kernels never wrote cannot equal the oracle
EINVAL = -1                 # TAI_SEPCONV_EINVAL
PLANE_IDS = ['%dx%d' % p for p in sc.FWD_PERSISTENT_PLANES]
NARROW = sc.FWD_PERSISTENT_PLANES[0]        # (20, 132): a 4-column last column tile, a 4-row last row tile


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rel(a, b):
    return float(np.max(np.abs(a.astype(np.float64) - b) / (1 + np.abs(b))))


def _dev(ts):
    return tuple((torch.tensor(t) if isinstance(t, np.ndarray) else t).to(DEV) for t in ts)


_ORACLE = {}


def _oracle(kind, shape, seed, keep=True):
    """(case on the host: input, v, h; the fp64 oracle's output as numpy): computed once per case, shared, never written to."""
    key = (kind, shape, seed)
    if key in _ORACLE:
        return _ORACLE[key]
    case = sc.fwd_int_case(*shape, seed) if kind == 'int' else sc.float_case(*shape, seed)[:3]
    ref = so.forward(case[0].numpy(), case[1].numpy(), case[2].numpy(), shape[4], f64=True)
    ref.setflags(write=False)
    if keep:
        _ORACLE[key] = (case, ref)
    return case, ref


def _launch(inp, v, h, out, ks):
    """tai_sepconv_forward through the C ABI on device tensors, into `out` -> return code."""
    B, C = inp.shape[:2]
    H, W = v.shape[2:]
    return _native.lib().tai_sepconv_forward(inp.data_ptr(), v.data_ptr(), h.data_ptr(), out.data_ptr(), B, C, H, W, ks,
                                             torch.cuda.current_stream().cuda_stream)


def _forward(inp, v, h, ks):
    """The output is filled with SENTINEL first: torch.empty would hand back the block that held the previous call's
    (correct) result."""
    B, C = inp.shape[:2]
    H, W = v.shape[2:]
    out = torch.full((B, C, H, W), SENTINEL, device=DEV)
    _native.check(_launch(inp, v, h, out, ks), 'tai_sepconv_forward')
    return out


class _Variant(object):
    """Select the forward variant for the block; the selector is restored on the way out."""

    def __init__(self, variant):
        self.want = variant

    def __enter__(self):
        self.prev = _native.lib().tai_sepconv_set_forward_variant(self.want)

    def __exit__(self, *exc):
        _native.lib().tai_sepconv_set_forward_variant(self.prev)


def _route(shape, variant):
    return _native.lib().tai_sepconv_forward_route(*shape, variant)


def _expected_route(shape, variant, cus):
    """include/tai_sepconv.h's description of tai_sepconv_forward_route, from sepconv_cases' predicates."""
    B, C, H, W, ks = shape
    if not sc.fwd_tileable(W, ks):
        return 1 if variant in (0, 1) else EINVAL
    forced = variant != 0
    if variant == 0:
        variant = 20 if C == 1 else 19
    if 20 <= variant <= 27:
        if C != 1 or not sc.fwd_persistent_runs(B, H, W, cus, forced):
            return 18
        if variant == 20:
            return 26 if 2 * B * 51 * H * W * 4 > (256 << 20) else 21
        return variant
    if variant in (17, 19):
        return variant if C >= 3 else 16
    return variant


def _assert_equal(got, want, what):
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        first = tuple(int(i) for i in bad[0])
        raise AssertionError('%s: %d of %d elements differ, first at %r: got %r, want %r'
                             % (what, bad.shape[0], want.numel(), first, float(got[first]), float(want[first])))


# ---- every variant at every small and colour shape, integer-exact ----------------------------------------------------------

@pytest.mark.parametrize('shape', sc.FWD_FIXED_SHAPES, ids=sc.shape_id)
def test_every_variant_matches_the_oracle_exactly(shape):
    """Variants 0-27 on integer-exact data: each equals the fp64 oracle, so all are equal to each other.  The 8-row kernels
    (2-6, 15) and the 16-row ones meet H % 8 = 1 and H % 16 = 1, a second and third column tile, a 4-column last tile, and
    C = 2-7 with its channel triples and leftovers.  Where the shape is not tileable, every variant but 0 and 1 is refused
    and writes nothing."""
    ks = shape[4]
    case, ref = _oracle('int', shape, 31)
    inp, v, h = _dev(case)
    want, = _dev([ref])
    cus = _cus()
    for variant in sc.FWD_VARIANTS:
        route = _route(shape, variant)
        assert route == _expected_route(shape, variant, cus), (variant, route)
        with _Variant(variant):
            if route < 0:
                out = torch.full(ref.shape, SENTINEL, device=DEV)
                assert _launch(inp, v, h, out, ks) == EINVAL and b'ks == 51' in _native.lib().tai_sepconv_last_error()
                torch.cuda.synchronize()
                assert bool((out == SENTINEL).all()), 'refused variant %d wrote to the output' % variant
            else:
                _assert_equal(_forward(inp, v, h, ks), want, 'variant %d (kernel %d)' % (variant, route))
    for t, t0 in zip((inp, v, h), case):
        assert torch.equal(t.cpu(), t0)                   # the operands are never written


def test_route_query_refuses_what_the_launcher_refuses():
    L = _native.lib()
    t = torch.full((16,), SENTINEL, device=DEV)
    p = t.data_ptr()
    for variant in (28, 29, 99, 100, 117, 120, 127, -1):
        assert L.tai_sepconv_forward_route(1, 1, 16, 128, 51, variant) == EINVAL and b'unknown forward variant' in L.tai_sepconv_last_error()
        with _Variant(variant):
            assert L.tai_sepconv_forward(p, p, p, p, 1, 1, 16, 128, 51, None) == EINVAL
            assert b'unknown forward variant' in L.tai_sepconv_last_error()
    for dims in ((0, 1, 8, 8, 51), (1, 0, 8, 8, 51), (1, 1, 0, 8, 51), (1, 1, 8, 0, 51), (1, 1, 8, 8, 0), (4096, 1, 1024, 1024, 51)):
        assert L.tai_sepconv_forward_route(*dims, 0) == EINVAL and b'dimension' in L.tai_sepconv_last_error()
        assert L.tai_sepconv_forward(p, p, p, p, *dims, None) == EINVAL
    assert L.tai_sepconv_forward_route(1, 1, 8, 10, 51, 18) == EINVAL and L.tai_sepconv_forward_route(1, 1, 8, 10, 51, 0) == 1
    assert L.tai_sepconv_forward_route(1, 1, 8, 8, 7, 20) == EINVAL and L.tai_sepconv_forward_route(1, 3, 8, 8, 7, 1) == 1
    torch.cuda.synchronize()
    assert bool((t == SENTINEL).all())


# ---- the persistent kernel ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('plane', sc.FWD_PERSISTENT_PLANES, ids=PLANE_IDS)
def test_persistent_kernel_on_ragged_planes(plane):
    """sepconv_forward_persistent with a narrow last column tile (4, 64, 80 columns: stage_patch_dma's qmax masking and its two
    edge floats inside the double-buffered loop) and a ragged last row tile, three tiles for some workgroup, so that both
    patch buffers are staged a second time while the previous tile is still computing.  ALL images against the oracle, for
    the automatic route, every persistent policy and the one-tile kernels 16 / 18; then launches on the frames and on their
    exact negation alternate: a patch or tap element left from the previous launch would show."""
    cus = _cus()
    shape = sc.fwd_persistent_shape(plane, cus)
    B, C, H, W, ks = shape
    assert sc.fwd_rounds(B, H, W, cus)[0] == sc.PERSISTENT_ROUNDS == 3
    for variant in (0,) + sc.FWD_PERSISTENT_VARIANTS:
        route = _route(shape, variant)
        assert 21 <= route <= 27 and route == _expected_route(shape, variant, cus), (variant, route)
    assert _route(shape, 16) == 16 and _route(shape, 18) == 18
    case, ref = _oracle('int', shape, 32)
    inp, v, h = _dev(case)
    want, = _dev([ref])
    neg = -inp
    for variant in (0, 16, 18) + sc.FWD_PERSISTENT_VARIANTS:
        with _Variant(variant):
            _assert_equal(_forward(inp, v, h, ks), want, 'variant %d' % variant)
            for _ in range(3):
                _assert_equal(_forward(neg, v, h, ks), -want, 'variant %d on the negated frames' % variant)
                _assert_equal(_forward(inp, v, h, ks), want, 'variant %d back on the frames' % variant)


@pytest.mark.parametrize('kind', ['ragged', 'few'])
@pytest.mark.parametrize('plane', sc.FWD_PERSISTENT_PLANES, ids=PLANE_IDS)
def test_persistent_fallbacks(plane, kind):
    """The same planes with the batch size that breaks one condition of the persistent route: a tile count that is no
    multiple of 8 (kernel 18, whatever was asked for), and a multiple of 8 with at most one tile per workgroup (kernel 18 on
    the automatic route; the persistent kernel, one tile per workgroup and `has_next` never true, when asked for by number)."""
    cus = _cus()
    shape = sc.fwd_fallback_shapes(plane, cus)[kind]
    B, C, H, W, ks = shape
    routes = {variant: _route(shape, variant) for variant in (0,) + sc.FWD_PERSISTENT_VARIANTS}
    assert routes == {variant: _expected_route(shape, variant, cus) for variant in routes}
    if kind == 'ragged':
        assert sc.fwd_tiles(B, H, W) % 8 != 0 and set(routes.values()) == {18}, routes
    elif sc.fwd_tiles(B, H, W) <= cus // 8 * 8:
        assert routes[0] == 18 and routes[20] in (21, 26) and all(routes[k] == k for k in range(21, 28)), routes
        assert sc.fwd_rounds(B, H, W, cus) == (1, 1)
    case, ref = _oracle('int', shape, 33, keep=False)
    inp, v, h = _dev(case)
    want, = _dev([ref])
    for variant in routes:
        with _Variant(variant):
            _assert_equal(_forward(inp, v, h, ks), want, 'variant %d (kernel %d)' % (variant, routes[variant]))


# ---- channels ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [s for s in sc.FWD_C3_SHAPES if s[1] != 3], ids=sc.shape_id)
def test_channel_offsets(shape):
    """C = 2, 4, 5, 6, 7: each channel of the output equals the oracle of THAT channel computed alone, as a C = 1 problem with
    the same taps -- on the colour routes (triples by kernel 19 / 17, leftovers by kernel 16 with c0 = 3, 4, ...) and on the
    kernels that loop over channels themselves.  A wrong c0 or plane stride shows as a permuted or repeated channel."""
    B, C, H, W, ks = shape
    case, _ = _oracle('int', shape, 31)
    alone = [so.forward(case[0][:, c:c + 1].contiguous().numpy(), case[1].numpy(), case[2].numpy(), ks, f64=True) for c in range(C)]
    assert all(not np.array_equal(alone[a], alone[b]) for a in range(C) for b in range(a))      # a swap cannot go unseen
    inp, v, h = _dev(case)
    want = _dev(alone)
    assert _route(shape, 0) == (19 if C >= 3 else 16) and _route(shape, 17) == (17 if C >= 3 else 16)
    for variant in (0, 17, 19, 14, 15, 4, 16, 18):
        with _Variant(variant):
            out = _forward(inp, v, h, ks)
        for c in range(C):
            _assert_equal(out[:, c:c + 1], want[c], 'channel %d of %d, variant %d' % (c, C, variant))


# ---- nothing outside the output -----------------------------------------------------------------------------------------------

BAND = 4096
BAND_SHAPES = [(1, 1, 9, 132, 51), (1, 3, 17, 132, 51), (2, 7, 5, 4, 51), NARROW]


@pytest.mark.parametrize('variant', [0, 16, 18, 19, 20])
@pytest.mark.parametrize('shape', BAND_SHAPES, ids=lambda s: sc.shape_id(s) if len(s) == 5 else '%dx%d' % s)
def test_nothing_is_written_outside_the_output(shape, variant):
    """The output is a 16-byte-aligned view in the middle of a larger allocation filled with a sentinel, 4,096 floats on either
    side: lanes with x >= W or y >= H store nothing, so the bands keep the sentinel bit for bit and the view equals the oracle.
    (The operands are not banded: this test adds no read outside them.)"""
    if len(shape) == 2:
        shape = sc.fwd_persistent_shape(shape, _cus())
    B, C, H, W, ks = shape
    case, ref = _oracle('int', shape, 32 if C == 1 and B > 8 else 31)
    inp, v, h = _dev(case)
    n = B * C * H * W
    fill = 7.5
    buf = torch.full((BAND + n + BAND,), fill, device=DEV)
    view = buf[BAND:BAND + n].view(B, C, H, W)
    assert view.data_ptr() % 16 == 0 and view.is_contiguous() and BAND % 4 == 0
    with _Variant(variant):
        _native.check(_launch(inp, v, h, view, ks), 'tai_sepconv_forward')
    torch.cuda.synchronize()
    assert bool((buf[:BAND] == fill).all()), 'band in front of the output was written'
    assert bool((buf[BAND + n:] == fill).all()), 'band behind the output was written'
    _assert_equal(view, _dev([ref])[0], 'output of variant %d' % variant)


# ---- stale and non-finite values ------------------------------------------------------------------------------------------------

def _poison_lds(cus):
    """Launches on all-NaN frames, more than two tiles per CU, with each kernel family the narrow cases run on: every patch
    slot of every CU (both buffers of the persistent kernel, the three channel patches of the colour kernels) then holds NaN."""
    ks, H, W = 51, 32, 256
    B = next(b for b in range(1, 1 << 20) if sc.fwd_tiles(b, H, W) > 2 * cus and sc.fwd_tiles(b, H, W) % 8 == 0)
    taps = torch.zeros(B, ks, H, W, device=DEV)
    for C, variants in ((1, (0, 16, 18)), (3, (19, 17))):
        nan = torch.full((B, C, H + ks - 1, W + ks - 1), float('nan'), device=DEV)
        if C == 1:
            assert 21 <= _route((B, 1, H, W, ks), 0) <= 27 and sc.fwd_rounds(B, H, W, cus)[0] >= 3
        for variant in variants:
            with _Variant(variant):
                out = _forward(nan, taps, taps, ks)
            assert bool(torch.isnan(out).all())         # the launch ran: NaN x 0 is NaN


@pytest.mark.parametrize('shape', [NARROW, (1, 3, 17, 132, 51), (1, 1, 16, 124, 51)],
                         ids=lambda s: sc.shape_id(s) if len(s) == 5 else '%dx%d' % s)
def test_stale_and_nonfinite_lds_cannot_reach_an_output(shape):
    """stage_patch_dma does not write the patch columns past the frame edge in the last column tile: they hold whatever the
    CU's LDS held, here NaN from the launches before.  Only lanes with x >= W read them, and those store nothing: the result
    is exactly the oracle.  (Best effort: where a CU's LDS is not reused the check is vacuous.)"""
    cus = _cus()
    if len(shape) == 2:
        shape = sc.fwd_persistent_shape(shape, cus)
    B, C, H, W, ks = shape
    case, ref = _oracle('int', shape, 32 if C == 1 and B > 8 else 31)
    inp, v, h = _dev(case)
    want, = _dev([ref])
    for variant in ((0, 19, 17) if C == 3 else (0, 18, 16, 23)):
        _poison_lds(cus)
        with _Variant(variant):
            _assert_equal(_forward(inp, v, h, ks), want, 'variant %d after NaN launches' % variant)


@pytest.mark.parametrize('shape,image', [(NARROW, None), ((2, 3, 33, 260, 51), 0)], ids=['20x132', '2x3x33x260-ks51'])
def test_a_nonfinite_image_stays_in_its_image(shape, image):
    """One image all NaN: every other image is exactly the oracle (the persistent kernel stages image b + 1's patch into the
    other buffer while image b computes; a workgroup of the colour kernel holds three channel patches), the NaN image is all NaN."""
    cus = _cus()
    if len(shape) == 2:
        shape = sc.fwd_persistent_shape(shape, cus)
    B, C, H, W, ks = shape
    image = B // 2 if image is None else image
    case, ref = _oracle('int', shape, 32 if C == 1 else 31)
    inp, v, h = _dev(case)
    want, = _dev([ref])
    inp[image] = float('nan')
    others = [b for b in range(B) if b != image]
    for variant in ((0, 19, 17, 16) if C == 3 else (0, 21, 23, 18, 16)):
        with _Variant(variant):
            out = _forward(inp, v, h, ks)
        assert bool(torch.isnan(out[image]).all()), 'variant %d: the NaN image has finite outputs' % variant
        _assert_equal(out[others], want[others], 'variant %d, the images next to a NaN image' % variant)


# ---- float data: the rounding guard ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', sc.FWD_FIXED_SHAPES + sc.FWD_PERSISTENT_PLANES,
                         ids=lambda s: sc.shape_id(s) if len(s) == 5 else '%dx%d' % s)
def test_default_route_matches_the_oracle_on_float_data(shape):
    if len(shape) == 2:
        shape = sc.fwd_persistent_shape(shape, _cus())
    ks = shape[4]
    case, ref = _oracle('float', shape, 34, keep=shape[:4] in ((1, 3, 17, 132), sc.fwd_persistent_shape(NARROW, _cus())[:4]))
    inp, v, h = _dev(case)
    err = _rel(_forward(inp, v, h, ks).cpu().numpy(), ref)
    print(sc.shape_id(shape), 'kernel', _route(shape, 0), 'error', err)
    assert err < FWD_TOL, err


@pytest.mark.parametrize('shape', [(1, 3, 17, 132, 51), NARROW], ids=['1x3x17x132-ks51', '20x132'])
def test_every_variant_matches_the_oracle_on_float_data(shape):
    if len(shape) == 2:
        shape = sc.fwd_persistent_shape(shape, _cus())
    ks = shape[4]
    case, ref = _oracle('float', shape, 34)
    inp, v, h = _dev(case)
    worst = {}
    for variant in sc.FWD_VARIANTS:
        with _Variant(variant):
            worst[variant] = _rel(_forward(inp, v, h, ks).cpu().numpy(), ref)
    print(sc.shape_id(shape), 'largest error', max(worst.values()))
    bad = {k: e for k, e in worst.items() if not e < FWD_TOL}
    assert not bad, bad


# ---- side stream, graph replay --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [(1, 3, 17, 132, 51), NARROW], ids=['1x3x17x132-ks51', '20x132'])
def test_colour_route_and_narrow_persistent_plane_on_a_side_stream_and_inside_a_graph(shape):
    """tests/test_gpu_sepconv.py's test_runs_on_a_side_stream_and_inside_a_graph for kernel 19 on two column tiles and for the
    persistent kernel with a 4-column last tile; integer data, so the results are exact -- the replay's too: it reads the
    CURRENT contents of the captured buffers, the frames times 0.5, a power of two."""
    if len(shape) == 2:
        shape = sc.fwd_persistent_shape(shape, _cus())
    B, C, H, W, ks = shape
    assert _route(shape, 0) == (19 if C == 3 else _expected_route(shape, 0, _cus())) and _route(shape, 0) not in (1, 16, 18)
    case, ref = _oracle('int', shape, 32 if C == 1 else 31)
    inp, v, h = _dev(case)
    want, = _dev([ref])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        out = vfi.SeparableConvolution.apply(inp, v, h, ks)
    s.synchronize()
    _assert_equal(out, want, 'on a side stream')
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        gout = vfi.SeparableConvolution.apply(inp, v, h, ks)
    inp.mul_(0.5)
    gout.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    _assert_equal(gout, 0.5 * want, 'graph replay on the halved frames')
    assert sepconv.set_forward_variant(0) == 0          # nothing above left a variant selected
