"""The Winograd kernels straight through the C ABI, on every instance, plan and seam: the cases of tests/wino_cases.py (conditions checked
without a GPU in tests/test_wino_cases_cpu.py).

  * Each case first asserts its plan through the launcher's own decision -- tai_conv3x3_wino_forward_plan (with the weight buffer the launch
    reads, so the split-bf16 arithmetic is part of the answer), tai_conv3x3_wino_wrw_plan, tai_conv3x3_wino43_splits -- so that "K = 70 runs
    the 128 x 32 workgroups" is a fact about the launch and not about the Python restatement.
  * F(2x2, 3x3) forward, its split-bf16 arithmetic and its weight gradient on integer data (+-512 outliers on the tile-block, image,
    channel-part, lane and split seams; every stage of the algorithm below 2^24) must EQUAL float64 in y, ypool, y2 / the sum, dw and db;
    the tanh instances run float data under 4e-6 of 1 + the magnitude sum.
  * F(4x4, 3x3) forward, its displaced-read (BLOCKS) and split-over-channels (SPLITC) forms: 2e-5 of 1 + the largest magnitude sum of
    the output's 4 x 4 tile; ypool == max_pool2d(y) and y2 == y + unpool(addx) exactly.  Weight gradient at tile 4: 2e-5 sqrt(N H W) on
    float data, one-hot probes on the block and split seams to 2e-5.
  * Tile independence, bit for bit, on every forward case: (a) an image launched alone gives its slice of the batch, (b) a slice of the
    output channels that crosses a 64-block gives its slice, (c) with every other image overwritten by NaN the image's bits do not move
    (a test of its own per case with more than one image; what it caught in the F(2x2, 3x3) fp32 kernel is in that test's docstring).
    The workspace entry point (tai_conv3x3_wino43_forward_ws) gets (c) only: N and K change its split plan.
  * Every tensor sits inside guard bands: NaN round the inputs, a non-integer sentinel round outputs and workspaces (whose interior
    starts as NaN); the bands are asserted after every launch.
  * Displaced reads at k = 9 (S = 3 with no zero tail: the zero_taps == 0 branch) on both launchers against float64 F.conv2d(padding=4),
    plane and block weights built from the header's geometry.

The worst figure of every family is printed by the module's last test (committed as profiles/wino_pin_errors.txt)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from video_frame_inpainting_amd import _native

import wino_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -1234.5          # finite and no integer
BAND = 4096                 # floats on either side of every buffer: a multiple of 64, so 16-byte alignment holds
WORST = {}                  # family -> (figure, case id)


def _s():
    return torch.cuda.current_stream().cuda_stream


def _count(family, hit, ident):
    """One more case of `family` (a count of cases that must stay 0); the first case that hit names it."""
    n, first = WORST.get(family, (0, '-'))
    WORST[family] = (n + int(hit), ident if hit and not n else first)


def _note(family, value, ident):
    if family not in WORST or value > WORST[family][0]:
        WORST[family] = (value, ident)


class _Framed(object):
    """A float tensor as a 16-byte-aligned view in the middle of a larger buffer.  Inputs: NaN bands.  Outputs and workspaces: SENTINEL
    bands around an interior of NaN."""

    def __init__(self, src=None, shape=None, out=False):
        shape = tuple(src.shape) if shape is None else tuple(shape)
        n = int(np.prod(shape))
        self.fill = SENTINEL if out else float('nan')
        self.buf = torch.full((2 * BAND + n,), self.fill, device=DEV)
        self.t = self.buf[BAND:BAND + n].view(shape)
        if src is not None:
            self.t.copy_(src)
        elif out:
            self.t.fill_(float('nan'))
        assert self.t.data_ptr() % 16 == 0 and self.t.is_contiguous()

    def ptr(self):
        return self.t.data_ptr()

    def bands_untouched(self, name):
        assert self.fill == SENTINEL
        assert bool((self.buf[:BAND] == SENTINEL).all()), 'the band in front of %s was written' % name
        assert bool((self.buf[BAND + self.t.numel():] == SENTINEL).all()), 'the band behind %s was written' % name


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_equal(got, want, what):
    """got (fp32) equals want (float64) element for element; a NaN in got (a store that never happened) differs from everything."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g = got.double()
    if not torch.equal(g, want):
        bad = (g != want).nonzero()
        first = tuple(int(i) for i in bad[0])
        raise AssertionError('%s: %d of %d elements differ (%d NaN), first at %r: got %r, want %r; max |diff| %g'
                             % (what, bad.shape[0], want.numel(), int(torch.isnan(g).sum()), first, float(g[first]), float(want[first]),
                                float((g - want).abs().nan_to_num(0).max())))


def _assert_same_bits(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(_bits(a), _bits(b)), '%s: %d of %d elements differ' % (what, int((_bits(a) != _bits(b)).sum()), a.numel())


def _unpooled(a):
    """a at [0::2, 0::2] of a plane twice the size, zero elsewhere: where the unpooling epilogue adds addx."""
    out = a.new_zeros(a.shape[0], a.shape[1], 2 * a.shape[2], 2 * a.shape[3])
    out[:, :, 0::2, 0::2] = a
    return out


def _ratio(got, ref, mag):
    err = (got.double() - ref).abs() / (1 + mag)
    return float('inf') if bool(torch.isnan(err).any()) else float(err.max())


# ---- F(2x2, 3x3) forward ----------------------------------------------------------------------------------------------------------

def _transform22(L, w3, K, C, arith):
    prev = L.tai_conv3x3_wino_set_arithmetic(1 if arith == 'split' else 0)
    try:
        n = L.tai_conv3x3_wino_weight_floats(K, C)
        assert n == (40 if arith == 'split' else 16) * (-(-K // wc.TM) * wc.TM) * (-(-C // wc.KC) * wc.KC)
        fw, U = _Framed(w3), _Framed(shape=(n,), out=True)
        _native.check(L.tai_conv3x3_wino_transform_weights(fw.ptr(), U.ptr(), K, C, _s()), 'tai_conv3x3_wino_transform_weights')
    finally:
        L.tai_conv3x3_wino_set_arithmetic(prev)
    torch.cuda.synchronize()
    U.bands_untouched('U')
    assert not bool(torch.isnan(U.t).any())
    return U


def _run22(c, x, w, b, addx, claim_plan=True):
    """One tai_conv3x3_wino_forward_ex launch of case c's form on host tensors (any N and K) -> {'y', 'pool', 'sum'} on the host, each where
    the epilogue produces it ('unpool_sum': y receives the sum, returned as 'sum')."""
    L = _native.lib()
    N, K, H, W = x.shape[0], w.shape[0], c.H, c.W
    if c.shift_k:               # the halo-carrying plane and the blocked weight, from the header's geometry
        plane, in_h, in_w, in_oy, in_ox = wc.halo_plane(x, c.shift_k)
        w3 = wc.block3x3_weight(w)
    else:
        plane, w3 = x, w
        in_h, in_w, in_oy, in_ox = c.window if c.window else (H, W, 0, 0)
    C = w3.shape[1]
    assert tuple(plane.shape) == (N, C if not c.shift_k else c.C, in_h, in_w)
    U = _transform22(L, w3, K, C, c.arith)
    try:
        has_pool, has_addx, has_y2 = c.epi == 'pool', c.epi.startswith('unpool'), c.epi == 'unpool'
        out = (ctypes.c_int * 9)()
        grid = L.tai_conv3x3_wino_forward_plan(c.nparts, c.shift_k, int(has_pool), int(has_addx), int(has_y2), N, C, K, H, W, in_h, in_w, in_oy, in_ox,
                                               wc.ACTS[c.act], U.ptr(), out)
        _native.check(grid if grid < 0 else 0, 'tai_conv3x3_wino_forward_plan')
        if claim_plan:          # the launcher's decision is the restated one: wc.fwd22_flags speaks about this launch
            want = wc.fwd22_plan(*wc._fwd22_args(c))
            assert dict(zip(wc.FWD_FIELDS, out)) == want and grid == want['grid'], (wc.fcase_id(c), list(out), want)
        parts = [_Framed(p.contiguous()) for p in plane.chunk(c.nparts, dim=1)]
        ptrs = (ctypes.c_void_p * c.nparts)(*[p.ptr() for p in parts])
        fb = _Framed(b)
        fy = _Framed(shape=(N, K, H, W), out=True)
        ph, pw, poy, pox = c.pool if c.pool else (0, 0, 0, 0)
        fpool = _Framed(shape=(N, K, ph or H // 2, pw or W // 2), out=True) if has_pool else None
        fadd = _Framed(addx) if has_addx else None
        fy2 = _Framed(shape=(N, K, H, W), out=True) if has_y2 else None
        rc = L.tai_conv3x3_wino_forward_ex(ptrs, c.nparts, c.shift_k, U.ptr(), fb.ptr(), fy.ptr(), fpool.ptr() if fpool else None, ph, pw, poy, pox,
                                           fadd.ptr() if fadd else None, fy2.ptr() if fy2 else None, N, C, K, H, W, in_h, in_w, in_oy, in_ox,
                                           wc.ACTS[c.act], _s())
        _native.check(rc, 'tai_conv3x3_wino_forward_ex')
        torch.cuda.synchronize()
    finally:
        L.tai_conv3x3_wino_forget_weights(U.ptr())
    res = {}
    for name, f in (('y', fy), ('pool', fpool), ('sum', fy2)):
        if f is not None:
            f.bands_untouched(name)
            res[name] = f.t.cpu()
    if c.pool:                  # the window of the pooled plane; everything around it keeps its NaN
        full = res['pool']
        res['pool'] = full[:, :, poy:poy + H // 2, pox:pox + W // 2].clone()
        full[:, :, poy:poy + H // 2, pox:pox + W // 2] = float('nan')
        assert bool(torch.isnan(full).all()), 'ypool was written outside its window'
    if c.epi == 'unpool_sum':
        res = {'sum': res['y']}
    return res


def _seam_images(N, tiles_per_image, wtn):
    """The first image, the image with the first block seam inside it (or at its start) and the last image."""
    return sorted({0, min(N - 1, wtn // tiles_per_image), N - 1})


def _slices_alone(run, x, w, b, addx, full, images, what):
    """(a) and (b) of the module's docstring around the outputs `full` of run(x, w, b, addx)."""
    K = w.shape[0]
    sub = lambda t, sl: None if t is None else t[sl].contiguous()
    for n in images:                                                                        # (a)
        alone = run(x[n:n + 1].contiguous(), w, b, sub(addx, slice(n, n + 1)))
        for name in full:
            _assert_same_bits(alone[name][0], full[name][n], '%s: image %d alone, %s' % (what, n, name))
    k0, k1 = (60, 70) if K >= 70 else (K // 3, max(K // 3 + 1, K - 1))                      # (b)
    part = run(x, w[k0:k1].contiguous(), b[k0:k1].contiguous(), None if addx is None else addx[:, k0:k1].contiguous())
    for name in full:
        _assert_same_bits(part[name], full[name][:, k0:k1], '%s: output channels %d:%d alone, %s' % (what, k0, k1, name))


def _poisoned_neighbours(run, x, w, b, addx, full, images, neighbours=float('nan')):
    """(c): every image but n overwritten with `neighbours` (NaN; +-512 alternating by channel where asked).  -> [(n, output, elements of
    image n whose bits moved)], empty when image n's bits are those of `full`."""
    moved = []
    for n in images:
        if x.shape[0] == 1:
            break
        poisoned = torch.full_like(x, neighbours)
        if neighbours == wc.OUTLIER:
            poisoned[:, 1::2] = -wc.OUTLIER
        poisoned[n] = x[n]
        got = run(poisoned, w, b, addx)
        for name in full:
            diff = int((_bits(got[name][n]) != _bits(full[name][n])).sum())
            if diff:
                moved.append((n, name, diff))
    return moved


@pytest.mark.parametrize('c', wc.FWD22_CASES, ids=wc.fcase_id)
def test_f22_forward_case(c):
    f = wc.fwd22_flags(c)
    assert all(f[name] for name in c.claims)
    x, w, b, addx = wc.fwd22_data(c)
    got = _run22(c, x, w, b, addx)
    ref = wc.conv_reference(x, w, b, c.H, c.W, None if c.shift_k else c.window, c.act, addx)
    assert set(got) == ({'sum'} if c.epi == 'unpool_sum' else {'y'} | ({'pool'} if c.epi == 'pool' else set()) | ({'sum'} if c.epi == 'unpool' else set()))
    family = 'F(2x2) %s %s' % (c.arith, c.data)
    for name in sorted(got):
        what = '%s %s' % (wc.fcase_id(c), name)
        if c.data == 'int':
            _note(family + ': elements that differ from float64', int((got[name].double() != ref[name]).sum()), what)
            _assert_equal(got[name], ref[name], what)
        else:
            mag = F.max_pool2d(ref['mag'], 2) if name == 'pool' else ref['mag'] + (0 if name != 'sum' else _unpooled(addx.double().abs()))
            r = _ratio(got[name], ref[name], mag)
            _note(family + ': max |got - ref| / (1 + mag)', r, what)
            assert r <= wc.TOL22, (what, r)
    run = lambda xx, ww, bb, aa: _run22(c, xx, ww, bb, aa, claim_plan=False)
    _slices_alone(run, x, w, b, addx, got, _images22(c), wc.fcase_id(c))


def _images22(c):
    return _seam_images(c.N, -(-c.H // 2) * -(-c.W // 2), wc.TTN if wc.fwd22_flags(c)['tall'] else wc.TN)


MANY22 = [c for c in wc.FWD22_CASES if c.N > 1]


@pytest.mark.parametrize('c', MANY22, ids=wc.fcase_id)
def test_f22_image_bits_do_not_depend_on_non_finite_neighbours(c):
    """(c) on an F(2x2, 3x3) forward case with more than one image (all of them): all other images NaN, the image's bits must not move.

    What it caught in the fp32 kernel (wino::conv3x3), both fixed in wino_conv.hip.inc:
      * 40 of the 70 cases -- every one in which an image ends inside a wave's run of tiles and its tile rows hold two tiles or more.  A
        patch row's outer columns come from the neighbouring lane by DPP, and the first and last tile of a tile row multiplied that value
        by a mask of 0.0 instead of not taking it: NaN in the next image's first tile became NaN in this image's last tile (and the other
        way round).  transform_rows now selects on a lane mask.
      * the 128 x 32 workgroups with an odd C (11 channels, K = 128): lanes 32-63 read channel c + 1, for c = C - 1 the next image's
        channel 0, times zero weights.  Those lanes now read nothing."""
    x, w, b, addx = wc.fwd22_data(c)
    run = lambda xx, ww, bb, aa: _run22(c, xx, ww, bb, aa, claim_plan=False)
    moved = _poisoned_neighbours(run, x, w, b, addx, run(x, w, b, addx), _images22(c))
    _count('F(2x2): cases whose image bits move among NaN neighbours', bool(moved), wc.fcase_id(c))
    assert not moved, moved


@pytest.mark.parametrize('c', MANY22, ids=wc.fcase_id)
def test_f22_image_bits_do_not_depend_on_finite_neighbours(c):
    """The same with +-512 in every other image (alternating by channel): finite neighbours never move a bit, on every case."""
    x, w, b, addx = wc.fwd22_data(c)
    run = lambda xx, ww, bb, aa: _run22(c, xx, ww, bb, aa, claim_plan=False)
    moved = _poisoned_neighbours(run, x, w, b, addx, run(x, w, b, addx), _images22(c), neighbours=wc.OUTLIER)
    assert not moved, moved


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------

def _wrw(c, x, dy, claim_plan=True):
    """One tai_conv3x3_wino_wrw(_window) launch under case c's settings -> (dw, db or None) on the host."""
    L = _native.lib()
    N, C, K, H, W = x.shape[0], x.shape[1], dy.shape[1], c.H, c.W
    prev = (L.tai_conv3x3_wino_wrw_set_tile(c.tile), L.tai_conv3x3_wino_wrw_set_paired(int(c.paired)), L.tai_conv3x3_wino43_set_placement(c.placement))
    try:
        out = (ctypes.c_int * 8)()
        grid = L.tai_conv3x3_wino_wrw_plan(N, C, K, H, W, *(c.window or (0, 0, 0, 0)), out)
        _native.check(grid if grid < 0 else 0, 'tai_conv3x3_wino_wrw_plan')
        if claim_plan:
            want = wc.wrw_plan(N, C, K, H, W, c.window, c.tile, c.paired)
            assert dict(zip(wc.WRW_FIELDS, out)) == want and want['tile'] == c.tile, (wc.gcase_id(c), list(out), want)
        floats = L.tai_conv3x3_wino_wrw_workspace_floats(N, C, K, H, W)
        assert floats > 0
        fx, fdy, ws = _Framed(x), _Framed(dy), _Framed(shape=(floats,), out=True)
        fdw = _Framed(shape=(K, C, 3, 3), out=True)
        fdb = _Framed(shape=(K,), out=True) if c.bias else None
        if c.window:
            rc = L.tai_conv3x3_wino_wrw_window(fx.ptr(), fdy.ptr(), fdw.ptr(), fdb.ptr() if fdb else None, ws.ptr(), N, C, K, H, W, *c.window, _s())
        else:
            rc = L.tai_conv3x3_wino_wrw(fx.ptr(), fdy.ptr(), fdw.ptr(), fdb.ptr() if fdb else None, ws.ptr(), N, C, K, H, W, _s())
        _native.check(rc, 'tai_conv3x3_wino_wrw')
        torch.cuda.synchronize()
    finally:
        L.tai_conv3x3_wino_wrw_set_tile(prev[0])
        L.tai_conv3x3_wino_wrw_set_paired(prev[1])
        L.tai_conv3x3_wino43_set_placement(prev[2])
    for name, f in (('dw', fdw), ('db', fdb), ('workspace', ws)):
        if f is not None:
            f.bands_untouched(name)
    return fdw.t.cpu(), fdb.t.cpu() if fdb else None


@pytest.mark.parametrize('c', wc.WRW_CASES, ids=wc.gcase_id)
def test_weight_gradient_case(c):
    f = wc.wrw_flags(c)
    assert all(f[name] for name in c.claims)
    if c.tile == 2:             # exact: integers with outliers
        x, dy = wc.wrw_data(c)
        dw, db = _wrw(c, x, dy)
        rw, rb = wc.wrw_reference(x, dy, c.H, c.W, c.window)
        _note('wrw tile 2 int: elements that differ from float64', int((dw.double() != rw).sum()), wc.gcase_id(c))
        _assert_equal(dw, rw, wc.gcase_id(c) + ' dw')
        if c.bias:
            _assert_equal(db, rb, wc.gcase_id(c) + ' db')
        return
    # tile 4: tests/test_gpu_wino_conv.py's bound on outlier-free float data, sums of N H W products of unit-variance terms
    x, dy = wc.wrw_data(c, outliers=False, integers=False)
    dw, db = _wrw(c, x, dy)
    rw, rb = wc.wrw_reference(x, dy, c.H, c.W, c.window)
    scale = (c.N * c.H * c.W) ** 0.5
    assert not bool(torch.isnan(dw).any())
    err = float((dw.double() - rw).abs().max()) / scale
    _note('wrw tile 4 float: max |dw - ref| / sqrt(N H W)', err, wc.gcase_id(c))
    assert err <= 2e-5, err
    if c.bias:
        eb = float((db.double() - rb).abs().max()) / scale
        _note('wrw tile 4 float: max |db - ref| / sqrt(N H W)', eb, wc.gcase_id(c))
        assert eb <= 2e-5, eb
    again = _wrw(c, x, dy, claim_plan=False)
    assert torch.equal(_bits(again[0]), _bits(dw))                   # fixed reduction order


def test_weight_gradient_rows_shorter_than_16_pixels_through_the_widening():
    """conv_ops.wino_weight_grad widens W = 8 and W = 4 to 16 columns with zeros before the (even H, W % 16 == 0) kernel: integers, exact."""
    from video_frame_inpainting_amd import conv_ops
    prev = conv_ops.set_weight_gradient_tile(2)
    try:
        for (N, C, K, H, W) in ((5, 24, 70, 8, 8), (9, 8, 8, 4, 4), (3, 70, 24, 6, 12)):
            c = wc.GCase(N, C, K, H, W, None, 2, True, True, 1, ())
            x, dy = wc.wrw_data(c)
            dw, db = conv_ops.wino_weight_grad(x.to(DEV), dy.to(DEV), with_bias=True)
            rw, rb = wc.wrw_reference(x, dy, H, W)
            _assert_equal(dw.cpu(), rw, 'widened %r dw' % ((N, C, K, H, W),))
            _assert_equal(db.cpu(), rb, 'widened %r db' % ((N, C, K, H, W),))
    finally:
        conv_ops.set_weight_gradient_tile(prev)


def _probe_sites(c):
    """Tiles on either side of every split boundary and of the first chunk seam, as (n, row, column) of the tile's first pixel."""
    p = wc.wrw_plan(c.N, c.C, c.K, c.H, c.W, c.window, c.tile, c.paired)
    tw, th = c.W // 4, c.H // 4
    cuts = [s * p['chunks_per_split'] * 4 for s in range(1, p['splits'])] + [4]
    tiles = sorted({t for cut in cuts for t in (cut - 1, cut) if 0 <= t < c.N * th * tw} | {0, c.N * th * tw - 1})
    return [(t // (th * tw), 4 * ((t // tw) % th), 4 * (t % tw)) for t in tiles]


@pytest.mark.parametrize('c', [wc.WRW_CASES[10], wc.WRW_CASES[16]], ids=wc.gcase_id)
def test_weight_gradient_tile_4_probes(c):
    """One-hot probes on (2, 70, 130, 32, 64) (9 blocks of 64 x 32, 64 chunks, splits of 3 and a last split of 1) and (3, 40, 70, 4, 48):
    dy one-hot in the tile on either side of every split boundary -> dw[k] is an integer patch of x, to 2e-5; x one-hot with integer dy
    -> dw[:, c] is a patch of dy.  k in {63, 64, K - 1}, c in {31, 32, C - 1}: the last and first rows of the 64 x 32 blocks."""
    assert c.tile == 4 and not c.window
    g = torch.Generator().manual_seed(3)
    sites = _probe_sites(c)
    assert len(sites) >= 4
    ks, cs = sorted({63, 64, c.K - 1}), sorted({31, 32, c.C - 1})
    x = torch.randint(-4, 5, (c.N, c.C, c.H, c.W), generator=g).float()
    dyi = torch.randint(-2, 3, (c.N, c.K, c.H, c.W), generator=g).float()
    xp, dyp = F.pad(x, (1, 1, 1, 1)), F.pad(dyi, (1, 1, 1, 1))
    worst = 0.0
    for j, (n, r, col) in enumerate(sites):
        k, ch = ks[j % len(ks)], cs[j % len(cs)]
        py, px = r + (j % 4), col + 3 * (j % 2)                    # a pixel of that tile: first or last column, any row
        dy = torch.zeros(c.N, c.K, c.H, c.W)
        dy[n, k, py, px] = 1.0
        dw, _ = _wrw(c, x, dy, claim_plan=(j == 0))
        want = torch.zeros(c.K, c.C, 3, 3)
        want[k] = xp[n, :, py:py + 3, px:px + 3]
        worst = max(worst, float((dw - want).abs().max()))
        assert float((dw - want).abs().max()) <= 2e-5, ('dy one-hot', n, k, py, px, float((dw - want).abs().max()))
        xo = torch.zeros(c.N, c.C, c.H, c.W)
        xo[n, ch, py, px] = 1.0
        dw, _ = _wrw(c, xo, dyi, claim_plan=False)
        want = torch.zeros(c.K, c.C, 3, 3)
        # dw[k, ch, a, b] = dy[n, k, py - a + 1, px - b + 1]
        want[:, ch] = dyp[n, :, py:py + 3, px:px + 3].flip(1, 2)
        worst = max(worst, float((dw - want).abs().max()))
        assert float((dw - want).abs().max()) <= 2e-5, ('x one-hot', n, ch, py, px, float((dw - want).abs().max()))
    _note('wrw tile 4 probes: max |dw - patch|', worst, wc.gcase_id(c))


# ---- F(4x4, 3x3) forward ----------------------------------------------------------------------------------------------------------

def _run43(c, x, w, b, addx, claim_plan=True):
    """One launch of case c's form (tai_conv3x3_wino43_forward_ex / _ws / _blocks) -> {'y', 'pool', 'sum'} on the host."""
    L = _native.lib()
    N, K, H, W = x.shape[0], w.shape[0], c.H, c.W
    if c.form == 'blocks':
        plane, in_h, in_w, in_oy, in_ox = wc.halo_plane(x, c.shift_k)
        w3 = wc.block3x3_weight(w)
    else:
        plane, w3 = x, w
    C = w3.shape[1]
    n = L.tai_conv3x3_wino43_weight_floats(K, C)
    fw, U = _Framed(w3), _Framed(shape=(n,), out=True)
    _native.check(L.tai_conv3x3_wino43_transform_weights(fw.ptr(), U.ptr(), K, C, _s()), 'tai_conv3x3_wino43_transform_weights')
    has_pool, has_addx, has_y2 = c.epi == 'pool', c.epi.startswith('unpool'), c.epi == 'unpool'
    parts = [_Framed(p.contiguous()) for p in plane.chunk(c.nparts, dim=1)]
    ptrs = (ctypes.c_void_p * c.nparts)(*[p.ptr() for p in parts])
    fb = _Framed(b)
    fy = _Framed(shape=(N, K, H, W), out=True)
    fpool = _Framed(shape=(N, K, H // 2, W // 2), out=True) if has_pool else None
    fadd = _Framed(addx) if has_addx else None
    fy2 = _Framed(shape=(N, K, H, W), out=True) if has_y2 else None
    opt = (fpool.ptr() if fpool else None, fadd.ptr() if fadd else None, fy2.ptr() if fy2 else None)
    ws = None
    prev = L.tai_conv3x3_wino43_set_placement(c.placement)
    try:
        if c.form == 'blocks':
            rc = L.tai_conv3x3_wino43_forward_blocks(parts[0].ptr(), c.shift_k, U.ptr(), fb.ptr(), fy.ptr(), opt[0], 0, 0, 0, 0, N, C, K, H, W, in_h, in_w,
                                                     in_oy, in_ox, wc.ACTS[c.act], _s())
        elif c.form == 'ws':
            cps = ctypes.c_int()
            splits = L.tai_conv3x3_wino43_splits(N, C, K, H, W, c.nparts, ctypes.byref(cps))
            if claim_plan:
                assert (splits, cps.value) == wc.w43_splits(N, C, K, H, W, c.nparts) and splits > 1, (wc.hcase_id(c), splits, cps.value)
            floats = L.tai_conv3x3_wino43_workspace_floats(N, C, K, H, W, c.nparts)
            assert floats == (splits * N * K * H * W if splits > 1 else 0)
            ws = _Framed(shape=(max(floats, 1),), out=True)
            rc = L.tai_conv3x3_wino43_forward_ws(ptrs, c.nparts, U.ptr(), fb.ptr(), fy.ptr(), *opt, ws.ptr(), floats, N, C, K, H, W, wc.ACTS[c.act], _s())
        else:
            rc = L.tai_conv3x3_wino43_forward_ex(ptrs, c.nparts, U.ptr(), fb.ptr(), fy.ptr(), *opt, N, C, K, H, W, wc.ACTS[c.act], _s())
        _native.check(rc, 'tai_conv3x3_wino43 ' + c.form)
        torch.cuda.synchronize()
    finally:
        L.tai_conv3x3_wino43_set_placement(prev)
    U.bands_untouched('U')
    res = {}
    for name, f in (('y', fy), ('pool', fpool), ('sum', fy2), ('workspace', ws)):
        if f is not None:
            f.bands_untouched(name)
            if name != 'workspace':
                res[name] = f.t.cpu()
    if c.epi == 'unpool_sum':
        res = {'sum': res['y']}
    return res


@pytest.mark.parametrize('c', wc.W43_CASES, ids=wc.hcase_id)
def test_f43_forward_case(c):
    f = wc.w43_flags(c)
    assert all(f[name] for name in c.claims)
    x, w, b, addx = wc.w43_data(c)
    got = _run43(c, x, w, b, addx)
    ref = wc.conv_reference(x, w, b, c.H, c.W, None, c.act, addx)
    family = 'F(4x4) %s: max |got - ref| / (1 + tile mag)' % c.form
    if c.epi == 'unpool_sum':
        r = wc.tile_ratio(got['sum'], ref['sum'], ref['mag'] + _unpooled(addx.double().abs()))
        _note(family, r, wc.hcase_id(c) + ' sum')
        assert r <= wc.TOL43, r
    else:
        r = wc.tile_ratio(got['y'], ref['y'], ref['mag'])
        _note(family, r, wc.hcase_id(c) + ' y')
        assert r <= wc.TOL43, r
        if c.epi == 'pool':
            _assert_same_bits(got['pool'], F.max_pool2d(got['y'], 2), wc.hcase_id(c) + ' ypool == max_pool2d(y)')
        if c.epi == 'unpool':
            want = got['y'].clone()
            want[:, :, 0::2, 0::2] += addx
            _assert_same_bits(got['sum'], want, wc.hcase_id(c) + ' y2 == y + unpool(addx)')
    if c.form != 'ws':          # (the workspace entry point: N and K change its split plan)
        run = lambda xx, ww, bb, aa: _run43(c, xx, ww, bb, aa, claim_plan=False)
        _slices_alone(run, x, w, b, addx, got, _seam_images(c.N, (c.H // 4) * (c.W // 4), wc.W43_TN), wc.hcase_id(c))


@pytest.mark.parametrize('c', [c for c in wc.W43_CASES if c.N > 1], ids=wc.hcase_id)
def test_f43_image_bits_do_not_depend_on_non_finite_neighbours(c):
    """(c) on an F(4x4, 3x3) forward case with more than one image (all of them): all other images NaN, the image's bits must not move.
    On the one-part ragged-C route the neighbours are +-512 instead: there the padded channels of the last chunk read the next image's
    first channels and rely on their zero weights (open) -- a NaN in image n + 1 becomes a NaN in image n, which is that
    known defect and not a seam this module pins."""
    x, w, b, addx = wc.w43_data(c)
    run = lambda xx, ww, bb, aa: _run43(c, xx, ww, bb, aa, claim_plan=False)
    ragged_one_part = wc.w43_flags(c)['ragged_c'] and c.nparts == 1
    moved = _poisoned_neighbours(run, x, w, b, addx, run(x, w, b, addx), _seam_images(c.N, (c.H // 4) * (c.W // 4), wc.W43_TN),
                                 neighbours=wc.OUTLIER if ragged_one_part else float('nan'))
    _count('F(4x4): cases whose image bits move among NaN neighbours', bool(moved), wc.hcase_id(c))
    assert not moved, moved


def test_displaced_reads_at_k_9_on_both_launchers():
    """shift_k = 9: S = 3 and 3 S == k, so no block carries a zero tail (zero_tail / zero_taps == 0, the branch k = 5 and 7 never take).  Both
    launchers against float64 F.conv2d(padding=4) on a plane and block weights built from the header's geometry: F(2x2) exactly on
    integers (both workgroup shapes), F(4x4) under the tile bound.  (The same launches are among the cases; this test names them.)"""
    k = 9
    S, top, left, in_h, in_w = wc.halo_geometry(6, 6, k)
    assert (S, top, left, in_h, in_w) == (3, 4, 5, 14, 16) and 3 * S == k
    for K in (64, 128, 70):
        c = wc._f(3, 8, K, 6, 6, act='relu', shift_k=k)
        x, w, b, _ = wc.fwd22_data(c)
        assert w.shape == (K, 8, 9, 9)
        got = _run22(c, x, w, b, None)['y']
        _assert_equal(got, torch.relu(F.conv2d(x.double(), w.double(), b.double(), padding=4)), 'F(2x2) k = 9, K = %d' % K)
    for act in (None, 'relu'):
        c = wc._h(2, 4, 70, 8, 8, act=act, epi='pool', form='blocks', shift_k=k)
        x, w, b, _ = wc.w43_data(c)
        got = _run43(c, x, w, b, None)
        ref = wc.activate(F.conv2d(x.double(), w.double(), b.double(), padding=4), act)
        mag = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=4)
        r = wc.tile_ratio(got['y'], ref, mag)
        _note('F(4x4) blocks k = 9: max |got - ref| / (1 + tile mag)', r, wc.hcase_id(c))
        assert r <= wc.TOL43, r
        _assert_same_bits(got['pool'], F.max_pool2d(got['y'], 2), 'k = 9 ypool')


def test_zz_print_the_worst_figures():
    """Last in the module: the worst figure of every family over the cases that ran (profiles/wino_pin_errors.txt is this printout)."""
    print()
    for family in sorted(WORST):
        value, ident = WORST[family]
        print('%-62s %-12.4g %s' % (family, value, ident))
