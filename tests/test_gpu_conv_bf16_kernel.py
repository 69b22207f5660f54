"""The bf16 convolution kernel (csrc/conv_bf16.hip.inc) straight through the C ABI, on every tile plan and instance: the cases of
tests/bf16_cases.py (conditions checked without a GPU in tests/test_bf16_cases_cpu.py).

  * Each case first asserts its plan through tai_conv_bf16_plan -- the launcher's own decision -- so that "this shape runs the MW = 4
    instance with a ragged last group" is a fact about the launch and not about the Python restatement.
  * Integer cases (+-512 outliers on tile, image, channel-part and lane seams; every partial sum below 2^24) must EQUAL the float64
    reference for act none and ReLU, in y, ypool, y2 and the sum-into-y form: one missing, doubled or misplaced term fails.
    tanh and float cases keep tests/test_gpu_conv_bf16.py's bound, 1e-5 of the reference's maximum.
  * Every output is pre-filled with NaN inside a buffer of SENTINEL bands, every input sits between NaN bands: a skipped store shows
    as a NaN, a store outside the output changes a band, a value read from outside an input poisons a result.
  * Further: every tap alone (plain and transposed, k = 3, 5, 7), bf16 rounding ties through x and through the weights, the packed
    weight layout bit for bit, one image's bits across two plans (MW = 4 in a batch, MW = 2 alone), and a non-finite image inside a
    multi-image MW = 4 tile.

Measured on the MI355X: the 57 tests of this module run in 4 s (the largest single test, the 14 G multiply-add float64
reference of (700, 80, 10, 13, 7), takes 0.4 s); the integer cases are bit-equal to float64."""
import ctypes

import numpy as np
import pytest
import torch

from video_frame_inpainting_amd import _native

import bf16_cases as bc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -1234.5          # finite and no integer
BAND = 4096                 # floats on either side of every buffer
REL_TOL = 1e-5              # tests/test_gpu_conv_bf16.py's bound: max |got - ref| <= 1e-5 max |ref|


def _s():
    return torch.cuda.current_stream().cuda_stream


class _Framed(object):
    """A float tensor as a 16-byte-aligned view in the middle of a larger buffer.  Inputs: NaN bands.  Outputs: SENTINEL bands
    around an interior of NaN."""

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


def _plan(L, N, K, H, W, k):
    out = (ctypes.c_int * len(bc.PLAN_FIELDS))()
    blocks = L.tai_conv_bf16_plan(N, K, H, W, k, out)
    _native.check(blocks if blocks < 0 else 0, 'tai_conv_bf16_plan')
    return dict(zip(bc.PLAN_FIELDS, out), blocks=blocks)


def _assert_plan(L, N, K, H, W, k, mw):
    """The library's plan is the restated one (so bc.flags speaks about this launch) and runs the MW = `mw` instance."""
    got, want = _plan(L, N, K, H, W, k), bc.plan(N, K, H, W, k)._asdict()
    assert got == dict(want), ((N, K, H, W, k), got, want)
    assert got['MW'] == mw, ((N, K, H, W, k), got)


def _pack(L, w, K, C, k, transposed):
    n = L.tai_conv_bf16_weight_elems(K, C, k)
    _native.check(n if n < 0 else 0, 'tai_conv_bf16_weight_elems')
    assert n % 2 == 0
    fw, wp = _Framed(w), _Framed(shape=(n // 2,), out=True)
    _native.check(L.tai_conv_bf16_pack_weights(fw.ptr(), wp.ptr(), K, C, k, int(transposed), _s()), 'tai_conv_bf16_pack_weights')
    torch.cuda.synchronize()
    wp.bands_untouched('Wp')
    return wp


def _forward(x, w, b, k, act=None, nparts=1, transposed=False, epi='plain', addx=None, mw=None):
    """One tai_conv_bf16_forward on host tensors -> {'y': ..., 'pool': ..., 'sum': ...} on the host (fp32), as the epilogue `epi`
    produces them ('unpool_sum': y receives the sum and is returned as 'sum')."""
    L = _native.lib()
    N, C, H, W = x.shape
    K = w.shape[1] if transposed else w.shape[0]
    if mw is not None:
        _assert_plan(L, N, K, H, W, k, mw)
    wp = _pack(L, w, K, C, k, transposed)
    parts = [_Framed(p.contiguous()) for p in x.chunk(nparts, dim=1)]
    assert len(parts) == nparts and all(p.t.shape[1] == C // nparts for p in parts)
    ptrs = (ctypes.c_void_p * nparts)(*[p.ptr() for p in parts])
    fb = _Framed(b)
    fy = _Framed(shape=(N, K, H, W), out=True)
    fpool = _Framed(shape=(N, K, H // 2, W // 2), out=True) if epi == 'pool' else None
    fadd = _Framed(addx) if epi.startswith('unpool') else None
    fy2 = _Framed(shape=(N, K, H, W), out=True) if epi == 'unpool' else None
    rc = L.tai_conv_bf16_forward(ptrs, nparts, wp.ptr(), fb.ptr(), fy.ptr(), fpool.ptr() if fpool else None, fadd.ptr() if fadd else None,
                                 fy2.ptr() if fy2 else None, N, C, K, H, W, k, bc.ACTS[act], _s())
    _native.check(rc, 'tai_conv_bf16_forward')
    torch.cuda.synchronize()
    out = {}
    for name, f in (('y', fy), ('pool', fpool), ('sum', fy2)):
        if f is not None:
            f.bands_untouched(name)
            out[name] = f.t.cpu()
    if epi == 'unpool_sum':
        out = {'sum': out['y']}
    return out


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


def _assert_close(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not bool(torch.isnan(got).any()), '%s: %d elements were never stored' % (what, int(torch.isnan(got).sum()))
    err, scale = float((got.double() - want).abs().max()), float(want.abs().max())
    assert scale > 0 and err <= REL_TOL * scale, '%s: error %.3g > %.3g of the maximum %.3g' % (what, err, REL_TOL, scale)


def _run_case(c):
    x, w, b, addx = bc.case_data(c)
    got = _forward(x, w, b, c.k, c.act, c.nparts, c.transposed, c.epi, addx, mw=c.mw)
    ref = bc.reference(c, x, w, b, addx)
    if c.epi == 'unpool_sum':
        ref = {'sum': ref['sum']}
    assert set(got) == set(ref)
    return got, ref


def test_the_mfma_sums_integer_products_exactly():
    """The smallest single-tile case, (3, 16, 1, 1, 3), first: v_mfma_f32_16x16x32_bf16 on integer operands whose partial sums stay
    below 2^24 gives the float64 sum bit for bit (outcome recorded in DESIGN.md 4.10), and the float data of the same shape are within
    the module's bound.  Everything below that compares with torch.equal rests on this."""
    c = bc.FIRST_CASE
    got, ref = _run_case(c)
    diff = float((got['y'].double() - ref['y']).abs().max())
    print('integer case %s: max |gpu - float64| = %g' % (bc.case_id(c), diff))
    fgot, fref = _run_case(c._replace(data='float'))
    _assert_close(fgot['y'], fref['y'], 'float data at the same shape')
    _assert_equal(got['y'], ref['y'], bc.case_id(c))


@pytest.mark.parametrize('c', bc.CASES, ids=bc.case_id)
def test_case_matches_float64_of_bf16_operands(c):
    f = bc.case_flags(c)
    assert f['mw'] == c.mw and all(f[name] for name in c.claims)
    got, ref = _run_case(c)
    for name in sorted(ref):
        what = '%s %s' % (bc.case_id(c), name)
        if c.data == 'int' and c.act != 'tanh':
            _assert_equal(got[name], ref[name], what)
        else:
            _assert_close(got[name], ref[name], what)


@pytest.mark.parametrize('transposed', [False, True], ids=['plain', 'transposed'])
@pytest.mark.parametrize('k', [3, 5, 7])
def test_every_tap_alone(k, transposed):
    """Output channel o has ONE non-zero tap, t = o mod k^2, K = max(16, k^2) so that every tap has a channel of its own; 9 x 10 plane
    (border and, at every k, interior pixels), C = 24 (a ragged second chunk).  A tap that the pack or the kernel's tap walk puts
    at another offset, in either weight form, moves a whole output plane."""
    N, C, H, W, K = 2, 24, 9, 10, max(16, k * k)
    g = torch.Generator().manual_seed(100 + k)
    x = torch.randint(-4, 5, (N, C, H, W), generator=g).float()
    x[:, :, 0, 0], x[:, :, H - 1, W - 1], x[:, :, 0, W - 1], x[:, :, H - 1, 0] = 7., -7., 5., -5.
    vals = bc._nonzero(torch.randint(-3, 4, (K, C), generator=g).float())
    w = torch.zeros(K, C, k, k)
    for o in range(K):
        t = o % (k * k)
        w[o, :, t // k, t % k] = vals[o]
    if transposed:      # the ConvTranspose2d weight of the same convolution: [C][K], taps flipped
        wt = w.permute(1, 0, 2, 3).flip(2, 3).contiguous()
        assert torch.equal(bc.conv64(x, wt, torch.zeros(K), True), bc.conv64(x, w, torch.zeros(K), False))
        w = wt
    b = torch.randint(-8, 9, (K,), generator=g).float()
    got = _forward(x, w, b, k, transposed=transposed, mw=2)['y']
    ref = bc.conv64(x, w, b, transposed)
    for o in range(K):
        _assert_equal(got[:, o], ref[:, o], 'k=%d %s tap %d (output channel %d)' % (k, 'transposed' if transposed else 'plain', o % (k * k), o))


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('k', [3, 5, 7])
def test_x_is_rounded_to_nearest_even(k):
    """x holds every bf16 tie of 49 binades and its fp32 neighbours (bf16_cases.tie_values); centre-tap identity weight, K = C = 16,
    zero bias: y is bf16_round(x) bit for bit."""
    vals = bc.tie_values()
    N, C, H, W = 3, 16, 28, 28
    assert vals.numel() == N * C * H * W
    x = vals[torch.randperm(vals.numel(), generator=torch.Generator().manual_seed(k))].view(N, C, H, W)
    w = torch.zeros(C, C, k, k)
    w[torch.arange(C), torch.arange(C), k // 2, k // 2] = 1.
    got = _forward(x, w, torch.zeros(C), k)['y']
    want = bc.bf16_round(x).float()
    assert torch.equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())
    assert not torch.equal(_bits(want), _bits(x)) and int(((_bits(x) & 0xFFFF) == 0x8000).sum()) == vals.numel() // 3


@pytest.mark.parametrize('transposed', [False, True], ids=['plain', 'transposed'])
def test_weights_are_rounded_to_nearest_even(transposed):
    """The same through tai_conv_bf16_pack_weights: the centre tap of w[o][c] holds the tie values, image n is 1 in channel n alone,
    so y[n][o] is bf16_round(w[o][n]) bit for bit on all four pixels of a 2 x 2 plane."""
    vals = bc.tie_values()
    K, C, k = 256, 160, 3
    flat = torch.ones(K * C)
    flat[:vals.numel()] = vals
    centre = flat[torch.randperm(K * C, generator=torch.Generator().manual_seed(5))].view(K, C)
    w = torch.zeros(K, C, k, k)
    w[:, :, 1, 1] = centre
    if transposed:
        w = w.permute(1, 0, 2, 3).contiguous()
    x = torch.zeros(C, C, 2, 2)
    x[torch.arange(C), torch.arange(C)] = 1.
    got = _forward(x, w, torch.zeros(K), k, transposed=transposed)['y']
    want = bc.bf16_round(centre).float().t().contiguous().view(C, K, 1, 1).expand(C, K, 2, 2)
    assert torch.equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())


@pytest.mark.parametrize('transposed', [False, True], ids=['plain', 'transposed'])
@pytest.mark.parametrize('k', [3, 5, 7])
def test_pack_layout_is_the_documented_one(k, transposed):
    """K = 80, C = 40: two channel blocks and three chunks, both ragged, and at every k a padded tap; the zeros past K, C and k^2
    included."""
    K, C = 80, 40
    g = torch.Generator().manual_seed(7 * k + transposed)
    w = torch.randn((C, K, k, k) if transposed else (K, C, k, k), generator=g)
    w.view(-1)[:64] = bc.tie_values()[:64]
    L = _native.lib()
    wp = _pack(L, w, K, C, k, transposed)
    got = wp.t.cpu().numpy().view(np.uint16)
    want = bc.pack_layout(w, K, C, k, transposed)
    assert got.shape == want.shape == (2 * 3 * bc.ksteps(k) * 2048,)
    assert np.array_equal(got, want), int((got != want).sum())
    assert int((want == 0).sum()) >= want.size - K * C * k * k


@pytest.mark.parametrize('k', [3, 7])
def test_an_image_has_the_same_bits_on_both_plans(k):
    """Float data: image i of an MW = 4 launch equals the same image run alone (MW = 2, another tile, another IMG) bit for bit --
    the header's "an image's output does not depend on its batch"."""
    for (N, H, W) in ((8200, 4, 4), (128, 32, 32)):
        c = bc.Case(N, 16, H, W, k, 16, 1, 'relu', 'plain', False, 'float', 4, ())
        x, w, b, _ = bc.float_case(c, seed=3)
        many = _forward(x, w, b, k, 'relu', mw=4)['y']
        assert bc.plan(N, 16, H, W, k)[:4] != bc.plan(1, 16, H, W, k)[:4]
        for i in (0, N // 2, N - 1):
            one = _forward(x[i:i + 1].clone(), w, b, k, 'relu', mw=2)['y']
            assert torch.equal(_bits(one[0]), _bits(many[i])), (k, N, H, W, i, int((_bits(one[0]) != _bits(many[i])).sum()))


def test_non_finite_images_stay_alone_in_a_multi_image_tile():
    """(2100, 16, 7, 9, 3): MW = 4, 16 images to a tile, a ragged last group of 4.  NaN and Inf in image 5 and in image 2097 (inside,
    on the border, in the last channel): every other image -- their 15 and 3 tile neighbours among them -- keeps the bits of the
    clean run, and both poisoned images show it."""
    N, K, H, W, k = 2100, 16, 7, 9, 3
    p = bc.plan(N, K, H, W, k)
    assert (p.MW, p.IMG) == (4, 16) and N % p.IMG == 4
    c = bc.Case(N, K, H, W, k, 16, 1, None, 'plain', False, 'float', 4, ())
    clean, w, b, _ = bc.float_case(c, seed=11)
    x = clean.clone()
    bad = (5, N - 3)
    for n in bad:
        x[n, 15, 0, 0] = float('nan')
        x[n, 15, H - 1, W - 1] = float('inf')
        x[n, 0, H // 2, W - 1] = -float('inf')
        x[n, 3, H - 1, 0] = float('nan')
        x[n, 8, 0, W // 2] = float('inf')
    got = _forward(x, w, b, k, mw=4)['y']
    ref = _forward(clean, w, b, k, mw=4)['y']
    keep = torch.ones(N, dtype=torch.bool)
    keep[list(bad)] = False
    assert bool(torch.isfinite(ref).all())
    assert torch.equal(_bits(got[keep]), _bits(ref[keep])), sorted(set((_bits(got) != _bits(ref)).nonzero()[:, 0].tolist()) - set(bad))
    assert all(not bool(torch.isfinite(got[n]).all()) for n in bad)
