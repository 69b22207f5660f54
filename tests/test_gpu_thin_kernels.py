"""The thin-layer and pointwise kernels through the C ABI, each against a plain reference of the same operation:
csrc/thin_conv.hip.inc (conv_cin1, conv_cin1_pool, conv_cout1_3x3, conv_cout1_5x5, shift_stack, thin_wrw and its reduce),
csrc/bias_act.hip.inc (bias_act_vec4 / _scalar, unpool2x_add, convlstm_gates and its backward, act_pool2x2_forward /
_backward), the four window_scale_* tails of csrc/spectral_norm.hip.inc and the `pairs` kernel of csrc/upsample.hip.inc.

  * The convolutions and thin_wrw run integer cases (tests/thin_cases.py: +-512 outliers on wave seams, row ends, corners,
    the rows where thin_wrw's row segments meet, the first item of a second grid-stride pass; every partial sum below 2^24,
    asserted in tests/test_thin_cases_cpu.py) and must EQUAL F.conv2d in float64 / fp64 autograd: one missing, doubled or
    misplaced term fails.
  * bias_act (none / relu), unpool2x_add, act_pool2x2, window_scale_* and shift_stack are one fp32 operation per element and
    must equal the same expression in torch.  act_pool2x2's backward reference is built here (thin_cases.
    act_pool_backward_ref: first maximum in row-major order), on data full of ties.
  * The tanh forms and the ConvLSTM gates are held to the project's bounds: 2e-6 forward, 5e-6 backward, 2e-6 * (1 + sum of
    |terms|) for the convolutions.
  * One shape per launcher is just past its grid cap (thin_cases.STRIDED): the loop runs a second time, and the first and the
    last item of that pass are asserted on their own, so that a failure names the pass.
  * Every output is a 16-byte-aligned view inside a buffer filled with a sentinel, every input a view inside a buffer of NaN,
    max(4096, 2 k W) floats on either side: the bands must come back untouched, and a value read from outside poisons a
    result that has to be exact.
All data are finite."""
import pytest
import torch
import torch.nn.functional as F

from video_frame_inpainting_amd import _native

import thin_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -1234.5          # finite and no integer: an element a kernel never wrote cannot equal an integer reference
FWD_TOL, BWD_TOL = 2e-6, 5e-6       # tests/test_gpu_model.py's bounds for the gates; FWD_TOL * (1 + mag): test_gpu_thin_conv.py's
UPS_TOL = 2e-6              # tests/test_gpu_upsample.py: the pairs kernel against ATen's fp32 kernel


def _s():
    return torch.cuda.current_stream().cuda_stream


def _band(k=1, W=0):
    return max(4096, 2 * k * W)


class _Framed(object):
    """A tensor as a view in the middle of a larger buffer: NaN around an input, SENTINEL around (and in) an output."""

    def __init__(self, src, band, fill, shape=None, offset=0):
        assert band % 4 == 0
        shape = tuple(src.shape) if shape is None else tuple(shape)
        n = 1
        for d in shape:
            n *= d
        self.band, self.fill, self.n, self.offset = band, fill, n, offset
        self.buf = torch.full((band + offset + n + band,), fill, device=DEV)
        self.t = self.buf[band + offset:band + offset + n].view(shape)
        if src is not None:
            self.t.copy_(src)
        assert self.t.data_ptr() % 16 == 4 * (offset % 4) and self.t.is_contiguous()

    def ptr(self):
        return self.t.data_ptr()

    def bands_untouched(self, name):
        lo, hi = self.buf[:self.band + self.offset], self.buf[self.band + self.offset + self.n:]
        assert bool((lo == self.fill).all()), 'the band in front of %s was written' % name
        assert bool((hi == self.fill).all()), 'the band behind %s was written' % name


def _in(src, band):
    return _Framed(src, band, float('nan'))


def _out(shape, band, src=None):
    return _Framed(src, band, SENTINEL, shape=shape)


def _assert_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        first = tuple(int(i) for i in bad[0])
        raise AssertionError('%s: %d of %d elements differ, first at %r: got %r, want %r'
                             % (what, bad.shape[0], want.numel(), first, float(got[first]), float(want[first])))


def _assert_close(got, want, tol, what, mag=None):
    err = (got.double() - want.double()).abs()
    err = float((err / (1 + mag)).max()) if mag is not None else float(err.max())
    assert err <= tol, '%s: error %.3g > %.3g' % (what, err, tol)


def _second_pass(launcher, shape, got, want, what, tol=None):
    """The first and the last work item of the second grid-stride pass, before the whole tensor."""
    assert tc.passes(launcher, shape) == 2
    for name, idx in zip(('first', 'last'), tc.second_pass(launcher, shape)):
        view, index = tc.item_slices(launcher, shape, idx)
        a, b = got.reshape(view)[index], want.reshape(view)[index]
        label = '%s: the %s item of the second pass (work item %d)' % (what, name, idx)
        if tol is None:
            _assert_equal(a.double(), b.double(), label)
        else:
            _assert_close(a, b, tol, label)


_REF = {}


def _cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _conv_case(launcher, shape, seed=11):
    """(x, w, b on the host; F.conv2d of them in float64, before the activation): computed once, shared, never written to."""
    def make():
        x, w, b = tc.conv_int_case(launcher, shape, seed)
        return (x, w, b), F.conv2d(x.double(), w.double(), b.double(), padding=w.shape[-1] // 2)
    return _cached((launcher, shape, seed), make)


def _act64(ref, act):
    return torch.relu(ref) if act == 1 else (torch.tanh(ref) if act == 2 else ref)


# ---- one input channel ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('k', [3, 5])
def test_cin1_equals_conv2d_in_float64(k, act):
    """conv_cin1<k, act> at Co = 1, 5 (one channel group), 16, 64 (four exact groups) and 17, 21 (cg = 5 and 6: the last group
    short), on one, 9 and 65 quads per row."""
    L = _native.lib()
    for shape in tc.CIN1_SHAPES:
        N, Co, H, W = shape
        (x, w, b), ref = _conv_case('cin1', shape + (k,))
        band = _band(k, W)
        fx, fw, fb, fy = _in(x, band), _in(w, band), _in(b, band), _out((N, Co, H, W), band)
        _native.check(L.tai_conv_cin1_forward(fx.ptr(), fw.ptr(), fb.ptr(), fy.ptr(), N, Co, H, W, k, act, _s()), 'cin1')
        _assert_equal(fy.t.double().cpu(), _act64(ref, act), 'conv_cin1 %s k=%d act=%d' % (tc.shape_id(shape), k, act))
        fy.bands_untouched('y')
        assert torch.equal(fx.t.cpu(), x)


@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('k', [3, 5])
def test_cin1_pool_equals_conv2d_and_max_pool_in_float64(k, act):
    """conv_cin1_pool<k, act>: the full-resolution output and the pooled one, plain (tai_conv_cin1_forward_maxpool) and as a
    window of a larger plane at even and odd origins and odd plane widths (the 8-byte pair store and its two 4-byte halves);
    everything of the plane outside the window keeps its sentinel."""
    L = _native.lib()
    for shape in tc.CIN1_SHAPES:
        N, Co, H, W = shape
        (x, w, b), ref = _conv_case('cin1_pool', shape + (k,))
        want = _act64(ref, act)
        want_pool = F.max_pool2d(want, 2)
        band = _band(k, W)
        fx, fw, fb = _in(x, band), _in(w, band), _in(b, band)
        for window in tc.POOL_WINDOWS:
            what = 'conv_cin1_pool %s k=%d act=%d window=%r' % (tc.shape_id(shape), k, act, window)
            fy = _out((N, Co, H, W), band)
            if window is None:
                oy, ox, ph, pw = 0, 0, H // 2, W // 2
                fp = _out((N, Co, ph, pw), band)
                rc = L.tai_conv_cin1_forward_maxpool(fx.ptr(), fw.ptr(), fb.ptr(), fy.ptr(), fp.ptr(), N, Co, H, W, k, act, _s())
            else:
                oy, ox, eh, ew = window
                ph, pw = H // 2 + oy + eh, W // 2 + ox + ew
                fp = _out((N, Co, ph, pw), band)
                rc = L.tai_conv_cin1_forward_maxpool_window(fx.ptr(), fw.ptr(), fb.ptr(), fy.ptr(), fp.ptr(), N, Co, H, W, k, act,
                                                            ph, pw, oy, ox, _s())
            _native.check(rc, what)
            _assert_equal(fy.t.double().cpu(), want, what + ': y')
            plane = fp.t.double().cpu()
            _assert_equal(plane[:, :, oy:oy + H // 2, ox:ox + W // 2], want_pool, what + ': pooled')
            outside = torch.ones(plane.shape, dtype=torch.bool)
            outside[:, :, oy:oy + H // 2, ox:ox + W // 2] = False
            assert bool((plane[outside] == SENTINEL).all()), what + ': written outside the window'
            fy.bands_untouched('y')
            fp.bands_untouched('ypool')


# ---- one output channel --------------------------------------------------------------------------------------------------

def _cout1(L, launcher, fx, fw, fb, fy, shape, act):
    N, Ci, H, W = shape
    if launcher == 'cout1_3x3':
        return L.tai_conv_cout1_3x3_forward(fx.ptr(), fw.ptr(), fb.ptr(), fy.ptr(), N, Ci, H, W, act, _s())
    return L.tai_conv_cout1_5x5_forward(fx.ptr(), fw.ptr(), fb.ptr() if fb is not None else None, fy.ptr(), N, Ci, H, W, _s())


@pytest.mark.parametrize('act', [0, 1])
def test_cout1_3x3_equals_conv2d_in_float64(act):
    """conv_cout1_3x3<act>: Ci around the channel loop's unroll of 4, H = 1, 2 (clamped rows meet zero weights), W = 4 and 8
    (no neighbour lane in the row / one), 36 and 260 (quads that do not divide 64: lanes 0 and 63 load their own edge column,
    every other lane takes it from its neighbour), 256 (a row is four waves)."""
    L = _native.lib()
    for shape in tc.COUT1_SHAPES:
        N, Ci, H, W = shape
        (x, w, b), ref = _conv_case('cout1_3x3', shape)
        band = _band(3, W)
        fx, fw, fb, fy = _in(x, band), _in(w, band), _in(b, band), _out((N, 1, H, W), band)
        _native.check(_cout1(L, 'cout1_3x3', fx, fw, fb, fy, shape, act), 'cout1_3x3')
        _assert_equal(fy.t.double().cpu(), _act64(ref, act), 'conv_cout1_3x3 %s act=%d' % (tc.shape_id(shape), act))
        fy.bands_untouched('y')


def test_cout1_3x3_tanh_within_the_projects_bound():
    """conv_cout1_3x3<2> on test_gpu_thin_conv.py's data, at its bound: 2e-6 of 1 + the sum of the absolute terms."""
    L = _native.lib()
    for shape in tc.COUT1_SHAPES:
        N, Ci, H, W = shape
        x, w, b = tc.conv_float_case(shape, 13)
        band = _band(3, W)
        fx, fw, fb, fy = _in(x, band), _in(w, band), _in(b, band), _out((N, 1, H, W), band)
        _native.check(_cout1(L, 'cout1_3x3', fx, fw, fb, fy, shape, 2), 'cout1_3x3 tanh')
        ref = torch.tanh(F.conv2d(x.double(), w.double(), b.double(), padding=1))
        mag = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=1)
        _assert_close(fy.t.cpu(), ref, FWD_TOL, 'conv_cout1_3x3 tanh %s' % tc.shape_id(shape), mag)
        fy.bands_untouched('y')


@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'no-bias'])
def test_cout1_5x5_equals_conv2d_in_float64(bias):
    """conv_cout1_5x5 with and without its bias: W = 4 (no flank), 8 (one flank per quad), wider rows (both), H = 1, 2 (rows
    outside the image at either end)."""
    L = _native.lib()
    for shape in tc.COUT1_SHAPES:
        N, Ci, H, W = shape
        (x, w, b), ref = _conv_case('cout1_5x5', shape)
        band = _band(5, W)
        fx, fw, fy = _in(x, band), _in(w, band), _out((N, 1, H, W), band)
        fb = _in(b, band) if bias else None
        _native.check(_cout1(L, 'cout1_5x5', fx, fw, fb, fy, shape, 0), 'cout1_5x5')
        want = ref if bias else ref - b.double().view(1, 1, 1, 1)
        _assert_equal(fy.t.double().cpu(), want, 'conv_cout1_5x5 %s bias=%r' % (tc.shape_id(shape), bias))
        fy.bands_untouched('y')


# ---- the weight / bias gradient of the thin layers -------------------------------------------------------------------------

def _wrw_case(shape, k, seed=17):
    """(big, thin on the host; dw [Cb, k, k], db [Cb] by fp64 autograd in both roles of the two tensors)."""
    def make():
        big, thin = tc.wrw_int_case(shape, seed)
        N, Cb, H, W = shape
        # one input channel: thin = x, big = dL/dy
        w = torch.zeros(Cb, 1, k, k, dtype=torch.float64, requires_grad=True)
        bias = torch.zeros(Cb, dtype=torch.float64, requires_grad=True)
        dw_in, db_in = torch.autograd.grad(F.conv2d(thin.double(), w, bias, padding=k // 2), (w, bias), big.double())
        # one output channel: big = x, thin = dL/dy, the taps come out flipped
        w1 = torch.zeros(1, Cb, k, k, dtype=torch.float64, requires_grad=True)
        dw_out, = torch.autograd.grad(F.conv2d(big.double(), w1, None, padding=k // 2), (w1,), thin.double())
        return (big, thin), (dw_in[:, 0].contiguous(), db_in), dw_out[0].flip(-1, -2).contiguous()
    return _cached(('wrw', shape, k, seed), make)


@pytest.mark.parametrize('k', [3, 5])
@pytest.mark.parametrize('shape', tc.WRW_SHAPES, ids=tc.shape_id)
def test_thin_wrw_equals_float64_autograd(shape, k):
    """thin_wrw<k> + thin_wrw_reduce where a lane walks several rows (the window slides: rs = 2, 3), where two segments meet
    and re-read each other's rows, with a short last segment, with more segments than rows, with two items for one lane
    (W = 1028) and with fewer items than lanes; weight and bias gradient together and each alone; in both roles of the operands."""
    L = _native.lib()
    N, Cb, H, W = shape
    (big, thin), (dw_in, db_in), dw_out = _wrw_case(shape, k)
    assert torch.equal(dw_in, dw_out)
    band = _band(k, W)
    fbig, fthin = _in(big, band), _in(thin, band)
    for outputs in tc.WRW_OUTPUTS:
        what = 'thin_wrw %s k=%d %s' % (tc.shape_id(shape), k, outputs)
        fdw = _out((Cb, k, k), band) if outputs != 'db' else None
        fdb = _out((Cb,), band) if outputs != 'dw' else None
        fws = _out((N * Cb * 32,), band)
        _native.check(L.tai_thin_conv_wrw(fbig.ptr(), fthin.ptr(), fdw.ptr() if fdw else None, fdb.ptr() if fdb else None, fws.ptr(),
                                          N, Cb, H, W, k, _s()), what)
        if fdw:
            _assert_equal(fdw.t.double().cpu(), dw_in, what + ': dw')
            fdw.bands_untouched('dw')
        if fdb:
            _assert_equal(fdb.t.double().cpu(), db_in, what + ': db')
            fdb.bands_untouched('db')
        fws.bands_untouched('workspace')
        ws = fws.t.view(N * Cb, 32).cpu()
        assert bool((ws[:, k * k + 1:] == SENTINEL).all()), what + ': workspace written past its K * K + 1 partial sums'


# ---- bias + activation in place ----------------------------------------------------------------------------------------------

def _bias_act_ref(x, bias, act):
    v = x + bias.view(1, -1, 1)
    return torch.relu(v) if act == 1 else v


@pytest.mark.parametrize('act', [0, 1, 2])
@pytest.mark.parametrize('shape', tc.BIAS_ACT_SHAPES, ids=tc.shape_id)
def test_bias_act_inplace(shape, act):
    """tai_bias_act_inplace on its 16-byte route (HW % 4 == 0), on its scalar route (HW % 4 != 0) and, where HW % 4 == 0, on a
    view one float past a 16-byte boundary: the scalar kernel again, whose result must be the aligned route's."""
    L = _native.lib()
    N, C, HW = shape
    g = torch.Generator().manual_seed(HW + act)
    x, bias = torch.randn(N, C, HW, generator=g), torch.randn(C, generator=g)
    fb = _in(bias, _band())
    fx = _out(shape, _band(), x)
    _native.check(L.tai_bias_act_inplace(fx.ptr(), fb.ptr(), N, C, HW, act, _s()), 'bias_act')
    if act == 2:
        _assert_close(fx.t.cpu(), torch.tanh(x.double() + bias.double().view(1, -1, 1)), FWD_TOL, 'bias_act tanh')
    else:
        _assert_equal(fx.t.cpu(), _bias_act_ref(x, bias, act), 'bias_act act=%d' % act)
    fx.bands_untouched('x')
    if HW % 4 == 0:
        off = _Framed(x, _band(), SENTINEL, offset=1)
        assert off.ptr() % 16 == 4
        _native.check(L.tai_bias_act_inplace(off.ptr(), fb.ptr(), N, C, HW, act, _s()), 'bias_act, offset pointer')
        _assert_equal(off.t, fx.t, 'bias_act act=%d on a pointer one float past a 16-byte boundary' % act)
        off.bands_untouched('x (offset)')


# ---- unpool + add, activation + pool, shift stack --------------------------------------------------------------------------

def _unpool_ref(x, res):
    want = res.clone()
    want[:, 0::2, 0::2] += x
    return want


@pytest.mark.parametrize('shape', tc.UNPOOL_SHAPES, ids=tc.shape_id)
def test_unpool2x_add(shape):
    L = _native.lib()
    planes, h, w = shape
    g = torch.Generator().manual_seed(h)
    x, res = torch.randn(planes, h, w, generator=g), torch.randn(planes, 2 * h, 2 * w, generator=g)
    fx, fres, fo = _in(x, _band()), _in(res, _band()), _out(res.shape, _band())
    _native.check(L.tai_unpool2x_add(fx.ptr(), fres.ptr(), fo.ptr(), planes, h, w, _s()), 'unpool2x_add')
    _assert_equal(fo.t.cpu(), _unpool_ref(x, res), 'unpool2x_add %s' % tc.shape_id(shape))
    fo.bands_untouched('out')


def _act_pool_fwd_ref(z, relu):
    y = torch.relu(z) if relu else z
    return y, F.max_pool2d(y.unsqueeze(0), 2)[0]


def _act_pool_run(L, z, gy, gyp, relu, shape, what):
    """Forward and backward through the C ABI inside guard bands -> (y, yp, gz) on the device."""
    planes, H, W = shape
    band = _band(2, W)
    fz, fy, fp = _in(z, band), _out(shape, band), _out((planes, H // 2, W // 2), band)
    _native.check(L.tai_act_maxpool2x2_forward(fz.ptr(), fy.ptr(), fp.ptr(), planes, H, W, relu, _s()), what)
    fy.bands_untouched('y')
    fp.bands_untouched('ypool')
    fgy = _in(gy, band) if gy is not None else None
    fgp = _in(gyp, band) if gyp is not None else None
    fyin, fgz = _in(fy.t, band), _out(shape, band)
    _native.check(L.tai_act_maxpool2x2_backward(fgy.ptr() if fgy else None, fgp.ptr() if fgp else None, fyin.ptr(), fgz.ptr(), planes,
                                                H, W, relu, _s()), what + ' backward')
    fgz.bands_untouched('grad_z')
    return fy.t, fp.t, fgz.t


@pytest.mark.parametrize('paths', ['both', 'pooled_only', 'full_only'])
@pytest.mark.parametrize('relu', [1, 0], ids=['relu', 'linear'])
@pytest.mark.parametrize('shape', tc.ACT_POOL_SHAPES, ids=tc.shape_id)
def test_act_pool2x2_forward_and_backward(shape, relu, paths):
    """act_pool2x2_forward / _backward on data full of ties (multiples of 0.5 in [-1.5, 1.5]; zeros after the ReLU), W = 4,
    H = 2, grad_y NULL, grad_ypool NULL and both present.  The backward's reference is the explicit first-maximum scatter."""
    L = _native.lib()
    planes, H, W = shape
    g = torch.Generator().manual_seed(W + relu)
    z = tc.quantised(g, 0.5, -3, 3, planes, H, W)
    gy = torch.randn(planes, H, W, generator=g) if paths != 'pooled_only' else None
    gyp = torch.randn(planes, H // 2, W // 2, generator=g) if paths != 'full_only' else None
    what = 'act_pool2x2 %s relu=%d %s' % (tc.shape_id(shape), relu, paths)
    y, yp, gz = _act_pool_run(L, z, gy, gyp, relu, shape, what)
    want_y, want_p = _act_pool_fwd_ref(z, relu)
    _assert_equal(y.cpu(), want_y, what + ': y')
    _assert_equal(yp.cpu(), want_p, what + ': ypool')
    win = want_y.view(planes, H // 2, 2, W // 2, 2)
    if yp.numel() >= 64:
        assert int((win.amax(dim=(2, 4), keepdim=True) == win).sum()) > yp.numel()     # there are ties
    _assert_equal(gz.cpu(), tc.act_pool_backward_ref(want_y, gy, gyp, relu), what + ': grad_z')


@pytest.mark.parametrize('shape', tc.SHIFT_STACK_SHAPES, ids=tc.shape_id)
def test_shift_stack(shape):
    L = _native.lib()
    N, C, H, W, k = shape
    S = {5: 2, 7: 3}[k]
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(k + W)) + 3.0      # no zeros: the halo's are the only ones
    fx, fo = _in(x, _band(k, W)), _out((N, S * S * C, H + 2, W + 4), _band(k, W))
    _native.check(L.tai_conv_shift_stack(fx.ptr(), fo.ptr(), N, C, H, W, k, _s()), 'shift_stack')
    _assert_equal(fo.t.cpu(), tc.shift_stack_ref(x, k), 'shift_stack %s' % tc.shape_id(shape))
    fo.bands_untouched('out')


# ---- the discriminator's window-scaled tails --------------------------------------------------------------------------------

def _window_data(shape, seed, device='cpu'):
    """z, gy [nw * B, C, HW], bias [C], inv_scale [nw].  z, bias and the factors are short binary fractions: z * s + b is exact,
    whether the compiler fuses it or not; the slope's product is one rounding either way."""
    nw, B, C, HW = shape
    g = torch.Generator(device=device).manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, device=device).float()
    z = ri(-32, 32, nw * B, C, HW) * 0.25
    bias = ri(-16, 16, C) * 0.125
    inv = ri(2, 7, nw) * 0.25
    gy = torch.randn(nw * B, C, HW, generator=g, device=device)
    return z, bias, inv, gy


def _window_ref(z, bias, inv, gy, shape, slope):
    nw, B, C, HW = shape
    s = inv.repeat_interleave(B).view(-1, 1, 1)
    v = z * s + bias.view(1, -1, 1)
    y = torch.where(v > 0, v, v * slope)
    gz = torch.where(y > 0, gy, gy * slope)
    return y, gz, gz * s


def _window_run(L, scalar, z, bias, inv, gy, shape, slope):
    nw, B, C, HW = shape
    fwd = L.tai_window_scale_bias_lrelu_scalar if scalar else L.tai_window_scale_bias_lrelu
    bwd = L.tai_window_scale_lrelu_backward_scalar if scalar else L.tai_window_scale_lrelu_backward
    fy, fb, fi = _out(z.shape, _band(), z), _in(bias, _band()), _in(inv, _band())
    _native.check(fwd(fy.ptr(), fb.ptr(), fi.ptr(), nw, B, C, HW, slope, _s()), 'window_scale forward')
    fy.bands_untouched('y')
    fg, fyin, fgz, fgs = _in(gy, _band()), _in(fy.t, _band()), _out(z.shape, _band()), _out(z.shape, _band())
    _native.check(bwd(fg.ptr(), fyin.ptr(), fi.ptr(), fgz.ptr(), fgs.ptr(), nw, B, C, HW, slope, _s()), 'window_scale backward')
    fgz.bands_untouched('grad_z')
    fgs.bands_untouched('grad_scaled')
    return fy.t, fgz.t, fgs.t


@pytest.mark.parametrize('shape', tc.WINDOW_SCALE_SHAPES, ids=tc.shape_id)
def test_window_scale_tails(shape):
    """The four window_scale_* kernels: the scalar forms on any plane, the 16-byte forms where HW % 4 == 0."""
    L = _native.lib()
    slope = 0.2
    z, bias, inv, gy = _window_data(shape, 3)
    want = _window_ref(z, bias, inv, gy, shape, slope)
    for scalar in (True, False) if shape[3] % 4 == 0 else (True,):
        got = _window_run(L, scalar, z, bias, inv, gy, shape, slope)
        for name, a, b in zip(('y', 'grad_z', 'grad_scaled'), got, want):
            _assert_equal(a.cpu(), b, 'window_scale%s %s: %s' % ('_scalar' if scalar else '', tc.shape_id(shape), name))


# ---- the ConvLSTM gates ----------------------------------------------------------------------------------------------------

def _gates_expr(gates, c, forget_bias):
    i, j, f, o = torch.chunk(gates, 4, dim=1)
    new_c = c * torch.sigmoid(f + forget_bias) + torch.sigmoid(i) * torch.tanh(j)
    return new_c, torch.tanh(new_c) * torch.sigmoid(o)


def _gates_grads(gates, c, forget_bias, gc, gh, dtype):
    gd, cd = gates.detach().to(dtype).requires_grad_(True), c.detach().to(dtype).requires_grad_(True)
    nc, nh = _gates_expr(gd, cd, forget_bias)
    loss = ((nc * gc.to(dtype)).sum() if gc is not None else 0) + ((nh * gh.to(dtype)).sum() if gh is not None else 0)
    dg, dc = torch.autograd.grad(loss, (gd, cd))
    return nc.detach(), nh.detach(), dg, dc


def _gates_run(L, gates, c, forget_bias, gc, gh):
    """Forward and backward through the C ABI inside guard bands -> (new_c, new_h, d_gates, d_c) on the device."""
    N, F4, HW = gates.shape
    Fe = F4 // 4
    fg, fc = _in(gates, _band()), _in(c, _band())
    fnc, fnh = _out(c.shape, _band()), _out(c.shape, _band())
    _native.check(L.tai_convlstm_gates_forward(fg.ptr(), fc.ptr(), fnc.ptr(), fnh.ptr(), N, Fe, HW, forget_bias, _s()), 'gates')
    fnc.bands_untouched('new_c')
    fnh.bands_untouched('new_h')
    fgc = _in(gc, _band()) if gc is not None else None
    fgh = _in(gh, _band()) if gh is not None else None
    fncin, fdg, fdc = _in(fnc.t, _band()), _out(gates.shape, _band()), _out(c.shape, _band())
    _native.check(L.tai_convlstm_gates_backward(fg.ptr(), fc.ptr(), fncin.ptr(), fgc.ptr() if fgc else None, fgh.ptr() if fgh else None,
                                                fdg.ptr(), fdc.ptr(), N, Fe, HW, forget_bias, _s()), 'gates backward')
    fdg.bands_untouched('grad_gates')
    fdc.bands_untouched('grad_c')
    return fnc.t, fnh.t, fdg.t, fdc.t


def _gates_data(N, Fe, HW, seed, scale=1.0, device='cpu'):
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    return rn(N, 4 * Fe, HW) * scale, rn(N, Fe, HW), rn(N, Fe, HW), rn(N, Fe, HW)


@pytest.mark.parametrize('forget_bias', tc.GATE_FORGET_BIAS)
@pytest.mark.parametrize('HW', tc.GATE_HW)
def test_convlstm_gates_forward_and_backward(HW, forget_bias):
    """convlstm_gates / _backward at HW = 4 (one item per plane), 60, 256, F = 1 and 16, three forget biases, gradients from new_h
    only, new_c only and both, against fp64 autograd of the reference's expression: 2e-6 forward, 5e-6 backward."""
    L = _native.lib()
    for Fe in tc.GATE_F:
        gates, c, gc, gh = _gates_data(tc.GATE_N, Fe, HW, HW + Fe)
        for paths in tc.GATE_PATHS:
            use_c, use_h = (gc if paths != 'h_only' else None), (gh if paths != 'c_only' else None)
            got = _gates_run(L, gates, c, forget_bias, use_c, use_h)
            want = _gates_grads(gates, c, forget_bias, use_c, use_h, torch.float64)
            what = 'convlstm_gates F=%d HW=%d fb=%g %s: ' % (Fe, HW, forget_bias, paths)
            for name, a, b, tol in zip(('new_c', 'new_h', 'grad_gates', 'grad_c'), got, want, (FWD_TOL, FWD_TOL, BWD_TOL, BWD_TOL)):
                _assert_close(a.cpu(), b, tol, what + name)


def test_convlstm_gates_saturated():
    """Gates scaled by 8: most sigmoids and tanhs sit in their tails.  No bound is known for that, so the bound is measured:
    the error of ATen's own fp32 evaluation of the same expression (and of its autograd) against fp64 on the same inputs, on
    the device; the kernels may be twice as far from fp64, and never need to be closer than the bounds of the test above.
    Measured on an MI355X (N, F, HW = 3, 16, 256; forget bias 1): ATen fp32 forward 3.44e-7, backward 6.58e-7; the
    kernels: forward 3.52e-7, backward 5.87e-7.  Twice ATen's error is below the floors, so the floors (2e-6, 5e-6) decide."""
    L = _native.lib()
    gates, c, gc, gh = _gates_data(3, 16, 256, 99, scale=8.0)
    assert float((gates.abs() > 8).float().mean()) > 0.25
    dev = [t.to(DEV) for t in (gates, c, gc, gh)]
    ref = _gates_grads(*dev[:2], 1.0, *dev[2:], torch.float64)
    aten = _gates_grads(*dev[:2], 1.0, *dev[2:], torch.float32)
    got = _gates_run(L, gates, c, 1.0, gc, gh)
    err = lambda xs: [float((a.double() - b).abs().max()) for a, b in zip(xs, ref)]
    e_aten, e_got = err(aten), err(got)
    print('saturated gates: ATen fp32 forward %.3g backward %.3g; kernels forward %.3g backward %.3g'
          % (max(e_aten[:2]), max(e_aten[2:]), max(e_got[:2]), max(e_got[2:])))
    assert max(e_got[:2]) <= max(FWD_TOL, 2 * max(e_aten[:2])), (e_got, e_aten)
    assert max(e_got[2:]) <= max(BWD_TOL, 2 * max(e_aten[2:])), (e_got, e_aten)


# ---- a second pass of every grid-stride loop ---------------------------------------------------------------------------------

@pytest.mark.parametrize('launcher', ['cin1', 'cin1_pool', 'cout1_3x3', 'cout1_5x5'])
def test_strided_convolutions(launcher):
    """N * H * W / 4 a few thousand items past 8,192 blocks of 256: the loop's second pass, against the fp64 convolution on the
    device (a sum of shifted copies), with outliers on the last item of the first pass and the first of the second."""
    L = _native.lib()
    shape = tc.STRIDED[launcher]
    N, C, H, W = shape[:4]
    x, w, b = tc.conv_int_case(launcher, shape, 23)
    k = w.shape[-1]
    band = _band(k, W)
    fx, fw, fb = _in(x, band), _in(w, band), _in(b, band)
    Co = w.shape[0]
    fy = _out((N, Co, H, W), band)
    if launcher == 'cin1':
        act = 0
        rc = L.tai_conv_cin1_forward(fx.ptr(), fw.ptr(), fb.ptr(), fy.ptr(), N, Co, H, W, k, act, _s())
    elif launcher == 'cin1_pool':
        act = 1
        fp = _out((N, Co, H // 2, W // 2), band)
        rc = L.tai_conv_cin1_forward_maxpool(fx.ptr(), fw.ptr(), fb.ptr(), fy.ptr(), fp.ptr(), N, Co, H, W, k, act, _s())
    else:
        act = 0
        rc = _cout1(L, launcher, fx, fw, fb, fy, shape, act)
    _native.check(rc, launcher)
    want = _act64(tc.conv_shifts64(fx.t, fw.t.cpu(), fb.t), act)
    got = fy.t.double()
    _second_pass(launcher, shape, got, want, launcher)
    _assert_equal(got, want, '%s %s' % (launcher, tc.shape_id(shape)))
    fy.bands_untouched('y')
    if launcher == 'cin1_pool':
        _assert_equal(fp.t.double(), F.max_pool2d(want, 2), 'cin1_pool %s: pooled' % tc.shape_id(shape))
        fp.bands_untouched('ypool')


@pytest.mark.parametrize('launcher', ['bias_act_vec4', 'bias_act_scalar'])
@pytest.mark.parametrize('act', [1, 2])
def test_strided_bias_act(launcher, act):
    L = _native.lib()
    shape = tc.STRIDED[launcher]
    N, C, HW = shape
    g = torch.Generator(device=DEV).manual_seed(5)
    x, bias = torch.randn(N, C, HW, generator=g, device=DEV), torch.randn(C, generator=g, device=DEV)
    fb, fx = _in(bias, _band()), _out(shape, _band(), x)
    _native.check(L.tai_bias_act_inplace(fx.ptr(), fb.ptr(), N, C, HW, act, _s()), launcher)
    if act == 2:
        want = torch.tanh(x.double() + bias.double().view(1, -1, 1))
        _second_pass(launcher, shape, fx.t, want, launcher, FWD_TOL)
        _assert_close(fx.t, want, FWD_TOL, launcher + ' tanh')
    else:
        want = _bias_act_ref(x, bias, act)
        _second_pass(launcher, shape, fx.t, want, launcher)
        _assert_equal(fx.t, want, launcher)
    fx.bands_untouched('x')


def test_strided_unpool2x_add():
    L = _native.lib()
    shape = tc.STRIDED['unpool']
    planes, h, w = shape
    g = torch.Generator(device=DEV).manual_seed(6)
    x, res = torch.randn(planes, h, w, generator=g, device=DEV), torch.randn(planes, 2 * h, 2 * w, generator=g, device=DEV)
    fx, fres, fo = _in(x, _band()), _in(res, _band()), _out(res.shape, _band())
    _native.check(L.tai_unpool2x_add(fx.ptr(), fres.ptr(), fo.ptr(), planes, h, w, _s()), 'unpool2x_add')
    want = _unpool_ref(x, res)
    _second_pass('unpool', shape, fo.t, want, 'unpool2x_add')
    _assert_equal(fo.t, want, 'unpool2x_add')
    fo.bands_untouched('out')


@pytest.mark.parametrize('relu', [1, 0], ids=['relu', 'linear'])
def test_strided_act_pool2x2(relu):
    """planes * (H / 2) * (W / 4) = 4,198,400 against the 4,194,304 one pass covers (a [32, 64, 128, 128] layer is exactly the
    cap; any larger batch strides), forward and backward."""
    L = _native.lib()
    shape = tc.STRIDED['act_pool']
    planes, H, W = shape
    g = torch.Generator(device=DEV).manual_seed(7)
    z = torch.randint(-3, 4, shape, generator=g, device=DEV).float() * 0.5
    gy = torch.randn(shape, generator=g, device=DEV)
    gyp = torch.randn(planes, H // 2, W // 2, generator=g, device=DEV)
    y, yp, gz = _act_pool_run(L, z, gy, gyp, relu, shape, 'act_pool2x2')
    want_y, want_p = _act_pool_fwd_ref(z, relu)
    _second_pass('act_pool', shape, y, want_y, 'act_pool2x2_forward')
    _assert_equal(y, want_y, 'act_pool2x2_forward: y')
    _assert_equal(yp, want_p, 'act_pool2x2_forward: ypool')
    want_g = tc.act_pool_backward_ref(want_y, gy, gyp, relu)
    _second_pass('act_pool', shape, gz, want_g, 'act_pool2x2_backward')
    _assert_equal(gz, want_g, 'act_pool2x2_backward')


def test_strided_shift_stack():
    L = _native.lib()
    shape = tc.STRIDED['shift_stack']
    N, C, H, W, k = shape
    x = torch.randn(N, C, H, W, generator=torch.Generator(device=DEV).manual_seed(8), device=DEV) + 3.0
    fx, fo = _in(x, _band(k, W)), _out((N, 4 * C, H + 2, W + 4), _band(k, W))
    _native.check(L.tai_conv_shift_stack(fx.ptr(), fo.ptr(), N, C, H, W, k, _s()), 'shift_stack')
    want = tc.shift_stack_ref(x, k)
    _second_pass('shift_stack', shape, fo.t, want, 'shift_stack')
    _assert_equal(fo.t, want, 'shift_stack')
    fo.bands_untouched('out')


@pytest.mark.parametrize('launcher', ['window_scale', 'window_scale_scalar'])
def test_strided_window_scale(launcher):
    """The 16-byte forms past 16,384 blocks; the scalar forms past 16,384 planes (production: 13 * 32 * 64 = 26,624)."""
    L = _native.lib()
    shape = tc.STRIDED[launcher]
    slope = 0.2
    z, bias, inv, gy = _window_data(shape, 9, device=DEV)
    got = _window_run(L, launcher == 'window_scale_scalar', z, bias, inv, gy, shape, slope)
    want = _window_ref(z, bias, inv, gy, shape, slope)
    for name, a, b in zip(('y', 'grad_z', 'grad_scaled'), got, want):
        _second_pass(launcher, shape, a, b, '%s: %s' % (launcher, name))
        _assert_equal(a, b, '%s: %s' % (launcher, name))


def test_strided_convlstm_gates():
    L = _native.lib()
    shape = tc.STRIDED['convlstm']
    N, Fe, HW = shape
    gates, c, gc, gh = _gates_data(N, Fe, HW, 10, device=DEV)
    got = _gates_run(L, gates, c, 1.0, gc, gh)
    want = _gates_grads(gates, c, 1.0, gc, gh, torch.float64)
    for name, a, b, tol in zip(('new_c', 'new_h', 'grad_gates', 'grad_c'), got, want, (FWD_TOL, FWD_TOL, BWD_TOL, BWD_TOL)):
        if name != 'grad_gates':            # (its four chunks are four planes: the items are not contiguous in it)
            _second_pass('convlstm', shape, a, b, 'convlstm_gates: ' + name, tol)
        _assert_close(a, b, tol, 'convlstm_gates: ' + name)
    del want


def test_strided_upsample_pairs():
    """upsample2x_align_corners_pairs on 192 x 192 planes: 18,432 items per plane against the 64 x 256 its x-blocks cover.  The
    blend is several fp32 operations, so the comparison is tests/test_gpu_upsample.py's: 2e-6 from ATen's fp32 kernel."""
    L = _native.lib()
    shape = tc.STRIDED['upsample_pairs']
    planes, H, W = shape
    x = torch.randn(planes, H, W, generator=torch.Generator(device=DEV).manual_seed(11), device=DEV)
    fx, fo = _in(x, _band(2, 2 * W)), _out((planes, 2 * H, 2 * W), _band(2, 2 * W))
    _native.check(L.tai_upsample_bilinear2x_forward(fx.ptr(), fo.ptr(), planes, H, W, _s()), 'upsample')
    want = F.interpolate(x.unsqueeze(0), scale_factor=2, mode='bilinear', align_corners=True)[0]
    _second_pass('upsample_pairs', shape, fo.t, want, 'upsample pairs', UPS_TOL)
    _assert_close(fo.t, want, UPS_TOL, 'upsample pairs')
    fo.bands_untouched('out')
