"""The discriminator's layer calls, recorded and judged one by one: what tests/test_gpu_training.py and tests/test_gpu_published_shapes.py
need before they hand the product's LeakyReLU sides to the CPU oracle (train_oracle.DiscriminatorState.forward, ``masks``).

The whole-step tests differentiate the oracle on the side of the kink the PRODUCT put every pre-activation on; the oracle then takes both
its forward and its gradient on those sides, so a wrong value or sign in sn_discriminator._WindowScaledConvLReLU (the space-to-depth
Winograd route, the per-window factor, the bias, the scalar tail for HW % 4 != 0, the seam between windows stacked along the batch) would be
imported into the reference and certified by the discriminator's tight gradient bound.  So every layer call is first held, LAYER-LOCALLY,
to a float64 evaluation of that layer on the product's own input, weight, bias and window factors:

    z = conv2d(x, w0) * inv_scale[window] + bias,   y = leaky_relu(z),   mag = conv2d(|x|, |w0|) * |inv_scale[window]| + |bias|,
    B = TOL43 * (1 + tile_mag(mag))

with the yardstick of the Winograd pins (wino_cases.TOL43, tile_mag: an outlier anywhere in a 4 x 4 output tile rounds into the whole
tile).  (A bound propagated from the clip through four layers is useless: conv(E, |w|) grows 10-50 x per layer and exceeds max |y| at the
third.)  ``check_layer`` asserts (i) every output within B of y, (ii) every sign that differs from z's at an element with |z| <= B -- the
only elements where either side is a legitimate fp32 answer -- and (iii) that those elements are at most 1e-3 of the layer call, so that
(ii) is no blank cheque.  tests/test_kink_sides_cpu.py judges the check itself without a GPU."""
import collections

import torch
import torch.nn.functional as F

from oracle import train_oracle

import wino_cases as wc  # noqa: E402

AMBIGUOUS_SHARE = 1e-3      # (iii): a condition, not a measurement (the float64 layers alone: <= 5.1e-4 at the geometries of the tests)

# One call of _WindowScaledConvLReLU.apply on the CPU: the arguments as sn_discriminator passes them (w0: the weight the convolution ran
# with; inv_scale: all nw factors) and the output; x and y hold the images of ``windows`` only, in that order, B = len(x) / len(windows)
LayerCall = collections.namedtuple('LayerCall', 'x w0 bias inv_scale nw stride padding slope y windows')


def ends_and_middle(nw):
    """The first, the middle and the last window: the images at both ends of the batch-stacked planes and one inside."""
    return sorted({0, nw // 2, nw - 1})


class DiscriminatorSpy(object):
    """Wraps sn_discriminator._WindowScaledConvLReLU.apply and keeps every call: ``layers`` -- which side of LeakyReLU's kink each output
    fell on (the sign of the layer's output: LeakyReLU keeps it), every window; ``calls`` -- a LayerCall with the images of the windows
    that ``keep`` selects (None: all; a list of window indices; or a function of nw such as ``ends_and_middle``)."""

    def __init__(self, monkeypatch, keep=None):
        from video_frame_inpainting_amd import sn_discriminator as snd
        self.layers, self.calls = [], []
        orig = snd._WindowScaledConvLReLU.apply

        def spy(*args):
            y = orig(*args)
            x, _, w0, bias, inv_scale, nw, stride, padding, slope = args
            self.layers.append((y.detach() > 0).cpu())
            windows = list(range(nw)) if keep is None else list(keep(nw) if callable(keep) else keep)
            B = x.shape[0] // nw
            rows = torch.tensor([t * B + b for t in windows for b in range(B)], device=x.device)
            host = lambda t: t.detach().cpu().clone()
            self.calls.append(LayerCall(host(x.detach().index_select(0, rows)), host(w0), host(bias), host(inv_scale), int(nw),
                                        tuple(stride), tuple(padding), float(slope), host(y.detach().index_select(0, rows)), windows))
            return y
        monkeypatch.setattr(snd._WindowScaledConvLReLU, 'apply', staticmethod(spy))

    def masks_of_call(self, call, B):
        """{(window, layer key): bool [B, Co, H, W]} of the ``call``-th discriminator evaluation (4 layers each, windows along the batch)."""
        out = {}
        for li, key in enumerate(train_oracle.SN_CONV_KEYS):
            m = self.layers[4 * call + li]
            for t0 in range(m.shape[0] // B):
                out[(t0, key)] = m[t0 * B:(t0 + 1) * B]
        return out


# The layer alone (tests/test_gpu_kink_sides.py), as (nw, B, C, K, H, W): the smallest shapes that still take each branch
LAYER_SHAPES = ((3, 2, 3, 8, 8, 8),         # first layer, 3 input channels
                (3, 2, 24, 40, 6, 10),      # odd space-to-depth plane (3 x 5)
                (2, 2, 8, 16, 20, 26),      # 10 x 13 output: the scalar tail (HW % 4 != 0)
                (13, 2, 8, 16, 8, 8))       # 13 windows: the window index of every image


def layer_case(shape):
    """Seeded operands of one layer call (x, w, bias, inv_scale, gy) on the CPU: x N(0, 1), w N(0, 2 / (16 C)), bias N(0, 0.01); the
    factors of 13 windows differ by 1e-4 between neighbours (an image scaled with its neighbour's factor is off by 1.2e-4 of its output)."""
    nw, B, C, K, H, W = shape
    g = torch.Generator().manual_seed(C + K + H + W)
    x = torch.randn(nw * B, C, H, W, generator=g)
    w = torch.randn(K, C, 4, 4, generator=g) * (2.0 / (16 * C)) ** 0.5
    b = 0.1 * torch.randn(K, generator=g)
    inv = 0.5 + torch.rand(nw, generator=g) if nw != 13 else 0.8 + 1e-4 * torch.arange(13, dtype=torch.float32)
    gy = torch.randn(nw * B, K, H // 2, W // 2, generator=g)
    return x, w, b, inv, gy


def layer_reference(rec):
    """(z, y, mag, B) of one LayerCall in float64 on the CPU (module docstring)."""
    x, w = rec.x.double(), rec.w0.double()
    per_window = x.shape[0] // len(rec.windows)
    s = rec.inv_scale.double()[list(rec.windows)].repeat_interleave(per_window).view(-1, 1, 1, 1)
    b = rec.bias.double().view(1, -1, 1, 1)
    z = F.conv2d(x, w, None, rec.stride, rec.padding) * s + b
    mag = F.conv2d(x.abs(), w.abs(), None, rec.stride, rec.padding) * s.abs() + b.abs()
    return z, F.leaky_relu(z, rec.slope), mag, wc.TOL43 * (1 + wc.tile_mag(mag))


def check_layer(rec):
    """Asserts (i)-(iii) of the module docstring on one LayerCall; -> {'worst': the largest |got - y| / B, 'sign_diffs': outputs on the
    other side of the kink than z, 'ambiguous': elements with |z| <= B, 'numel'}."""
    z, y, _, bound = layer_reference(rec)
    got = rec.y.double()
    assert got.shape == y.shape, (got.shape, y.shape)
    ratio = (got - y).abs() / bound
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float('inf')), ratio)          # a NaN counts as infinite
    differ = (got > 0) != (z > 0)
    ambiguous = z.abs() <= bound
    res = {'worst': float(ratio.max()), 'sign_diffs': int(differ.sum()), 'ambiguous': int(ambiguous.sum()), 'numel': z.numel(),
           'of_max': float((got - y).abs().nan_to_num(float('inf')).max()) / float(y.abs().max())}        # for the record, not asserted
    at = tuple(int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape))
    assert res['worst'] <= 1.0, '(i) |got - y| = %.3g B at %s (got %.9g, float64 %.9g): %s' % (res['worst'], at, got[at], y[at], res)
    illegitimate = differ & ~ambiguous
    assert not bool(illegitimate.any()), '(ii) %d outputs on the other side of the kink than a z with |z| > B, the first at %s: %s' % (
        int(illegitimate.sum()), tuple(int(i) for i in illegitimate.nonzero()[0]), res)
    assert res['ambiguous'] <= max(AMBIGUOUS_SHARE * res['numel'], 2), '(iii) either side would pass at %d of %d elements: %s' % (
        res['ambiguous'], res['numel'], res)
    return res


def format_layer(res):
    return 'worst |got - y| / B %.3f (%.1e of max |y|)  sign differences from the float64 layer %d  ambiguous %d of %d (%.1e)' % (
        res['worst'], res['of_max'], res['sign_diffs'], res['ambiguous'], res['numel'], res['ambiguous'] / res['numel'])


class OracleSides(object):
    """The kink sides that train_oracle.discriminator_leg picks from its own rounding: ``with OracleSides() as own`` around the call;
    ``own.layers`` then holds y > 0 of every discriminator convolution in the oracle's order (evaluation, window, layer)."""

    def __init__(self):
        self.layers = []

    def __enter__(self):
        self._conv2d = conv2d = train_oracle.F.conv2d

        def spying_conv2d(x, w, b=None, **kw):
            y = conv2d(x, w, b, **kw)
            self.layers.append(y.detach() > 0)
            return y
        train_oracle.F.conv2d = spying_conv2d
        return self

    def __exit__(self, *exc):
        train_oracle.F.conv2d = self._conv2d
        return False

    def differences(self, spy, B):
        """{(evaluation of the product, layer index): imposed sides that differ from the oracle's own} for the two evaluations of the D
        half (the product's second and third: the first one, inside the G loss, imposes nothing)."""
        nw = len(self.layers) // 8
        assert len(self.layers) == 8 * nw and nw > 0, len(self.layers)
        out = {}
        for call in (1, 2):
            for li in range(4):
                imposed = spy.layers[4 * call + li]
                assert imposed.shape[0] == nw * B, (imposed.shape, nw, B)
                out[(call, li)] = sum(int((imposed[t0 * B:(t0 + 1) * B] != self.layers[((call - 1) * nw + t0) * 4 + li]).sum())
                                      for t0 in range(nw))
        return out


def check_discriminator_calls(spy):
    """check_layer on every recorded call, in call order (3 evaluations x 4 layers in a training step) -> its results."""
    return [check_layer(rec) for rec in spy.calls]


def report_lines(spy, results, differences=None):
    """One line per evaluation and layer: check_layer's numbers and ``differences`` (OracleSides.differences)."""
    lines = []
    for i, (rec, res) in enumerate(zip(spy.calls, results)):
        call, li = divmod(i, 4)
        lines.append('D evaluation %d %-13s windows %-8s %s  imposed sides that differ from the oracle\'s own %s' % (
            call, train_oracle.SN_CONV_KEYS[li], ','.join(map(str, rec.windows)) if len(rec.windows) < rec.nw else 'all %d' % rec.nw,
            format_layer(res), (differences or {}).get((call, li), '-')))
    return lines
