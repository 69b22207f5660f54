"""sn_discriminator._WindowScaledConvLReLU alone on the magnitude-scaled bound of tests/kink_sides.py: the output of one layer call
against the float64 layer per element (check_layer: values within TOL43 of 1 + the tile's magnitude sum, kink sides legitimate, the
ambiguous set tiny), then -- sound once the sides are legitimate -- the three gradients against float64 autograd on the product's sides.
Shapes (kink_sides.LAYER_SHAPES): the smallest that take each branch -- 3 input channels, an odd space-to-depth plane, a 10 x 13 output on
the scalar tail, 13 windows whose factors differ by 1e-4 between neighbours.  Each on the in-tree route (3x3 Winograd layer over
space-to-depth planes) and on the stock route (ATen's convolution, then the same tail kernels)."""
import pytest
import torch
import torch.nn.functional as F

import kink_sides as ks  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GRAD_TOL = 2e-5            # gradients: max |got - ref| <= GRAD_TOL * max |ref| (the bound of the layer's tests in tests/test_gpu_training.py)


@pytest.fixture(autouse=True)
def _fp32_convs():
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False


@pytest.mark.parametrize('route', ['in-tree', 'stock'])
@pytest.mark.parametrize('shape', ks.LAYER_SHAPES)
def test_discriminator_layer_alone_passes_the_layer_check_and_its_gradients_follow(shape, route, monkeypatch):
    """A second run reproduces every bit on the in-tree route; on the stock route the output only (ATen's backward kernels sum with
    atomics: their bits are not this project's to promise)."""
    from conftest import miopen_convolutions
    from video_frame_inpainting_amd import conv_ops, sn_discriminator as snd
    nw, B, C, K, H, W = shape
    x, w, b, inv, gy = ks.layer_case(shape)
    monkeypatch.setattr(conv_ops, 'WINO_MIN_WORKGROUPS', 1)
    monkeypatch.setattr(conv_ops, 'WINO43_MIN_WORKGROUPS', 1)
    assert snd._s2d_applies(x.to(DEV), w.to(DEV), (2, 2), (1, 1))
    if route == 'stock':
        monkeypatch.setattr(snd, '_s2d_applies', lambda *a: False)
    spy = ks.DiscriminatorSpy(monkeypatch)

    def run():
        xr, wr, br = (t.to(DEV).requires_grad_() for t in (x, w, b))
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU], record_shapes=True) as prof:
            y = snd._WindowScaledConvLReLU.apply(xr, wr, wr.detach(), br, inv.to(DEV), nw, (2, 2), (1, 1), 0.2)
            y.backward(gy.to(DEV))
        return [t.cpu() for t in (y.detach(), xr.grad, wr.grad, br.grad)], miopen_convolutions(prof)

    got, convs = run()
    assert bool(convs) == (route == 'stock'), convs[:4]
    again, _ = run()
    for name, a, c in list(zip(('y', 'gx', 'gw', 'gb'), got, again))[:4 if route == 'in-tree' else 1]:
        assert torch.equal(a, c), name

    rec = spy.calls[0]
    assert rec.windows == list(range(nw)) and torch.equal(rec.y, got[0]) and torch.equal(rec.x, x) and torch.equal(rec.inv_scale, inv)
    res = ks.check_layer(rec)
    print('%s %s: %s' % (shape, route, ks.format_layer(res)))

    # float64 autograd on the product's sides (legitimate by (i) and (ii))
    xd, bd = x.double().requires_grad_(), b.double().requires_grad_()
    z = F.conv2d(xd, w.double(), None, 2, 1)
    z = (z.view(nw, B, -1) * inv.double().view(nw, 1, 1)).view_as(z) + bd.view(1, -1, 1, 1)
    side = (got[0] > 0).double()
    slope = side + 0.2 * (1 - side)
    (z * slope).backward(gy.double())
    # the weight gradient takes the pre-activation gradient WITHOUT the window's factor (_WindowScaledConv's docstring)
    wu = w.double().requires_grad_()
    F.conv2d(x.double(), wu, None, 2, 1).backward(gy.double() * slope)
    for name, a, r in zip(('gx', 'gw', 'gb'), got[1:], (xd.grad, wu.grad, bd.grad)):
        scale = float(r.abs().max())
        err = float((a.double() - r).abs().max()) / scale
        print('%s %s %s: %.2e of the maximum' % (shape, route, name, err))
        assert scale > 0 and err <= GRAD_TOL, (name, err)
