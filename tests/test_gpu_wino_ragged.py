"""Odd planes on the F(2x2, 3x3) kernels (csrc/wino_conv.hip.inc, EPI 3) and any row length on the weight-gradient kernel
(csrc/wino_wrw.hip.inc, WRW_RAGGED): the 15 x 20 / 10 x 13 bottoms of the kernel network at the published 240 x 320 / 160 x 208
frames, the 20-104 pixel rows of the ConvLSTM, ContentEnc / DecCnn and MotionEnc there.  Against fp64, against the even kernel on
the zero-extended plane (bit for bit), against the host-widened weight gradient (to rounding), and the refusals that stay."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ACT = {None: 0, 'relu': 1, 'tanh': 2}


def _lib():
    from video_frame_inpainting_amd import _native
    return _native, _native.lib()


def _weights(w):
    _native, L = _lib()
    K, C = w.shape[0], w.shape[1]
    U = torch.empty(L.tai_conv3x3_wino_weight_floats(K, C), device='cuda')
    _native.check(L.tai_conv3x3_wino_transform_weights(w.data_ptr(), U.data_ptr(), K, C, torch.cuda.current_stream().cuda_stream),
                  'transform')
    return U


def _forward(parts, U, b, K, act, H, W):
    """y = act(conv(cat(parts)) + b) through tai_conv3x3_wino_forward_ex (one part) / _forward_parts (tai_conv3x3_wino_forward keeps
    its even-plane contract)"""
    _native, L = _lib()
    N, Cp = parts[0].shape[0], parts[0].shape[1]
    C = Cp * len(parts)
    y = torch.full((N, K, H, W), float('nan'), device='cuda')
    s = torch.cuda.current_stream().cuda_stream
    if len(parts) == 1:
        xs = (ctypes.c_void_p * 1)(parts[0].data_ptr())
        _native.check(L.tai_conv3x3_wino_forward_ex(xs, 1, 0, U.data_ptr(), b.data_ptr(), y.data_ptr(), None, 0, 0, 0, 0, None, None,
                                                    N, C, K, H, W, H, W, 0, 0, ACT[act], s), 'forward_ex')
    else:
        ptrs = (ctypes.c_void_p * len(parts))(*[p.data_ptr() for p in parts])
        _native.check(L.tai_conv3x3_wino_forward_parts(ptrs, len(parts), U.data_ptr(), b.data_ptr(), y.data_ptr(), N, C, K, H, W,
                                                       ACT[act], s), 'forward_parts')
    return y


def _operands(N, C, K, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g).cuda()
    w = (torch.randn(K, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).cuda()
    b = torch.randn(K, generator=g).cuda()
    return x, w, b


def _fp64_error(got, x, w, b, act):
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    ref = torch.relu(ref) if act == 'relu' else (torch.tanh(ref) if act == 'tanh' else ref)
    mag = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=1)
    return ((got.double() - ref).abs() / (1 + mag)).max().item()        # the bound of tests/test_gpu_wino_conv.py: 4e-6


PLANES = [(15, 20), (10, 13), (7, 9), (3, 2), (1, 1), (31, 45)]
CHANNELS = [(256, 256), (64, 51), (3, 64)]


@pytest.fixture(params=[1, 0], ids=['tall', 'square'])
def tall(request):
    _native, L = _lib()
    prev = L.tai_conv3x3_wino_set_tall(request.param)
    yield request.param
    L.tai_conv3x3_wino_set_tall(prev)


@pytest.mark.parametrize('act', [None, 'relu', 'tanh'])
@pytest.mark.parametrize('chans,tall_on', [((256, 256), 1), ((256, 256), 0), ((64, 51), 1), ((3, 64), 1)],
                         ids=['256-256-tall', '256-256-square', '64-51', '3-64'])
@pytest.mark.parametrize('plane', PLANES, ids=lambda p: '%dx%d' % p)
def test_odd_plane_forward_matches_fp64(plane, chans, tall_on, act):
    """Plain single-tensor form; the 256 -> 256 layers take the 128 x 32 (TALL) workgroups with the set_tall switch on, the 64 x 64
    ones with it off (K < 128 always takes those)."""
    _native, L = _lib()
    prev = L.tai_conv3x3_wino_set_tall(tall_on)
    try:
        _forward_matches_fp64(plane, chans, act)
    finally:
        L.tai_conv3x3_wino_set_tall(prev)


def _forward_matches_fp64(plane, chans, act):
    (H, W), (C, K) = plane, chans
    N = 3
    x, w, b = _operands(N, C, K, H, W, H * 100 + W + C)
    got = _forward([x], _weights(w), b, K, act, H, W)
    assert torch.isfinite(got).all()
    assert _fp64_error(got, x, w, b, act) <= 4e-6


# parts of a multiple of 8 channels: 256 in 2 and 4, 64 in 2 and 4, 96 in 2, 3 and 4
@pytest.mark.parametrize('chans,nparts', [((256, 256), 2), ((256, 256), 4), ((64, 51), 2), ((64, 51), 4), ((96, 64), 2), ((96, 64), 3),
                                          ((96, 64), 4)], ids=lambda v: '%d-%d' % v if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize('plane', [(15, 20), (10, 13), (7, 9), (1, 1)], ids=lambda p: '%dx%d' % p)
def test_odd_plane_forward_of_channel_parts_matches_fp64(plane, chans, nparts, tall):
    (H, W), (C, K) = plane, chans
    assert C % nparts == 0 and (C // nparts) % 8 == 0
    N = 2
    x, w, b = _operands(N, C, K, H, W, 7 * nparts + H)
    parts = [p.contiguous() for p in x.chunk(nparts, dim=1)]
    got = _forward(parts, _weights(w), b, K, 'relu', H, W)
    assert _fp64_error(got, x, w, b, 'relu') <= 4e-6
    assert torch.equal(got, _forward([x], _weights(w), b, K, 'relu', H, W))      # the parts read where they lie: the same bits


@pytest.mark.parametrize('act', [None, 'relu', 'tanh'])
@pytest.mark.parametrize('chans', [(256, 256), (64, 51), (3, 64)], ids=lambda c: '%d-%d' % c)
@pytest.mark.parametrize('plane', PLANES, ids=lambda p: '%dx%d' % p)
def test_odd_plane_equals_the_even_kernel_on_the_zero_extended_plane(plane, chans, act, tall):
    """The edge tiles see the same patch values as the even kernel's tiles on the plane zero-extended by one row / column, and do
    the same arithmetic in the same order: the odd-plane output is the crop of that output, bit for bit."""
    (H, W), (C, K) = plane, chans
    He, We = H + H % 2, W + W % 2
    N = 2
    x, w, b = _operands(N, C, K, H, W, 3 * H + W)
    U = _weights(w)
    got = _forward([x], U, b, K, act, H, W)
    xe = F.pad(x, (0, We - W, 0, He - H)).contiguous()
    even = _forward([xe], U, b, K, act, He, We)
    assert torch.equal(got, even[:, :, :H, :W])
    if C % 16 == 0:
        parts = [p.contiguous() for p in x.chunk(2, dim=1)]
        parts_e = [p.contiguous() for p in xe.chunk(2, dim=1)]
        assert torch.equal(_forward(parts, U, b, K, act, H, W), _forward(parts_e, U, b, K, act, He, We)[:, :, :H, :W])


def test_odd_plane_writes_nothing_outside_its_output():
    """Row H and column W are never stored: a tensor in the middle of a larger buffer keeps its neighbours."""
    _native, L = _lib()
    N, C, K, H, W = 2, 64, 64, 15, 13
    x, w, b = _operands(N, C, K, H, W, 5)
    U = _weights(w)
    buf = torch.full((3 * N * K * H * W,), 1234.5, device='cuda')
    y = buf[N * K * H * W:2 * N * K * H * W].view(N, K, H, W)
    xs = (ctypes.c_void_p * 1)(x.data_ptr())
    _native.check(L.tai_conv3x3_wino_forward_ex(xs, 1, 0, U.data_ptr(), b.data_ptr(), y.data_ptr(), None, 0, 0, 0, 0, None, None,
                                                N, C, K, H, W, H, W, 0, 0, 1, torch.cuda.current_stream().cuda_stream), 'forward_ex')
    assert bool((buf[:N * K * H * W] == 1234.5).all()) and bool((buf[2 * N * K * H * W:] == 1234.5).all())
    assert _fp64_error(y, x, w, b, 'relu') <= 4e-6


def test_odd_plane_routes_through_conv_ops():
    """conv_bias_act (inference) and the autograd form (forward, input gradient) take the odd plane on the Winograd kernel."""
    from video_frame_inpainting_amd import conv_ops
    conv = torch.nn.Conv2d(256, 256, 3, padding=1).cuda()
    x = torch.randn(16, 256, 15, 20, device='cuda')
    assert conv_ops._wino_ok(16, 256, 256, 15, 20, 3, 3, 1, ragged=True)
    with torch.no_grad():
        y = conv_ops.conv_bias_act(x, conv.weight, conv.bias, 1, 'relu')
        assert ('wino', False, 0) in conv.weight._tai_derived                      # the MFMA kernel ran, not MIOpen
        ref = torch.relu(F.conv2d(x.double(), conv.weight.double(), conv.bias.double(), padding=1))
        assert float((y.double() - ref).abs().max()) <= 5e-5
    xr = x.clone().requires_grad_()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU], record_shapes=True) as prof:
        y = conv_ops.conv_bias_act(xr, conv.weight, conv.bias, 1, 'relu')
        y.backward(torch.ones_like(y))
    from conftest import miopen_convolutions
    assert not miopen_convolutions(prof), miopen_convolutions(prof)[:4]


def _autograd_fp64(parts, w, b, act, gy, transposed):
    """float64 autograd of act(conv(cat(parts), w_eff) + b), w_eff = w (Conv2d) or w transposed and flipped (ConvTranspose2d), with
    the product's ReLU sides (``act_mask``) -- (y, [d part], dw, db)"""
    ps = [p.detach().double().requires_grad_() for p in parts]
    wd, bd = w.double().requires_grad_(), b.double().requires_grad_()
    x = torch.cat(ps, dim=1)
    y = F.conv_transpose2d(x, wd, bd, padding=1) if transposed else F.conv2d(x, wd, bd, padding=1)
    return y, ps, wd, bd


@pytest.mark.parametrize('transposed', [False, True], ids=['conv', 'convT'])
@pytest.mark.parametrize('plane,chans,nparts', [((15, 20), (256, 256), 1), ((15, 20), (256, 256), 2), ((10, 13), (64, 48), 1),
                                                ((10, 13), (64, 48), 2), ((7, 9), (32, 3), 1), ((7, 9), (32, 3), 2),
                                                ((5, 26), (3, 64), 1)],
                         ids=['15x20', '15x20-parts', '10x13', '10x13-parts', '7x9-to3', '7x9-to3-parts', '5x26-from3'])
def test_odd_plane_autograd_gradients_match_fp64(plane, chans, nparts, transposed, monkeypatch):
    """_WinoConv3x3 / _WinoConv3x3Parts under autograd on odd planes (forward, input gradient per part through the transposed weight,
    weight and bias gradients on the ragged weight-gradient kernel) against float64 autograd of the same operands; no ATen convolution."""
    from conftest import miopen_convolutions
    from video_frame_inpainting_amd import conv_ops
    (H, W), (C, K) = plane, chans
    assert C % (8 * nparts) == 0 or nparts == 1
    monkeypatch.setattr(conv_ops, 'WINO_MIN_WORKGROUPS', 1)
    N = 3
    g = torch.Generator().manual_seed(H * 31 + W + C + nparts)
    x = torch.randn(N, C, H, W, generator=g).cuda()
    w = (torch.randn(*((C, K) if transposed else (K, C)), 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).cuda()
    b = (0.1 * torch.randn(K, generator=g)).cuda()
    gy = torch.randn(N, K, H, W, generator=g).cuda()
    parts = [p.contiguous().requires_grad_() for p in x.chunk(nparts, dim=1)]
    wr, br = w.clone().requires_grad_(), b.clone().requires_grad_()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU], record_shapes=True) as prof:
        y = conv_ops.conv_bias_act(parts if nparts > 1 else parts[0], wr, br, 1, 'relu', transposed=transposed)
        y.backward(gy)
    assert not miopen_convolutions(prof), miopen_convolutions(prof)[:4]
    z, ps, wd, bd = _autograd_fp64(parts, w, b, 'relu', gy, transposed)
    (z * (y > 0).double()).backward(gy.double())          # the product's ReLU sides: the comparison is about the convolutions
    got = [y.detach()] + [p.grad for p in parts] + [wr.grad, br.grad]
    want = [torch.relu(z).detach()] + [p.grad for p in ps] + [wd.grad, bd.grad]
    for name, a, r in zip(['y'] + ['gx%d' % i for i in range(nparts)] + ['gw', 'gb'], got, want):
        scale = float(r.abs().max())
        assert scale > 0, name
        err = float((a.double() - r).abs().max()) / scale
        assert err <= 2e-5, (name, err)


@pytest.mark.parametrize('shape', [(3, 2, 256, 512, 20, 26), (3, 2, 24, 40, 6, 10), (2, 2, 3, 64, 22, 14)])
def test_discriminator_layer_on_odd_space_to_depth_planes_matches_fp64(shape, monkeypatch):
    """The sliding-window discriminator's 4x4 stride-2 layer + LeakyReLU (_WindowScaledConvLReLU) on inputs with H or W % 4 == 2 -- a
    space-to-depth plane with an odd side (the last layer at 160 x 208 frames: 20 x 26 -> 10 x 13), HW % 4 != 0 outputs on the scalar
    tail -- forward, input gradient (pixel_shuffle of the transposed 3x3 layer), weight gradient folded back from the ragged kernel and
    bias gradient, against float64 autograd; no ATen convolution, and bit-reproducible."""
    import torch.nn.functional as Fn
    from conftest import miopen_convolutions
    from video_frame_inpainting_amd import conv_ops, sn_discriminator as snd
    nw, B, C, K, H, W = shape
    g = torch.Generator().manual_seed(C + K + H + W)
    x = torch.randn(nw * B, C, H, W, generator=g).cuda()
    w = (torch.randn(K, C, 4, 4, generator=g) * (2.0 / (16 * C)) ** 0.5).cuda()
    b = (0.1 * torch.randn(K, generator=g)).cuda()
    inv = (0.5 + torch.rand(nw, generator=g)).cuda()
    gy = torch.randn(nw * B, K, H // 2, W // 2, generator=g).cuda()
    monkeypatch.setattr(conv_ops, 'WINO_MIN_WORKGROUPS', 1)
    assert snd._s2d_applies(x, w, (2, 2), (1, 1))

    def run():
        xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU], record_shapes=True) as prof:
            y = snd._WindowScaledConvLReLU.apply(xr, wr, wr.detach(), br, inv, nw, (2, 2), (1, 1), 0.2)
            y.backward(gy)
        return (y.detach(), xr.grad, wr.grad, br.grad), miopen_convolutions(prof)

    got, convs = run()
    assert not convs, convs[:4]
    again, _ = run()
    assert all(torch.equal(a, c) for a, c in zip(got, again))
    xd, wd, bd = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    z = Fn.conv2d(xd, wd, None, 2, 1)
    z = (z.view(nw, B, -1) * inv.double().view(nw, 1, 1)).view_as(z) + bd.view(1, -1, 1, 1)
    yd = Fn.leaky_relu(z, 0.2)
    side = (got[0] > 0).double()
    slope = side + 0.2 * (1 - side)
    (z * slope).backward(gy.double())
    # the weight gradient takes the pre-activation gradient without the window's factor (tests/test_gpu_training.py, the same layer)
    wu = w.double().requires_grad_()
    Fn.conv2d(x.double(), wu, None, 2, 1).backward(gy.double() * slope)
    for name, a, r in zip(('y', 'gx', 'gw', 'gb'), got, (yd.detach(), xd.grad, wu.grad, bd.grad)):
        scale = float(r.abs().max())
        err = float((a.double() - r).abs().max()) / scale
        assert err <= 2e-5, (name, err)


# ---- weight gradient on any row length
def _weight_grad_fp64(x, go):
    xd = x.double()
    wd = torch.zeros(go.shape[1], x.shape[1], 3, 3, dtype=torch.float64, device=x.device, requires_grad=True)
    return torch.autograd.grad(F.conv2d(xd, wd, None, padding=1), wd, go.double())[0]


def _wrw(x, go, with_bias=True, window=None, widen=False):
    """tai_conv3x3_wino_wrw / _window straight (``widen``: on both planes zero-extended on the host to an even number of rows and
    roundup(W, 16) columns, the computation the kernel's ragged form reproduces)"""
    _native, L = _lib()
    N, C = x.shape[0], x.shape[1]
    K, H, W = go.shape[1], go.shape[2], go.shape[3]
    if widen:
        He, We = H + H % 2, (W + 15) // 16 * 16
        x, go, H, W = F.pad(x, (0, We - W, 0, He - H)).contiguous(), F.pad(go, (0, We - W, 0, He - H)).contiguous(), He, We
    floats = L.tai_conv3x3_wino_wrw_workspace_floats(N, C, K, H, W)
    assert floats > 0
    ws = torch.full((floats,), float('nan'), device='cuda')
    dw = torch.empty(K, C, 3, 3, device='cuda')
    db = torch.empty(K, device='cuda') if with_bias else None
    s = torch.cuda.current_stream().cuda_stream
    if window is None:
        _native.check(L.tai_conv3x3_wino_wrw(x.data_ptr(), go.data_ptr(), dw.data_ptr(), db.data_ptr() if with_bias else None,
                                             ws.data_ptr(), N, C, K, H, W, s), 'wrw')
    else:
        _native.check(L.tai_conv3x3_wino_wrw_window(x.data_ptr(), go.data_ptr(), dw.data_ptr(), db.data_ptr() if with_bias else None,
                                                    ws.data_ptr(), N, C, K, H, W, x.shape[2], x.shape[3], window[0], window[1], s),
                      'wrw_window')
    return dw, db


@pytest.fixture(params=[2, 4], ids=['wrw-tile2', 'wrw-tile4'])
def wrw_tile(request):
    """the ragged shapes run the F(2x2, 3x3)-domain kernel whichever tile is chosen (F(4x4, 3x3) needs H % 4 == 0 and W % 16 == 0)"""
    from video_frame_inpainting_amd import conv_ops
    prev = conv_ops.set_weight_gradient_tile(request.param)
    yield request.param
    conv_ops.set_weight_gradient_tile(prev)


@pytest.mark.parametrize('W', [13, 20, 24, 26, 40, 52, 104])
@pytest.mark.parametrize('H', [6, 7, 15])
def test_weight_gradient_any_row_length(H, W, wrw_tile):
    N, C, K = 3, 40, 72
    g = torch.Generator().manual_seed(H * 1000 + W)
    x = torch.randn(N, C, H, W, generator=g).cuda()
    go = torch.randn(N, K, H, W, generator=g).cuda()
    dw, db = _wrw(x, go)
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    scale = (N * H * W) ** 0.5
    ref = _weight_grad_fp64(x, go)
    assert (dw.double() - ref).abs().max().item() / scale <= 2e-5
    assert float((db.double() - go.double().sum((0, 2, 3))).abs().max()) / scale <= 2e-5
    # the host-widened computation: the same sums, other split / load scheme -> equal to rounding
    # (tile 4: the widened planes with H % 4 == 0 run the F(4x4, 3x3)-domain kernel, ~7x the rounding of the F(2x2, 3x3) one)
    wd, wb = _wrw(x, go, widen=True)
    bound = 2e-6 if wrw_tile == 2 else 2e-5
    assert (dw - wd).abs().max().item() / scale <= bound
    assert (db - wb).abs().max().item() / scale <= bound
    # a fixed reduction order: two calls, the same bits
    dw2, db2 = _wrw(x, go)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    # and through conv_ops (the autograd paths' entry)
    from video_frame_inpainting_amd import conv_ops
    got = conv_ops.wino_weight_grad(x, go, ragged=True)
    assert got is not None and torch.equal(got, dw)


@pytest.mark.parametrize('W', [13, 20, 26, 52, 104])
@pytest.mark.parametrize('H', [7, 10])
def test_weight_gradient_window_any_row_length(H, W, wrw_tile):
    """The halo-plane form (MotionEnc's 5 x 5 / 7 x 7 stacks, origin (1, 2)): a zero frame around x gives the plain gradient to
    rounding (the frame's zeros stand where the plain entry pads; the frame's last columns lie inside the plane and are read)."""
    N, C, K = 2, 32, 48
    g = torch.Generator().manual_seed(H * 7 + W)
    x = torch.randn(N, C, H, W, generator=g).cuda()
    go = torch.randn(N, K, H, W, generator=g).cuda()
    plane = torch.zeros(N, C, H + 2, W + 4, device='cuda')
    plane[:, :, 1:1 + H, 2:2 + W] = x
    dw, db = _wrw(plane, go, window=(1, 2))
    scale = (N * H * W) ** 0.5
    assert (dw.double() - _weight_grad_fp64(x, go)).abs().max().item() / scale <= 2e-5
    assert torch.equal(db, _wrw(x, go)[1])
    dw2, _ = _wrw(plane, go, window=(1, 2))
    assert torch.equal(dw, dw2)
    # a non-zero frame is read, not padded over: the valid convolution over the framed plane
    plane = torch.randn(N, C, H + 2, W + 4, generator=g).cuda()
    dw, _ = _wrw(plane, go, window=(1, 2))
    wd = torch.zeros(K, C, 3, 3, dtype=torch.float64, device='cuda', requires_grad=True)
    ref = torch.autograd.grad(F.conv2d(plane.double()[:, :, :, 1:-1], wd, None), wd, go.double())[0]
    assert (dw.double() - ref).abs().max().item() / scale <= 2e-5


def test_weight_gradient_even_shapes_keep_their_bits():
    """Shapes the kernel took before (even H, W % 16 == 0) keep their plan, and the W < 16 rows keep the host widening."""
    from video_frame_inpainting_amd import conv_ops
    g = torch.Generator().manual_seed(3)
    for (N, C, K, H, W) in ((2, 16, 16, 8, 16), (3, 24, 40, 6, 32), (2, 40, 24, 6, 12)):
        x = torch.randn(N, C, H, W, generator=g).cuda()
        go = torch.randn(N, K, H, W, generator=g).cuda()
        got = conv_ops.wino_weight_grad(x, go)
        if W % 16 == 0:
            assert torch.equal(got, _wrw(x, go)[0])
        else:
            assert torch.equal(got, _wrw(F.pad(x, (0, 16 - W)).contiguous(), F.pad(go, (0, 16 - W)).contiguous())[0])


def test_weight_gradient_ragged_declines_only_oversized_tensors():
    """With ragged=True (the autograd paths) what the workspace query accepts is what wino_weight_grad takes: every shape but tensors of
    2 GiB or more; the default keeps the old answers (None off the kernel's native grid)."""
    from video_frame_inpainting_amd import conv_ops
    _native, L = _lib()
    for shape in ((1, 8, 6, 24), (1, 8, 5, 16)):
        x, go = torch.randn(*shape, device='cuda'), torch.randn(*shape, device='cuda')
        assert conv_ops.wino_weight_grad(x, go) is None
        got = conv_ops.wino_weight_grad(x, go, ragged=True)
        assert got is not None and float((got.double() - _weight_grad_fp64(x, go)).abs().max()) <= 2e-5 * shape[2] * shape[3]
    assert L.tai_conv3x3_wino_wrw_workspace_floats(1, 8, 8, 5, 13) > 0
    assert L.tai_conv3x3_wino_wrw_workspace_floats(64, 512, 64, 128, 128) == -1       # 2 GiB input
    assert L.tai_conv3x3_wino_wrw_workspace_floats(1, 8, 8, 0, 16) == -1


# ---- the variants that keep even planes
def test_epilogue_variants_still_refuse_odd_planes():
    _native, L = _lib()
    N, C, K = 1, 8, 8
    U = torch.zeros(L.tai_conv3x3_wino_weight_floats(K, C), device='cuda')
    b = torch.zeros(K, device='cuda')
    x = torch.randn(N, C, 8, 8, device='cuda')
    b = torch.ones(K, device='cuda')                     # (a launched kernel would write the bias, not the sentinel)
    y = torch.full((N, K, 8, 8), 1234.5, device='cuda')
    yp = torch.full((N, K, 4, 4), 1234.5, device='cuda')
    s = torch.cuda.current_stream().cuda_stream
    for H, W in ((5, 4), (4, 5), (7, 7)):
        assert L.tai_conv3x3_wino_forward_maxpool(x.data_ptr(), U.data_ptr(), b.data_ptr(), y.data_ptr(), yp.data_ptr(), N, C, K, H, W, 1,
                                                  s) != 0
        assert b'even H and W' in L.tai_sepconv_last_error()
        xs = (ctypes.c_void_p * 1)(x.data_ptr())
        assert L.tai_conv3x3_wino_forward_ex(xs, 1, 0, U.data_ptr(), b.data_ptr(), y.data_ptr(), None, 0, 0, 0, 0, yp.data_ptr(),
                                             y.data_ptr(), N, C, K, H, W, H, W, 0, 0, 0, s) != 0          # unpool + residual epilogue
        assert b'even H and W' in L.tai_sepconv_last_error()
        assert L.tai_conv3x3_wino_forward_window(x.data_ptr(), U.data_ptr(), b.data_ptr(), y.data_ptr(), None, N, C, K, H, W, 8, 8, 0, 0,
                                                 1, s) != 0                                                 # input window
        assert b'even H and W' in L.tai_sepconv_last_error()
    torch.cuda.synchronize()
    assert bool((y == 1234.5).all()) and bool((yp == 1234.5).all())          # nothing was launched


def test_split_arithmetic_refuses_odd_planes():
    from video_frame_inpainting_amd import conv_ops
    _native, L = _lib()
    prev = conv_ops.set_winograd_arithmetic('bf16x3')
    try:
        assert not conv_ops._wino_ok(64, 256, 256, 15, 20, 3, 3, 1, ragged=True)     # conv_ops keeps those planes off the split buffers
        assert conv_ops._wino_ok(64, 256, 256, 16, 20, 3, 3, 1, ragged=True)
        w = torch.randn(64, 64, 3, 3, device='cuda')
        U = _weights(w)
        x = torch.randn(1, 64, 5, 6, device='cuda')
        y = torch.zeros(1, 64, 5, 6, device='cuda')
        b = torch.zeros(64, device='cuda')
        xs = (ctypes.c_void_p * 1)(x.data_ptr())
        assert L.tai_conv3x3_wino_forward_ex(xs, 1, 0, U.data_ptr(), b.data_ptr(), y.data_ptr(), None, 0, 0, 0, 0, None, None,
                                             1, 64, 64, 5, 6, 5, 6, 0, 0, 0, torch.cuda.current_stream().cuda_stream) != 0
        assert b'split' in L.tai_sepconv_last_error()
    finally:
        conv_ops.set_winograd_arithmetic(prev)


# ---- the discriminator's element-wise tail on planes with H * W % 4 != 0
@pytest.mark.parametrize('HW', [130, 6, 1, 4 * 37])
def test_window_scale_tail_on_any_plane(HW):
    _native, L = _lib()
    nw, B, C, slope = 3, 2, 24, 0.2
    g = torch.Generator().manual_seed(HW)
    z = torch.randn(nw * B, C, HW, generator=g).cuda()
    bias = torch.randn(C, generator=g).cuda()
    inv = (0.5 + torch.rand(nw, generator=g)).cuda()
    gy = torch.randn(nw * B, C, HW, generator=g).cuda()
    s = torch.cuda.current_stream().cuda_stream
    y = z.clone()
    _native.check(L.tai_window_scale_bias_lrelu_scalar(y.data_ptr(), bias.data_ptr(), inv.data_ptr(), nw, B, C, HW, slope, s), 'fwd')
    pre = z.double() * inv.double().repeat_interleave(B).view(-1, 1, 1) + bias.double().view(1, -1, 1)
    assert float((y.double() - F.leaky_relu(pre, slope)).abs().max()) <= 1e-6 * (1 + float(pre.abs().max()))
    gz, gs = torch.empty_like(y), torch.empty_like(y)
    _native.check(L.tai_window_scale_lrelu_backward_scalar(gy.data_ptr(), y.data_ptr(), inv.data_ptr(), gz.data_ptr(), gs.data_ptr(), nw, B,
                                                           C, HW, slope, s), 'bwd')
    want = torch.where(y > 0, gy, gy * slope)
    assert torch.equal(gz, want) and torch.equal(gs, want * inv.repeat_interleave(B).view(-1, 1, 1))
    if HW % 4 == 0:        # the 4-element form gives the same bits where it applies
        y4, gz4, gs4 = z.clone(), torch.empty_like(y), torch.empty_like(y)
        _native.check(L.tai_window_scale_bias_lrelu(y4.data_ptr(), bias.data_ptr(), inv.data_ptr(), nw, B, C, HW, slope, s), 'fwd4')
        _native.check(L.tai_window_scale_lrelu_backward(gy.data_ptr(), y4.data_ptr(), inv.data_ptr(), gz4.data_ptr(), gs4.data_ptr(), nw, B,
                                                        C, HW, slope, s), 'bwd4')
        assert torch.equal(y4, y) and torch.equal(gz4, gz) and torch.equal(gs4, gs)
    else:                  # ... and keeps its HW % 4 == 0 contract
        assert L.tai_window_scale_bias_lrelu(y.data_ptr(), bias.data_ptr(), inv.data_ptr(), nw, B, C, HW, slope, s) != 0
