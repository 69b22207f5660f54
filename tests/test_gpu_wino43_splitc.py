"""F(4x4, 3x3) forward with its reduction split over the input channels on small grids (tai_conv3x3_wino43_forward_ws; csrc/wino43_conv.hip.inc,
conv3x3_gen<..., SPLITC> + splitc_reduce): against an fp64 convolution of the same operands, against the unsplit kernel, with every epilogue,
bit for bit from run to run and from graph replay to replay, and bit-identical to the unsplit kernel where the split count is 1.
Shapes: the small-grid layers of the configs[1] forward (N = 160 / 64 / 32).
(Nothing here runs between guard bands: the read behind the end of x with one ragged part, C % 4 != 0, is pinned by the `ws` cases of
tests/test_gpu_wino_kernels.py.)"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

_ACT = {None: 0, 'relu': 1, 'tanh': 2}
TOL = 2e-5           # tests/test_gpu_wino43.py's bound against fp64
CLOSE = 4e-6         # split against unsplit: two summation orders of the same products

# (N, C, K, H, W, nparts)
SHAPES = [(160, 512, 512, 4, 4, 1), (160, 512, 512, 8, 8, 1), (160, 256, 256, 16, 16, 1), (160, 128, 128, 16, 16, 1),
          (160, 256, 512, 8, 8, 1), (160, 256, 128, 16, 16, 1), (160, 64, 64, 32, 32, 1), (160, 128, 64, 32, 32, 1),
          (64, 256, 128, 16, 16, 1), (64, 128, 256, 16, 16, 1), (32, 128, 128, 32, 32, 1), (64, 512, 256, 16, 16, 2),
          (32, 512, 128, 32, 32, 2), (160, 256, 256, 8, 8, 1), (160, 512, 256, 8, 8, 1),
          (160, 512, 51, 8, 8, 1), (160, 512, 512, 8, 8, 4), (64, 206, 130, 8, 8, 1)]


def _lib():
    from video_frame_inpainting_amd import _native
    return _native, _native.lib()


def _operands(N, C, K, H, W, nparts, seed=0):
    g = torch.Generator().manual_seed(seed + N + C + K + H + nparts)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(K, generator=g)
    return x, w, b


def _weights(w):
    _native, L = _lib()
    K, C = w.shape[:2]
    wd = w.cuda()
    U = torch.empty(L.tai_conv3x3_wino43_weight_floats(K, C), device='cuda')
    _native.check(L.tai_conv3x3_wino43_transform_weights(wd.data_ptr(), U.data_ptr(), K, C, torch.cuda.current_stream().cuda_stream),
                  'transform')
    return U


class _Layer(object):
    """Device operands and outputs of one layer; run(split) launches through forward_ws (split: the library's choice) or forward_ex."""

    def __init__(self, shape, act=None, epi=0, seed=0):
        N, C, K, H, W, nparts = shape
        self.shape, self.act, self.epi = shape, act, epi
        x, w, b = _operands(N, C, K, H, W, nparts, seed)
        self.x, self.w, self.b = x, w, b
        self.parts = [p.contiguous().cuda() for p in x.chunk(nparts, dim=1)]
        self.ptrs = (ctypes.c_void_p * nparts)(*[p.data_ptr() for p in self.parts])
        self.U, self.bd = _weights(w), b.cuda()
        self.addx = torch.randn(N, K, H // 2, W // 2).cuda() if epi in (2, 3) else None
        _native, L = _lib()
        self.ws_floats = L.tai_conv3x3_wino43_workspace_floats(N, C, K, H, W, nparts)
        self.ws = torch.empty(max(self.ws_floats, 1), device='cuda')

    def outputs(self):
        N, C, K, H, W, nparts = self.shape
        y = torch.full((N, K, H, W), float('nan'), device='cuda')
        yp = torch.full((N, K, H // 2, W // 2), float('nan'), device='cuda') if self.epi == 1 else None
        y2 = torch.full_like(y, float('nan')) if self.epi == 2 else None
        return y, yp, y2

    def launch(self, split, outs):
        N, C, K, H, W, nparts = self.shape
        _native, L = _lib()
        y, yp, y2 = outs
        ptr = lambda t: t.data_ptr() if t is not None else None
        s = torch.cuda.current_stream().cuda_stream
        if split:
            _native.check(L.tai_conv3x3_wino43_forward_ws(self.ptrs, nparts, self.U.data_ptr(), self.bd.data_ptr(), y.data_ptr(), ptr(yp),
                                                          ptr(self.addx), ptr(y2), self.ws.data_ptr(), self.ws_floats, N, C, K, H, W,
                                                          _ACT[self.act], s), 'forward_ws')
        else:
            _native.check(L.tai_conv3x3_wino43_forward_ex(self.ptrs, nparts, self.U.data_ptr(), self.bd.data_ptr(), y.data_ptr(), ptr(yp),
                                                          ptr(self.addx), ptr(y2), N, C, K, H, W, _ACT[self.act], s), 'forward_ex')

    def run(self, split):
        outs = self.outputs()
        self.launch(split, outs)
        torch.cuda.synchronize()
        return [t for t in outs if t is not None]


def _splits(shape):
    _native, L = _lib()
    return L.tai_conv3x3_wino43_splits(*shape, None)


def _fp64_ref(layer, imgs):
    x = layer.x[imgs].double()
    ref = F.conv2d(x, layer.w.double(), layer.b.double(), padding=1)
    ref = torch.relu(ref) if layer.act == 'relu' else (torch.tanh(ref) if layer.act == 'tanh' else ref)
    mag = F.conv2d(x.abs(), layer.w.double().abs(), layer.b.double().abs(), padding=1)
    return ref, mag


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_splitc_matches_fp64_and_unsplit(shape):
    N = shape[0]
    layer = _Layer(shape)
    got, = layer.run(True)
    base, = layer.run(False)
    assert torch.isfinite(got).all()
    imgs = [0, N // 2, N - 1]
    ref, mag = _fp64_ref(layer, imgs)
    g = got[imgs].cpu().double()
    assert float(((g - ref).abs() / (1 + mag)).max()) <= TOL
    # against the unsplit kernel on every image (the magnitude bound of the fp64 check, from the whole tensor's scale)
    scale = 1 + float(mag.max())
    assert float((got - base).abs().max()) <= CLOSE * scale
    if _splits(shape) == 1:
        assert torch.equal(got, base)


def test_table_layers_split():
    """the layers the split is for do split, and a grid that fills the chip does not"""
    assert _splits((160, 512, 512, 8, 8, 1)) > 1
    assert _splits((64, 512, 256, 16, 16, 2)) > 1
    assert _splits((160, 512, 512, 4, 4, 1)) > 1
    assert _splits((64, 256, 256, 32, 32, 1)) == 1


@pytest.mark.parametrize('act', [None, 'relu', 'tanh'])
def test_splitc_activations(act):
    shape = (160, 512, 256, 8, 8, 1)
    assert _splits(shape) > 1
    layer = _Layer(shape, act=act, seed=1)
    got, = layer.run(True)
    base, = layer.run(False)
    ref, mag = _fp64_ref(layer, [0, 159])
    assert float(((got[[0, 159]].cpu().double() - ref).abs() / (1 + mag)).max()) <= TOL
    assert float((got - base).abs().max()) <= CLOSE * (1 + float(mag.max()))


@pytest.mark.parametrize('epi,act', [(1, None), (1, 'relu'), (2, None), (3, None)])
@pytest.mark.parametrize('shape', [(160, 512, 512, 8, 8, 1), (64, 512, 256, 16, 16, 2), (160, 512, 51, 8, 8, 1)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_splitc_epilogues(shape, epi, act):
    """pooled second output (EPI 1), unpooled residual add into a second output (2) or in place (3): split against unsplit"""
    assert _splits(shape) > 1
    layer = _Layer(shape, act=act, epi=epi, seed=2)
    got = layer.run(True)
    base = layer.run(False)
    for a, b in zip(got, base):
        assert torch.isfinite(a).all()
        assert float((a - b).abs().max()) <= CLOSE * (1 + float(b.abs().max()))


def test_splitc_off_is_the_unsplit_kernel():
    """tai_conv3x3_wino43_set_splitc(0): forward_ws launches exactly the unsplit kernel (the same bits)"""
    _native, L = _lib()
    shape = (160, 512, 512, 8, 8, 1)
    layer = _Layer(shape, act='relu', epi=1)
    prev = L.tai_conv3x3_wino43_set_splitc(0)
    try:
        assert _splits(shape) == 1 and L.tai_conv3x3_wino43_workspace_floats(*shape) == 0
        got = layer.run(True)
    finally:
        L.tai_conv3x3_wino43_set_splitc(prev)
    base = layer.run(False)
    assert all(torch.equal(a, b) for a, b in zip(got, base))


@pytest.mark.parametrize('shape', [(160, 512, 512, 8, 8, 1), (64, 512, 256, 16, 16, 2)], ids=lambda s: 'x'.join(map(str, s)))
def test_splitc_repeats_bit_for_bit(shape):
    """two runs and two replays of a captured graph give the same bits (fixed summation order, no atomics)"""
    layer = _Layer(shape, act='relu', epi=1, seed=3)
    first, second = layer.run(True), layer.run(True)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    outs = layer.outputs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        layer.launch(True, outs)        # warm-up outside the capture (LDS attribute, code object load)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        layer.launch(True, outs)
    replays = []
    for _ in range(2):
        for t in outs:
            if t is not None:
                t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        replays.append([t.clone() for t in outs if t is not None])
    assert all(torch.equal(a, b) for a, b in zip(replays[0], first))
    assert all(torch.equal(a, b) for a, b in zip(replays[1], first))
