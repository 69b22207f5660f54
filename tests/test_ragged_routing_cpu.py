"""Routing is unchanged by the odd-plane kernels: _wino_ok, the weight-gradient kernel's shape acceptance and the discriminator's
space-to-depth rule give their old answers on every shape they accepted before -- every layer plane of configs[0-4] (128 x 128,
256 x 256 frames, TAI_gray / TAI_color, the 8 x 8 ... 2 x 2 kernel-network bottoms) and of the 64 x 96 training test -- and differ
only on shapes that were refused (odd planes, rows that are not a multiple of 16 pixels)."""
import itertools
from types import SimpleNamespace

import torch

from video_frame_inpainting_amd import conv_ops, sn_discriminator


def _old_wino_ok(N, Ci, Co, H, W, kh, kw, padding, min_ci=8):
    # conv_ops._wino_ok before odd planes were taken
    return (kh == kw == 3 and padding == 1 and H % 2 == 0 and W % 2 == 0 and Ci >= min_ci and N * max(Ci, Co) * H * W < 2 ** 29
            and ((N * (H // 2) * (W // 2) + 63) // 64) * ((Co + 63) // 64) >= conv_ops.WINO_MIN_WORKGROUPS)


def _old_s2d(H, W):
    return H % 4 == 0 and W % 4 == 0


def _planes(h, w, levels=6):
    out = []
    for _ in range(levels):
        out.append((h, w))
        h, w = h // 2, w // 2
        if h == 0 or w == 0:
            break
    return out


# frames of configs[0-4] and of tests/test_gpu_training.py's non-square step; the published shapes for the odd side
FRAMES_BEFORE = [(128, 128), (256, 256), (64, 96)]
FRAMES_NEW = [(240, 320), (160, 208)]
CHANNELS = [1, 2, 3, 8, 16, 24, 32, 51, 64, 128, 256, 512, 1024]
BATCHES = [1, 2, 4, 8, 16, 32, 64, 80, 160]


def _shapes(frames):
    planes = sorted(set(p for f in frames for p in _planes(*f)))
    return planes


def test_wino_ok_keeps_every_old_answer():
    n_before = 0
    for (H, W), Ci, Co, N in itertools.product(_shapes(FRAMES_BEFORE + FRAMES_NEW), CHANNELS, CHANNELS, BATCHES):
        for min_ci in (8, 2):
            old = _old_wino_ok(N, Ci, Co, H, W, 3, 3, 1, min_ci=min_ci)
            new = conv_ops._wino_ok(N, Ci, Co, H, W, 3, 3, 1, min_ci=min_ci, ragged=True)
            if old:
                n_before += 1
                assert new, (N, Ci, Co, H, W)
            elif new:
                assert H % 2 or W % 2, (N, Ci, Co, H, W)       # only odd planes are new
            # the even-plane variants (epilogues, windows, displaced reads) -- the default -- answer exactly as before
            assert conv_ops._wino_ok(N, Ci, Co, H, W, 3, 3, 1, min_ci=min_ci) == old
    assert n_before > 1000


def test_odd_planes_are_taken_at_the_published_shapes():
    # the kernel network's 256 -> 256 layers on its 15 x 20 / 10 x 13 bottom at the batch of 16 / 32 clips
    assert not _old_wino_ok(16 * 3, 256, 256, 15, 20, 3, 3, 1) and conv_ops._wino_ok(16 * 3, 256, 256, 15, 20, 3, 3, 1, ragged=True)
    assert conv_ops._wino_ok(32 * 3, 256, 256, 10, 13, 3, 3, 1, ragged=True)
    assert not conv_ops._wino_ok(32 * 3, 256, 256, 10, 13, 3, 3, 1)
    # the workgroup count uses ceil tiles (a 1 x 1 plane is one tile)
    assert conv_ops._wino_ok(64 * 72, 64, 64, 1, 1, 3, 3, 1, ragged=True) and not conv_ops._wino_ok(64 * 71, 64, 64, 1, 1, 3, 3, 1, ragged=True)
    # the A/B switch restores the old answers
    prev = conv_ops.set_ragged_routes(False)
    try:
        assert not conv_ops._wino_ok(16 * 3, 256, 256, 15, 20, 3, 3, 1, ragged=True)
    finally:
        conv_ops.set_ragged_routes(prev)


def test_split_arithmetic_keeps_even_planes_only():
    prev = conv_ops._WINO_ARITH[0]
    try:
        conv_ops._WINO_ARITH[0] = 1
        assert not conv_ops._wino_ok(64, 256, 256, 15, 20, 3, 3, 1, ragged=True)
        assert conv_ops._wino_ok(64, 256, 256, 16, 20, 3, 3, 1, ragged=True) == _old_wino_ok(64, 256, 256, 16, 20, 3, 3, 1)
    finally:
        conv_ops._WINO_ARITH[0] = prev


class _StubLib(object):
    """The two entry points wino_weight_grad calls, recording the shapes it hands to the workspace query and to the kernel; the query
    answers as the library does for tensors below 2 GiB (any shape)."""

    def __init__(self):
        self.queried, self.launched = [], []

    def tai_conv3x3_wino_wrw_workspace_floats(self, N, C, K, H, W):
        self.queried.append((N, C, K, H, W))
        return 1 if N * max(C, K) * H * W * 4 < 2 ** 31 else -1

    def tai_conv3x3_wino_wrw(self, x, dy, dw, db, ws, N, C, K, H, W, stream):
        self.launched.append((N, C, K, H, W))
        return 0

    def tai_conv3x3_wino_wrw_window(self, x, dy, dw, db, ws, N, C, K, H, W, in_h, in_w, oy, ox, stream):
        self.launched.append((N, C, K, H, W))
        return 0


class _CpuTensor(object):
    """Shape, dtype and pointer of a tensor, without storage: wino_weight_grad's decisions depend on nothing else."""

    def __init__(self, *shape):
        self.shape, self.dtype, self.device = shape, torch.float32, torch.device('cpu')

    def data_ptr(self):
        return 0


def _old_wrw_takes(H, W, window):
    # conv_ops.wino_weight_grad before the ragged kernel: kernel-native shapes, and rows < 16 pixels on even H widened on the host
    return H % 2 == 0 and (W % 16 == 0 or (window is None and W < 16))


def test_weight_gradient_shape_acceptance(monkeypatch):
    """wino_weight_grad without ragged gives its old answer on every plane of the configs and of the published shapes, and hands the
    kernel the same (widened) shape as before; with ragged=True it takes every shape, unwidened except for the host widening of rows
    shorter than 16 pixels on an even number of rows (the same bits as before for those)."""
    from video_frame_inpainting_amd import _native
    stub = _StubLib()
    monkeypatch.setattr(_native, 'lib', lambda: stub)
    monkeypatch.setattr(conv_ops._WRW_WORKSPACE, 'get', lambda device, floats: _CpuTensor(floats))
    monkeypatch.setattr(conv_ops.torch, 'empty', lambda *a, **k: _CpuTensor(*a[0]) if isinstance(a[0], tuple) else _CpuTensor(*a))
    monkeypatch.setattr(conv_ops.torch.cuda, 'device', lambda d: __import__('contextlib').nullcontext())
    monkeypatch.setattr(conv_ops.torch.cuda, 'current_stream', lambda d: SimpleNamespace(cuda_stream=None))
    monkeypatch.setattr(conv_ops.F, 'pad', lambda t, pad: _CpuTensor(t.shape[0], t.shape[1], t.shape[2], t.shape[3] + pad[1]))
    monkeypatch.setattr(_native, 'check', lambda rc, what: None)
    n = 0
    for (H, W) in _shapes(FRAMES_BEFORE + FRAMES_NEW) + [(7, 13), (15, 20), (1, 1), (5, 16), (6, 24)]:
        for window in (None, (1, 2)):
            x = _CpuTensor(2, 16, H + 2, W + 4) if window else _CpuTensor(2, 16, H, W)
            go = _CpuTensor(2, 32, H, W)
            for ragged in (False, True):
                stub.launched.clear()
                r = conv_ops.wino_weight_grad(x, go, window=window, ragged=ragged)
                old = _old_wrw_takes(H, W, window)
                if not ragged:
                    assert (r is not None) == old, (H, W, window)
                else:
                    assert r is not None, (H, W, window)
                if r is not None:
                    widened = window is None and H % 2 == 0 and W < 16 and W % 16
                    assert stub.launched == [(2, 16, 32, H, 16 if widened else W)], (H, W, window, ragged, stub.launched)
                    n += 1
    assert n > 50
    prev = conv_ops.set_ragged_routes(False)        # the A/B switch: the old answers with ragged=True too
    try:
        assert conv_ops.wino_weight_grad(_CpuTensor(2, 16, 15, 20), _CpuTensor(2, 32, 15, 20), ragged=True) is None
    finally:
        conv_ops.set_ragged_routes(prev)


def _fake(shape):
    return SimpleNamespace(is_cuda=True, dtype=torch.float32, shape=shape)


def test_s2d_applies_keeps_every_old_answer():
    w = _fake((64, 32, 4, 4))
    frames = FRAMES_BEFORE + FRAMES_NEW
    for (H, W) in _shapes(frames) + [(h, w_) for h in range(1, 24) for w_ in range(1, 24)]:
        x = _fake((2, 32, H, W))
        new = sn_discriminator._s2d_applies(x, w, (2, 2), (1, 1))
        if _old_s2d(H, W):
            assert new, (H, W)
        else:
            assert new == (H % 2 == 0 and W % 2 == 0), (H, W)
        assert not sn_discriminator._s2d_applies(x, _fake((64, 32, 3, 3)), (2, 2), (1, 1))
    # 160 x 208: the last layer's 20 x 26 input (a 10 x 13 space-to-depth plane) now takes the in-tree route
    assert not _old_s2d(20, 26) and sn_discriminator._s2d_applies(_fake((2, 256, 20, 26)), w, (2, 2), (1, 1))
