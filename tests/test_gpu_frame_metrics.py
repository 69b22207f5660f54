"""The HIP frame-metrics kernels (csrc/frame_metrics.hip.inc) through metrics.compute_errors_device against the host restatement
metrics.compute_errors: PSNR bit-identical, SSIM to 1e-12, L2 to 1e-6 relative; reproducible, batch-independent, isolated from
non-finite frames, capturable into a hipGraph."""
import numpy as np
import pytest
import torch

from video_frame_inpainting_amd import metrics, synthetic

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _steps_near_uint8_edges(shape, seed):
    """Values a few ulp below and above every uint8 step k/255*2-1, values outside [-1, 1], and plain noise."""
    rs = np.random.RandomState(seed)
    k = rs.randint(0, 256, shape)
    edge = (k / 255. * 2 - 1).astype(np.float32)
    ulps = rs.randint(-3, 4, shape).astype(np.int32)
    bits = edge.view(np.int32) + np.where(edge < 0, -ulps, ulps)
    near = bits.view(np.float32)
    out = rs.uniform(-1.5, 1.5, shape).astype(np.float32)
    noise = rs.uniform(-1, 1, shape).astype(np.float32)
    pick = rs.randint(0, 3, shape)
    return np.where(pick == 0, near, np.where(pick == 1, out, noise)).astype(np.float32)


def _pair(B, T, C, H, W, seed):
    clips = synthetic.make_clips(B, 2 * T, C, H, W, seed)
    gt = clips[:, :T].copy()
    pred = clips[:, T:].copy()
    pred[:, 0] = _steps_near_uint8_edges(pred[:, 0].shape, seed)          # edge values against smooth frames
    gt[-1, -1] = _steps_near_uint8_edges(gt[-1, -1].shape, seed + 1)
    if T > 1:
        pred[0, 1] = gt[0, 1]                                              # identical frames: PSNR inf, SSIM 1
    return pred, gt


def _check(pred, gt):
    ref = metrics.compute_errors(pred, gt)
    got = metrics.compute_errors_device(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV))
    for r, g in zip(ref, got):
        assert g.dtype == np.float64 and g.shape == r.shape
    assert np.array_equal(got[0], ref[0]), (got[0], ref[0])                                  # PSNR bit for bit (inf included)
    np.testing.assert_allclose(got[1], ref[1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got[2], ref[2], rtol=1e-6, atol=0)
    return got


@pytest.mark.parametrize('B,T,C,H,W', [
    (4, 5, 1, 128, 128),
    (2, 3, 3, 256, 256),
    (2, 2, 3, 240, 320),
    (3, 2, 1, 15, 20),
    (2, 2, 3, 15, 20),
    (2, 2, 1, 7, 7),
    (2, 2, 3, 7, 9),
    (1, 3, 1, 23, 71),          # one past a tile edge in both directions
])
def test_device_metrics_match_host(B, T, C, H, W):
    pred, gt = _pair(B, T, C, H, W, 11 + H + W)
    psnr, ssim, _ = _check(pred, gt)
    if T > 1:
        assert psnr[0, 1] == float('inf') and ssim[0, 1] == 1.0


def test_runs_are_bitwise_reproducible_and_batch_independent():
    pred, gt = _pair(6, 3, 3, 64, 80, 5)
    p, g = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    a = metrics.compute_errors_device(p, g)
    b = metrics.compute_errors_device(p, g)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))
    sub = metrics.compute_errors_device(p[2:4], g[2:4])           # the same clips inside a smaller batch
    for x, y in zip(a, sub):
        assert np.array_equal(x[2:4].view(np.int64), y.view(np.int64))


def test_non_finite_frame_leaves_the_others_alone():
    pred, gt = _pair(3, 4, 1, 40, 48, 9)
    p, g = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    clean = metrics.compute_errors_device(p, g)
    p2, g2 = p.clone(), g.clone()
    p2[1, 2, 0, 5, 7] = float('nan')
    g2[1, 2, 0, 9, 9] = float('inf')
    p2[2, 0] = float('-inf')
    dirty = metrics.compute_errors_device(p2, g2)
    torch.cuda.synchronize()
    keep = np.ones((3, 4), bool)
    keep[1, 2] = keep[2, 0] = False
    for x, y in zip(clean, dirty):
        assert np.array_equal(x[keep].view(np.int64), y[keep].view(np.int64))


def test_graph_capture_replays_the_eager_bits():
    pred, gt = _pair(4, 5, 1, 128, 128, 3)
    p, g = torch.from_numpy(pred).to(DEV).reshape(20, 1, 128, 128), torch.from_numpy(gt).to(DEV).reshape(20, 1, 128, 128)
    eager = metrics.frame_metrics_device(p, g).cpu()
    from video_frame_inpainting_amd import _native
    nbytes = _native.lib().tai_frame_metrics_workspace_bytes(20, 1, 128, 128)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.full((3, 20), -1.0, dtype=torch.float64, device=DEV)
    metrics.frame_metrics_device(p, g, out, ws)                    # warm-up outside the capture
    out.fill_(-1.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        metrics.frame_metrics_device(p, g, out, ws)
    out.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int64), eager.view(torch.int64))
    # the int64 row is the exact SSE
    u = lambda x: ((np.clip(x, -1, 1) + np.float32(1)) / np.float32(2) * np.float32(255)).astype(np.uint8).astype(np.int64)
    want = ((u(pred) - u(gt)) ** 2).reshape(20, -1).sum(axis=1)
    assert np.array_equal(eager[0].view(torch.int64).numpy(), want)


@pytest.mark.parametrize('H,W', [(6, 32), (32, 6), (1, 1)])
def test_planes_below_the_window_are_refused(H, W):
    x = torch.zeros(1, 2, 1, H, W, device=DEV)
    with pytest.raises(ValueError):
        metrics.compute_errors_device(x, x)
    from video_frame_inpainting_amd import _native
    L = _native.lib()
    assert L.tai_frame_metrics_workspace_bytes(2, 1, H, W) < 0
    out = torch.empty(3, 2, dtype=torch.float64, device=DEV)
    ws = torch.empty(1024, dtype=torch.uint8, device=DEV)
    rc = L.tai_frame_metrics(x.data_ptr(), x.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(),
                             2, 1, H, W, torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b'7' in L.tai_sepconv_last_error()
