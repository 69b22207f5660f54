"""numpy float64 restatement of the SSIM training loss as include/tai_sepconv.h defines it for tai_ssim_loss, operation for operation
(numpy's element-wise float64 arithmetic is one IEEE operation per written operation: no contraction).  Shared by the CPU and the GPU
tests; the inputs it makes are seeded."""
import numpy as np

C1, C2, COV = 0.01 * 0.01, 0.03 * 0.03, 49.0 / 48.0


def _sum7(m):
    """[..., h, w] -> [..., h-6, w-6]: vertical 7-row sums (k ascending, from 0.0), then horizontal sums of 7 of those."""
    h, w = m.shape[-2:]
    v = np.zeros(m.shape[:-2] + (h - 6, w), np.float64)
    for k in range(7):
        v = v + m[..., k:k + h - 6, :]
    s = np.zeros(m.shape[:-2] + (h - 6, w - 6), np.float64)
    for k in range(7):
        s = s + v[..., :, k:k + w - 6]
    return s


def ssim_loss_ref(pred, gt):
    """pred, gt: arrays [..., C, H, W] of one shape.  float32 inputs follow the definition (x = (pred + 1) / 2 in fp32); float64 inputs
    are mapped in float64 (the form the torch path takes for float64 tensors).  -> dict: S [N*C, H-6, W-6], plane_ssim [N*C], mean_ssim,
    loss (float64), grad64 and grad (float32, pred's shape), term_scale."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    assert pred.shape == gt.shape and pred.dtype == gt.dtype and pred.dtype in (np.float32, np.float64)
    H, W = pred.shape[-2:]
    one, two = pred.dtype.type(1), pred.dtype.type(2)
    x = ((pred + one) / two).astype(np.float64).reshape(-1, H, W)
    y = ((gt + one) / two).astype(np.float64).reshape(-1, H, W)
    planes = x.shape[0]
    with np.errstate(all='ignore'):
        ux, uy = _sum7(x) / 49.0, _sum7(y) / 49.0
        uxx, uyy, uxy = _sum7(x * x) / 49.0, _sum7(y * y) / 49.0, _sum7(x * y) / 49.0
        vx, vy, vxy = COV * (uxx - ux * ux), COV * (uyy - uy * uy), COV * (uxy - ux * uy)
        A1, A2 = (2.0 * ux) * uy + C1, 2.0 * vxy + C2
        B1, B2 = (ux * ux + uy * uy) + C1, (vx + vy) + C2
        D = B1 * B2
        S = (A1 * A2) / D
        plane_ssim = np.array([S[n].sum() for n in range(planes)]) / (float(H - 6) * float(W - 6))
        mean_ssim = plane_ssim.sum() / float(planes)
        gamma = -(((2.0 * COV) * S) / B2)
        beta = ((2.0 * COV) * A1) / D
        alpha = ((((2.0 * uy) * A2) / D - ((2.0 * S) * ux) / B1) - beta * uy) - gamma * ux
        pad = lambda m: np.pad(m, ((0, 0), (6, 6), (6, 6)))          # windows outside the interior count as zero
        Sa, Sb, Sg = _sum7(pad(alpha)), _sum7(pad(beta)), _sum7(pad(gamma))
        dS = ((Sa + y * Sb) + x * Sg) / 49.0
        divisor = float(planes) * (float(H - 6) * float(W - 6))
        grad64 = ((-0.5 * dS) / divisor).reshape(pred.shape)
        grad = grad64.astype(np.float32)
        # the size of the three terms the gradient is the sum of: what its rounding error scales with where they cancel (pred == gt)
        term_scale = float(((np.abs(Sa) + np.abs(y * Sb) + np.abs(x * Sg)) / 49.0 * 0.5 / divisor).max())
    return dict(S=S, plane_ssim=plane_ssim, mean_ssim=mean_ssim, loss=1.0 - mean_ssim, grad64=grad64, grad=grad, term_scale=term_scale)


KINDS = ('uniform', 'smooth', 'equal', 'flat', 'wide')


def make_pair(kind, shape, seed):
    """Seeded float32 (pred, gt) of ``shape`` [..., H, W]: uniform random in [-1, 1]; a smooth pattern plus 2 % noise; pred == gt; flat
    planes with different levels; uniform values scaled to [-1.5, 1.5]."""
    rs = np.random.RandomState(seed)
    H, W = shape[-2:]
    lead = tuple(shape[:-2])
    if kind == 'uniform':
        pred, gt = rs.uniform(-1, 1, shape), rs.uniform(-1, 1, shape)
    elif kind == 'smooth':
        r, c = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        phase = rs.uniform(0, 6.28, lead + (1, 1))
        gt = 0.6 * np.sin(r / 9.0 + phase) * np.cos(c / 7.0 - phase) + 0.1
        pred = gt + 0.02 * rs.standard_normal(shape)
    elif kind == 'equal':
        gt = rs.uniform(-1, 1, shape)
        pred = gt.copy()
    elif kind == 'flat':
        pred = np.broadcast_to(rs.uniform(-1, 1, lead + (1, 1)), shape)
        gt = np.broadcast_to(rs.uniform(-1, 1, lead + (1, 1)), shape)
    elif kind == 'wide':
        pred, gt = rs.uniform(-1.5, 1.5, shape), rs.uniform(-1.5, 1.5, shape)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(pred, dtype=np.float32), np.ascontiguousarray(gt, dtype=np.float32)
