"""numpy restatement of the census (soft ternary) loss as include/tai_sepconv.h defines it for tai_census_loss, operation for operation
(numpy's element-wise arithmetic is one IEEE operation per written operation in the arrays' own precision: no contraction; its fp32
division and square root are correctly rounded).  Shared by the CPU and the GPU tests; the inputs it makes are seeded."""
import numpy as np

R = 3                                           # the window reaches 3 pixels each way
OFFSETS = [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if (dy, dx) != (0, 0)]          # "the order"
GRAY = (0.1140, 0.5870, 0.2989)                 # util.gray01's weights, in its operand order


def intensity(frames, f=np.float32):
    """[B, T, C, H, W] in [-1, 1] -> I [B, T, H, W] in precision ``f``: the range map per channel, then gray for C = 3."""
    x = (frames.astype(f) + f(1)) / f(2)
    if frames.shape[2] == 1:
        return x[:, :, 0]
    w0, w1, w2 = (f(np.float32(w)) for w in GRAY)               # the fp32 constants, whatever the precision
    return (w0 * x[:, :, 0] + w1 * x[:, :, 1]) + w2 * x[:, :, 2]


def census_loss_ref(pred, gt, f=np.float32):
    """pred, gt: float32 arrays [B, T, C, H, W] of one shape, C in {1, 3}, H, W >= 7.  -> dict: frame_terms [B * T] float64 (the sum
    over Omega is numpy's: the order is not the kernel's), loss (float64), count, kappa, G [B, T, H, W] float64, grad64 (float64) and grad
    (float32), both of pred's shape.  ``f = np.float64`` evaluates every fp32 operation of the definition in float64 instead (the constants
    stay the fp32 ones widened, as the gray weights do)."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    assert pred.shape == gt.shape and pred.ndim == 5 and pred.dtype == gt.dtype == np.float32
    B, T, C, H, W = pred.shape
    assert C in (1, 3) and H >= 2 * R + 1 and W >= 2 * R + 1 and B >= 1 and T >= 1
    c32 = np.float32
    k255, k81, k1, k2 = f(c32(255)), f(c32(0.81)), f(c32(0.1)), f(c32(2))
    with np.errstate(all='ignore'):
        I, J = intensity(pred, f), intensity(gt, f)
        omega = np.zeros((H, W), bool)
        omega[R:H - R, R:W - R] = True
        phi_sum = np.zeros((B, T, H - 2 * R, W - 2 * R), np.float64)
        acc = np.zeros((B, T, H, W), np.float64)
        for dy, dx in OFFSETS:
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)          # the q with q + j in the plane
            here = (slice(None), slice(None), slice(y0, y1), slice(x0, x1))
            there = (slice(None), slice(None), slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            s = k255 * (I[there] - I[here])
            u = k81 + s * s
            r = np.sqrt(u)
            t = s / r
            sp = k255 * (J[there] - J[here])
            up = k81 + sp * sp
            tp = sp / np.sqrt(up)
            d = t - tp
            e = d * d
            n = k1 + e
            phi = e / n
            dphi = ((k2 * d) * k1) / (n * n)
            tau = k81 / (u * r)
            assert phi.dtype == dphi.dtype == tau.dtype == f
            w = dphi.astype(np.float64) * tau.astype(np.float64)
            m = omega[y0:y1, x0:x1].astype(np.float64) + omega[y0 + dy:y1 + dy, x0 + dx:x1 + dx].astype(np.float64)
            acc[here] = acc[here] + m * w
            phi_sum = phi_sum + phi[:, :, R - y0:H - R - y0, R - x0:W - R - x0].astype(np.float64)
        D = phi_sum / 49.0
        interior = float((H - 2 * R) * (W - 2 * R))
        frame_terms = D.sum(axis=(2, 3)).reshape(B * T) / interior
        loss = float(np.cumsum(frame_terms)[-1] / float(B * T))                     # in frame order, from 0.0
        count = float(B * T) * interior
        kappa = (255.0 * 0.5) / (49.0 * count)
        G = -acc
        gk = G * kappa
        if C == 1:
            grad64 = gk[:, :, None]
        else:
            grad64 = np.stack([gk * float(c32(wc)) for wc in GRAY], axis=2)
        grad = grad64.astype(np.float32)
    return dict(frame_terms=frame_terms, loss=loss, count=count, kappa=kappa, G=G, grad64=grad64, grad=grad)


KINDS = ('uniform', 'smooth', 'equal', 'flat', 'wide', 'dyadic')


def make_pair(kind, shape, seed):
    """Seeded float32 (pred, gt) of ``shape`` [B, T, C, H, W]: uniform random in [-1, 1]; a sinusoid plus 2 % noise; pred == gt; flat
    planes (one value per frame and tensor: every s is 0); uniform in [-3, 3] (unclipped); multiples of 2^-8 in [-1, 1]."""
    rs = np.random.RandomState(seed)
    B, T, C, H, W = shape
    if kind == 'uniform':
        pred, gt = rs.uniform(-1, 1, shape), rs.uniform(-1, 1, shape)
    elif kind == 'smooth':
        r, c = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        phase = rs.uniform(0, 6.28, (B, 1, C, 1, 1)) + 0.3 * np.arange(T).reshape(1, T, 1, 1, 1)
        gt = 0.6 * np.sin(r / 9.0 + phase) * np.cos(c / 7.0 - phase) + 0.1
        pred = gt + 0.02 * rs.standard_normal(shape)
    elif kind == 'equal':
        gt = rs.uniform(-1, 1, shape)
        pred = gt.copy()
    elif kind == 'flat':
        pred = np.broadcast_to(rs.uniform(-1, 1, (B, T, C, 1, 1)), shape)
        gt = np.broadcast_to(rs.uniform(-1, 1, (B, T, C, 1, 1)), shape)
    elif kind == 'wide':
        pred, gt = rs.uniform(-3, 3, shape), rs.uniform(-3, 3, shape)
    elif kind == 'dyadic':
        pred, gt = rs.randint(-256, 257, shape) / 256.0, rs.randint(-256, 257, shape) / 256.0
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(pred, dtype=np.float32), np.ascontiguousarray(gt, dtype=np.float32)
