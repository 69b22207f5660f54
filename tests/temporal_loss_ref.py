"""numpy restatement of the temporal-difference loss as include/tai_sepconv.h defines it for tai_temporal_loss, operation for operation
(numpy's element-wise arithmetic is one IEEE operation per written operation in the arrays' own precision: no contraction; its fp32
division and square root are correctly rounded).  Shared by the CPU and the GPU tests; the inputs it makes are seeded."""
import numpy as np

KIND_NAMES = ('l2', 'l1', 'charbonnier')          # kind 0, 1, 2 of the C ABI


def _sgn(v):
    """sgn(0) = 0 (either zero), NaN kept; in v's precision."""
    s = (v > 0).astype(v.dtype) - (v < 0).astype(v.dtype)
    return np.where(np.isnan(v), v, s)


def temporal_loss_ref(pred, gt, kind, eps=1e-3):
    """pred, gt: float32 arrays [B, T, C, H, W] of one shape; kind 0 (L2), 1 (L1), 2 (Charbonnier).  -> dict: seq_terms [B * C, T + 1]
    float64 (the sum of rho(d_j) per sequence b * C + c, summed by numpy: the order is not the kernel's), terms [T + 1] (per-position
    means), loss (float64), count, ct, grad64 and grad (float32, pred's shape), delta, rho, drho (the fp32 terms [B, T + 1, C, H, W])."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    assert pred.shape == gt.shape and pred.ndim == 5 and pred.dtype == gt.dtype == np.float32 and kind in (0, 1, 2)
    B, T, C, H, W = pred.shape
    assert min(pred.shape) >= 1
    f = np.float32
    with np.errstate(all='ignore'):
        x = (pred + f(1)) / f(2)
        y = (gt + f(1)) / f(2)
        e = np.zeros((B, T + 2, C, H, W), np.float32)             # e_{-1} = +0, e_0 .. e_{T-1}, e_T = +0
        e[:, 1:T + 1] = x - y
        d = e[:, 1:] - e[:, :-1]                                  # d_0 .. d_T
        if kind == 0:
            rho, drho = d * d, f(2) * d
        elif kind == 1:
            rho, drho = np.abs(d), _sgn(d)
        else:
            e2 = f(eps) * f(eps)
            s = np.sqrt(d * d + e2)
            rho, drho = s, d / s
        assert d.dtype == rho.dtype == drho.dtype == np.float32
        seq_terms = rho.astype(np.float64).sum(axis=(3, 4)).transpose(0, 2, 1).reshape(B * C, T + 1)
        S = B * C
        n_pos = float(S) * H * W
        count = float(S) * (T + 1) * H * W
        terms = seq_terms.sum(axis=0) / n_pos
        loss = seq_terms.sum() / count
        ct = 0.5 / count
        grad64 = (drho[:, :-1].astype(np.float64) - drho[:, 1:].astype(np.float64)) * ct
        grad = grad64.astype(np.float32)
    return dict(seq_terms=seq_terms, terms=terms, loss=loss, count=count, ct=ct, grad64=grad64, grad=grad, delta=d, rho=rho, drho=drho)


KINDS = ('uniform', 'smooth', 'equal', 'wide', 'grid')


def make_pair(kind, shape, seed):
    """Seeded float32 (pred, gt) of ``shape`` [B, T, C, H, W]: uniform random in [-1, 1]; a pattern that drifts over t plus 2 % noise;
    pred == gt; uniform in [-3, 3] (unclipped); values k / 64 - 1 with k integer in [0, 128], about a third of pred's pixels copied from gt
    (ties d = 0 are frequent; every x, y is a multiple of 2^-7 in [0, 1], so every d is a multiple of 2^-7 of size at most 2 and every
    rho of kind 0 and 1 a multiple of 2^-14 below 4: float64 sums of up to 2^18 of them are exact in any order)."""
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
    elif kind == 'wide':
        pred, gt = rs.uniform(-3, 3, shape), rs.uniform(-3, 3, shape)
    elif kind == 'grid':
        gt = rs.randint(0, 129, shape) / 64.0 - 1.0
        pred = rs.randint(0, 129, shape) / 64.0 - 1.0
        pred = np.where(rs.uniform(0, 1, shape) < 1.0 / 3.0, gt, pred)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(pred, dtype=np.float32), np.ascontiguousarray(gt, dtype=np.float32)
