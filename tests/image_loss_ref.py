"""numpy restatement of the pointwise + gradient-difference image loss as include/tai_sepconv.h defines it for tai_image_loss, operation for
operation (numpy's element-wise arithmetic is one IEEE operation per written operation in the arrays' own precision: no contraction; its
fp32 division and square root are correctly rounded).  Shared by the CPU and the GPU tests; the inputs it makes are seeded."""
import numpy as np

KIND_NAMES = ('l2', 'l1', 'charbonnier')          # kind 0, 1, 2 of the C ABI


def _sgn(v):
    """sgn(0) = 0 (either zero), NaN kept; in v's precision."""
    s = (v > 0).astype(v.dtype) - (v < 0).astype(v.dtype)
    return np.where(np.isnan(v), v, s)


def image_loss_ref(pred, gt, kind, eps=1e-3):
    """pred, gt: float32 arrays [..., H, W] of one shape; kind 0 (L2), 1 (L1), 2 (Charbonnier).  -> dict: plane_terms [P, 2] float64
    (sum of rho, sum of |gw| + |gh| per plane, summed by numpy: the order is not the kernel's), point, gdl, loss (float64), grad64 and
    grad (float32, pred's shape), S (the integer map, float32), rho, gw, gh (the fp32 terms: for order-independence checks)."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    assert pred.shape == gt.shape and pred.dtype == gt.dtype == np.float32 and kind in (0, 1, 2)
    H, W = pred.shape[-2:]
    assert H >= 2 and W >= 2
    f = np.float32
    with np.errstate(all='ignore'):
        x = ((pred + f(1)) / f(2)).reshape(-1, H, W)
        y = ((gt + f(1)) / f(2)).reshape(-1, H, W)
        P = x.shape[0]
        d = x - y
        if kind == 0:
            rho, drho = d * d, f(2) * d
        elif kind == 1:
            rho, drho = np.abs(d), _sgn(d)
        else:
            e2 = f(eps) * f(eps)
            s = np.sqrt(d * d + e2)
            rho, drho = s, d / s
        assert rho.dtype == np.float32 and drho.dtype == np.float32
        gw = (x[:, 1:, :-1] - x[:, 1:, 1:]) - (y[:, 1:, :-1] - y[:, 1:, 1:])          # gw(r, c): [P, r-1, c], r in 1..H-1, c in 0..W-2
        gh = (x[:, 1:, 1:] - x[:, :-1, 1:]) - (y[:, 1:, 1:] - y[:, :-1, 1:])          # gh(r, c): [P, r-1, c-1], r in 1..H-1, c in 1..W-1
        plane_point = rho.astype(np.float64).reshape(P, -1).sum(axis=1)
        plane_gdl = np.abs(gw).astype(np.float64).reshape(P, -1).sum(axis=1) + np.abs(gh).astype(np.float64).reshape(P, -1).sum(axis=1)
        point = plane_point.sum() / (float(P) * H * W)
        gdl = plane_gdl.sum() / (float(P) * (H - 1) * (W - 1))
        sw, sh = _sgn(gw), _sgn(gh)
        t1, t2, t3, t4 = (np.zeros((P, H, W), np.float32) for _ in range(4))
        t1[:, 1:, :-1] = sw                       # [r>=1, c<=W-2] sgn(gw(r, c))
        t2[:, 1:, 1:] = sw                        # [r>=1, c>=1]   sgn(gw(r, c-1))
        t3[:, 1:, 1:] = sh                        # [r>=1, c>=1]   sgn(gh(r, c))
        t4[:, :-1, 1:] = sh                       # [r<=H-2, c>=1] sgn(gh(r+1, c))
        S = ((t1 - t2) + t3) - t4
        cp = 0.5 / (float(P) * H * W)
        cg = 0.5 / (float(P) * (H - 1) * (W - 1))
        grad64 = (drho.astype(np.float64) * cp + S.astype(np.float64) * cg).reshape(pred.shape)
        grad = grad64.astype(np.float32)
    return dict(plane_terms=np.stack([plane_point, plane_gdl], axis=1), point=point, gdl=gdl, loss=point + gdl, grad64=grad64, grad=grad,
                S=S, rho=rho, gw=gw, gh=gh)


KINDS = ('uniform', 'smooth', 'equal', 'wide', 'grid')


def make_pair(kind, shape, seed):
    """Seeded float32 (pred, gt) of ``shape`` [..., H, W]: uniform random in [-1, 1]; a low-frequency pattern plus 2 % noise; pred == gt;
    uniform in [-3, 3] (unclipped); values k / 64 - 1 with k integer in [0, 128], about a third of pred's pixels copied from gt (ties
    d = 0, gw = 0, gh = 0 are frequent, and every term is a multiple of 2^-33 below 2: sums of up to 2^18 of them are exact in float64)."""
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
    elif kind == 'wide':
        pred, gt = rs.uniform(-3, 3, shape), rs.uniform(-3, 3, shape)
    elif kind == 'grid':
        gt = rs.randint(0, 129, shape) / 64.0 - 1.0
        pred = rs.randint(0, 129, shape) / 64.0 - 1.0
        pred = np.where(rs.uniform(0, 1, shape) < 1.0 / 3.0, gt, pred)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(pred, dtype=np.float32), np.ascontiguousarray(gt, dtype=np.float32)
