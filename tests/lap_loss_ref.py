"""numpy restatement of the Laplacian-pyramid loss as include/tai_sepconv.h defines it for tai_lap_loss, operation for operation (numpy's
element-wise float64 arithmetic is one IEEE operation per written operation: no contraction).  The pyramid is built with element-wise
operations in the written order; the adjoints are products with the operators' dense matrices, which is allowed because every value in
them is a dyadic rational that float64 holds exactly, so the order of those sums does not matter.  Shared by the CPU and the GPU tests;
the inputs it makes are seeded."""
import numpy as np

K5 = (1.0 / 16.0, 4.0 / 16.0, 6.0 / 16.0, 4.0 / 16.0, 1.0 / 16.0)
MAX_LEVELS = 6


def sizes(H, W, levels):
    """[(H_l, W_l)] for l = 0..levels-1: each level is the ceiling of half the one below."""
    out = [(H, W)]
    for _ in range(levels - 1):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def _reduce_axis(g, axis):
    """One pass of D along ``axis``: out[i] = sum_{a=0..4} k[a] g[clamp(2i + a - 2)], accumulated left to right."""
    n = g.shape[axis]
    m = (n + 1) // 2
    acc = None
    for a in range(5):
        idx = np.clip(2 * np.arange(m) + a - 2, 0, n - 1)
        term = K5[a] * np.take(g, idx, axis=axis)
        acc = term if acc is None else acc + term
    return acc


def reduce(g):
    """D: [P, h, w] -> [P, ceil(h/2), ceil(w/2)], rows (axis 1) first, then columns."""
    return _reduce_axis(_reduce_axis(g, 1), 2)


def _expand_axis(g, n, axis):
    """One pass of U along ``axis``, from m = ceil(n/2) entries to n."""
    m = g.shape[axis]
    i = np.arange(m)
    lo, hi = np.clip(i - 1, 0, m - 1), np.clip(i + 1, 0, m - 1)
    centre, before, after = g, np.take(g, lo, axis=axis), np.take(g, hi, axis=axis)
    even = (before / 8.0 + (6.0 * centre) / 8.0) + after / 8.0
    odd = centre / 2.0 + after / 2.0
    shape = list(g.shape)
    shape[axis] = n
    out = np.empty(shape, np.float64)
    sl = [slice(None)] * g.ndim
    sl[axis] = slice(0, n, 2)
    out[tuple(sl)] = even
    sl[axis] = slice(1, n, 2)
    src = [slice(None)] * g.ndim
    src[axis] = slice(0, n // 2)
    out[tuple(sl)] = odd[tuple(src)]
    return out


def expand(g, h, w):
    """U: [P, ceil(h/2), ceil(w/2)] -> [P, h, w], rows (axis 1) first, then columns."""
    return _expand_axis(_expand_axis(g, h, 1), w, 2)


def _reduce_matrix(n):
    m = (n + 1) // 2
    M = np.zeros((m, n))
    for i in range(m):
        for a in range(5):
            M[i, min(max(2 * i + a - 2, 0), n - 1)] += K5[a]
    return M


def _expand_matrix(n):
    m = (n + 1) // 2
    M = np.zeros((n, m))
    for f in range(n):
        i = f // 2
        if f % 2 == 0:
            M[f, max(i - 1, 0)] += 1.0 / 8.0
            M[f, i] += 6.0 / 8.0
            M[f, min(i + 1, m - 1)] += 1.0 / 8.0
        else:
            M[f, i] += 0.5
            M[f, min(i + 1, m - 1)] += 0.5
    return M


def _sign(v):
    """-1, 0, 1 with sign(0) = +0; a NaN stays a NaN."""
    return np.where(v > 0, 1.0, np.where(v < 0, -1.0, np.where(v == 0, 0.0, v)))


def lap_loss_ref(pred, gt, levels):
    """pred, gt: arrays [..., H, W] of one shape.  float32 inputs follow the definition (x = (pred + 1) / 2 and d = x - y in fp32);
    float64 inputs take the same operations in float64 (the form the torch path takes for float64 tensors).  -> dict: laplacians (list
    of [P, H_l, W_l]), plane_terms [P, levels] (the sums of |L_l|), terms [levels], loss, t0 [P, H, W], grad64 and grad (float32, pred's
    shape)."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    assert pred.shape == gt.shape and pred.dtype == gt.dtype and pred.dtype in (np.float32, np.float64)
    H, W = pred.shape[-2:]
    assert 1 <= levels <= MAX_LEVELS and min(H, W) >= 2 ** (levels - 1)
    one, two = pred.dtype.type(1), pred.dtype.type(2)
    with np.errstate(all='ignore'):
        d = ((pred + one) / two - (gt + one) / two).astype(np.float64).reshape(-1, H, W)
        P = d.shape[0]
        dims = sizes(H, W, levels)
        G = [d]
        for l in range(1, levels):
            G.append(reduce(G[-1]))
        lap = [G[l] - expand(G[l + 1], *dims[l]) for l in range(levels - 1)] + [G[levels - 1]]
        plane_terms = np.stack([np.abs(L).sum(axis=(1, 2)) for L in lap], axis=1)
        count = (float(P) * float(H)) * float(W)
        terms = np.array([(2.0 ** l * sum(plane_terms[p, l] for p in range(P))) / count for l in range(levels)])
        loss = 0.0
        for l in range(levels):
            loss = loss + terms[l]
        s = [2.0 ** l * _sign(lap[l]) for l in range(levels)]
        r = [s[0]]
        for l in range(1, levels):
            Ur, Uc = _expand_matrix(dims[l - 1][0]), _expand_matrix(dims[l - 1][1])
            r.append(s[l] - np.einsum('fi,pfg,gj->pij', Ur, s[l - 1], Uc))
        t = r[levels - 1]
        for l in range(levels - 2, -1, -1):
            Dr, Dc = _reduce_matrix(dims[l][0]), _reduce_matrix(dims[l][1])
            t = r[l] + np.einsum('if,pij,jg->pfg', Dr, t, Dc)
        grad64 = ((t * 0.5) / count).reshape(pred.shape)
    return dict(laplacians=lap, plane_terms=plane_terms, terms=terms, loss=float(loss), t0=t, grad64=grad64,
                grad=grad64.astype(np.float32), level_pixels=[h * w for h, w in dims])


KINDS = ('noise', 'smooth', 'equal', 'offset', 'impulse')


def make_pair(kind, shape, seed):
    """Seeded float32 (pred, gt) of ``shape`` [..., H, W]: uniform noise in [-1, 1]; a smooth pattern plus 2 % noise; pred == gt; gt plus
    a constant; gt plus one impulse per plane."""
    rs = np.random.RandomState(seed)
    H, W = shape[-2:]
    lead = tuple(shape[:-2])
    if kind == 'noise':
        pred, gt = rs.uniform(-1, 1, shape), rs.uniform(-1, 1, shape)
    elif kind == 'smooth':
        r, c = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        phase = rs.uniform(0, 6.28, lead + (1, 1))
        gt = 0.6 * np.sin(r / 9.0 + phase) * np.cos(c / 7.0 - phase) + 0.1
        pred = gt + 0.02 * rs.standard_normal(shape)
    elif kind == 'equal':
        gt = rs.uniform(-1, 1, shape)
        pred = gt.copy()
    elif kind == 'offset':
        # a grid of 1/64 steps keeps (gt + 0.25 + 1) / 2 - (gt + 1) / 2 one constant in fp32
        gt = np.round(rs.uniform(-0.5, 0.5, shape) * 64.0) / 64.0
        pred = gt + 0.25
    elif kind == 'impulse':
        gt = np.round(rs.uniform(-0.5, 0.5, shape) * 64.0) / 64.0
        pred = gt.copy().reshape(-1, H, W)
        for p in range(pred.shape[0]):
            pred[p, rs.randint(H), rs.randint(W)] += 0.5
        pred = pred.reshape(shape)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(pred, dtype=np.float32), np.ascontiguousarray(gt, dtype=np.float32)
