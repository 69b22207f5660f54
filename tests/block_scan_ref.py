"""numpy restatements of tai_block_scan (include/tai_sepconv.h) and of the rule that tells damage from content (restore.damage_runs)."""
import numpy as np


def block_scan_ref(frames, bs, tol=0):
    """uint8 [n, h, w, c] -> int64 [n, Bh, Bw, 4] = (s1, s2, sad, ndiff) over the bytes of each block; ragged edge blocks hold fewer."""
    v = np.asarray(frames).astype(np.int64)
    n, h, w, _ = v.shape
    Bh, Bw = -(-h // bs), -(-w // bs)
    out = np.zeros((n, Bh, Bw, 4), dtype=np.int64)
    for by in range(Bh):
        for bx in range(Bw):
            b = v[:, by * bs:(by + 1) * bs, bx * bs:(bx + 1) * bs].reshape(n, -1)
            out[:, by, bx, 0] = b.sum(axis=1)
            out[:, by, bx, 1] = (b * b).sum(axis=1)
            d = np.abs(b[1:] - b[:-1])
            out[1:, by, bx, 2] = d.sum(axis=1)
            out[1:, by, bx, 3] = (d > tol).sum(axis=1)
    return out


def damage_runs_ref(raw, max_T):
    """bool [n, Bh, Bw] -> bool [n, Bh, Bw]: frame i of a block position is damage iff it is raw-flagged and the maximal run of flagged
    frames around it has at most max_T frames and contains neither frame 0 nor frame n - 1.  Stated per frame, not per run."""
    raw = np.asarray(raw, dtype=bool)
    n = raw.shape[0]
    out = np.zeros_like(raw)
    for i in range(n):
        for by in range(raw.shape[1]):
            for bx in range(raw.shape[2]):
                if not raw[i, by, bx]:
                    continue
                a = b = i
                while a > 0 and raw[a - 1, by, bx]:
                    a -= 1
                while b < n - 1 and raw[b + 1, by, bx]:
                    b += 1
                out[i, by, bx] = b - a + 1 <= max_T and a > 0 and b < n - 1
    return out
