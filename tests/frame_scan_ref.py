"""numpy restatement of tai_frame_scan (include/tai_sepconv.h): int64 [n, 4] = (s1, s2, sad, ndiff) per frame."""
import numpy as np


def frame_scan_ref(frames, tol=0):
    v = np.asarray(frames)
    v = v.reshape(v.shape[0], -1).astype(np.int64)
    out = np.zeros((v.shape[0], 4), dtype=np.int64)
    out[:, 0] = v.sum(axis=1)
    out[:, 1] = (v * v).sum(axis=1)
    d = np.abs(v[1:] - v[:-1])
    out[1:, 2] = d.sum(axis=1)
    out[1:, 3] = (d > tol).sum(axis=1)
    return out
