"""numpy restatements of tai_damage_composite (include/tai_sepconv.h) and of the tap tables it is given (restore.tap_tables)."""
import numpy as np


def tap_tables_ref(n_in, n_out):
    """(i0, i1) int32 [n_out]: the source indices data.resize_bilinear multiplies by a non-zero weight at output index i, one index at a
    time (weights 1 - f and f of clip(floor(s)) and clip(floor(s) + 1), s = (i + 0.5) * (n_in / n_out) - 0.5 in float64)."""
    i0, i1 = [], []
    for i in range(n_out):
        s = (np.float64(i) + 0.5) * (n_in / float(n_out)) - 0.5
        fl = int(np.floor(s))
        a, b = min(max(fl, 0), n_in - 1), min(max(fl + 1, 0), n_in - 1)
        i0.append(a)
        i1.append(b if s - np.floor(s) > 0 else a)
    return np.array(i0, dtype=np.int32), np.array(i1, dtype=np.int32)


def u_ref(x):
    """tai_frames_to_uint8's u in fp32: uint8(trunc(255 * ((clip(x, -1, 1) + 1) / 2))), NaN -> 0."""
    x = np.asarray(x, dtype=np.float32)
    c = np.where(np.isnan(x), np.float32(-1), np.minimum(np.maximum(x, np.float32(-1)), np.float32(1))).astype(np.float32)
    unit = ((c + np.float32(1)) / np.float32(2)).astype(np.float32)
    return (unit * np.float32(255)).astype(np.float32).astype(np.int64)


def core_ref(blocks, taps, bs, h, w):
    """D bool [h, w]: a model pixel is damaged when a source pixel its resize reads with non-zero weight lies in a damaged block."""
    r0, r1, c0, c1 = (np.asarray(t).astype(np.int64) for t in taps)
    blocks = np.asarray(blocks) != 0
    D = np.zeros((h, w), dtype=bool)
    for r in (r0, r1):
        for c in (c0, c1):
            D |= blocks[(r[:h] // bs)[:, None], (c[:w] // bs)[None, :]]
    return D


def alpha_ref(D, feather):
    """A int [h, w] = max(0, R - Chebyshev distance to the nearest D = 1 inside the frame), R = feather + 1.  The pixels within Chebyshev
    distance d of the core are the core grown d times by one pixel in all eight directions; nothing lies outside the frame."""
    R = feather + 1
    h, w = D.shape
    grown = np.asarray(D, dtype=bool)
    A = np.where(grown, R, 0).astype(np.int64)
    for d in range(1, R):
        p = np.zeros((h + 2, w + 2), dtype=bool)
        p[1:-1, 1:-1] = grown
        grown = np.zeros((h, w), dtype=bool)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                grown |= p[dy:dy + h, dx:dx + w]
        A = np.maximum(A, np.where(grown, R - d, 0))
    return A


def damage_composite_ref(pred, src, blocks, taps, bs, h, w, feather, reverse_channels):
    """pred, src fp32 [C, Hs, Ws]; blocks [Bh, Bw]; taps (r0, r1, c0, c1) -> uint8 [h, w, C]."""
    R = feather + 1
    A = alpha_ref(core_ref(blocks, taps, bs, h, w), feather)[:, :, None]
    order = slice(None, None, -1) if reverse_channels else slice(None)
    P = u_ref(np.asarray(pred)[order, :h, :w]).transpose(1, 2, 0)
    S = u_ref(np.asarray(src)[order, :h, :w]).transpose(1, 2, 0)
    return ((2 * (A * P + (R - A) * S) + R) // (2 * R)).astype(np.uint8)
