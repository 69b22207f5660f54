"""The augmented clip pipeline restated in numpy (include/tai_sepconv.h, at tai_clip_from_frames_aug): what data._ClipReader.clip (host)
and tai_clip_from_frames_aug (device) must both give, bit for bit.  Nothing here calls the package: the resize, the crop window, the
level tables and the assembly of a clip are written out again from the definition."""
import numpy as np

GRAY_BGR = (np.float32(0.1140), np.float32(0.5870), np.float32(0.2989))


def crop_window(h, w, smin, u_scale, u_top, u_left):
    s = np.float64(smin) + np.float64(u_scale) * (np.float64(1.0) - np.float64(smin))
    ch, cw = max(1, int(np.floor(s * h))), max(1, int(np.floor(s * w)))
    top = min(int(np.floor(np.float64(u_top) * (h - ch + 1))), h - ch)
    left = min(int(np.floor(np.float64(u_left) * (w - cw + 1))), w - cw)
    return top, left, ch, cw


def resize(frame, H, W):
    """[h, w, 3] uint8 -> [H, W, 3] uint8: half-pixel centres, taps clamped to the array's edges, fp64 with every product and sum
    rounded on its own, round half up.  Written per axis with explicit loops over the taps' arrays (no shortcut for equal sizes)."""
    h, w = frame.shape[:2]

    def taps(n_out, n_in):
        i = np.arange(n_out, dtype=np.float64)
        src = (i + 0.5) * (np.float64(n_in) / np.float64(n_out)) - 0.5
        fl = np.floor(src)
        i0 = fl.astype(np.int64)
        return np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), src - fl

    y0, y1, fy = taps(H, h)
    x0, x1, fx = taps(W, w)
    f = frame.astype(np.float64)
    gx, gy = (1.0 - fx)[None, :, None], (1.0 - fy)[:, None, None]
    fx, fy = fx[None, :, None], fy[:, None, None]
    a, b, c, d = f[y0][:, x0], f[y0][:, x1], f[y1][:, x0], f[y1][:, x1]
    top = a * gx + b * fx
    bot = c * gx + d * fx
    v = top * gy + bot * fy
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def level_table(gamma, gain, offset):
    """float32 [4, 256] of one frame: float64, rounded once, then the range map and the gray products in float32."""
    x = np.arange(256, dtype=np.float64) / 255.0
    if gamma != 1.0:
        x = x ** np.float64(gamma)
    x = (x - 0.5) * np.float64(gain) + 0.5 + np.float64(offset)
    x = np.minimum(np.maximum(x, 0.0), 1.0)
    row0 = x.astype(np.float32) * np.float32(2) - np.float32(1)
    return np.stack([row0] + [k * row0 for k in GRAY_BGR]).astype(np.float32)


NEUTRAL = level_table(1.0, 1.0, 0.0)


def clip(frames, c_dim, size, pad, window, mirror, vflip, gamma=1.0, gain=1.0, offset=0.0, flicker=None):
    """frames: uint8 [T, h, w, 3] RGB in PLAYBACK order -> float32 [T, C, H + pad_h, W + pad_w].  ``flicker``: None or T offsets, the one
    of playback position t added to ``offset`` in float64 before the table of frame t is formed."""
    T = frames.shape[0]
    (H, W), (ph, pw) = size, pad
    top, left, ch, cw = window
    C = 1 if c_dim == 1 else 3
    pad_value = NEUTRAL[0, 0] if C == 3 else np.float32(np.float32(NEUTRAL[1, 0] + NEUTRAL[2, 0]) + NEUTRAL[3, 0])
    out = np.full((T, C, H + ph, W + pw), pad_value, dtype=np.float32)
    for t in range(T):
        tab = level_table(gamma, gain, offset if flicker is None else np.float64(offset) + np.float64(flicker[t]))
        q = resize(frames[t][top:top + ch, left:left + cw], H, W)[:, :, ::-1]               # BGR
        if vflip:
            q = q[::-1]
        if mirror:
            q = q[:, ::-1]
        q = q.astype(np.int64)
        if C == 3:
            out[t, :, :H, :W] = np.transpose(tab[0][q], (2, 0, 1))
        else:
            out[t, 0, :H, :W] = (tab[1][q[..., 0]] + tab[2][q[..., 1]]) + tab[3][q[..., 2]]
    return out
