"""CPU statement of the opt-in bf16 convolution mode (conv_ops.set_conv_precision('bf16')), shared by the tests and
tools/bf16_emulation_study.py: the bf16 rounding of an operand, the layer rule, and the CPU oracle with every eligible
F.conv2d / F.conv_transpose2d fed bf16-rounded operands in float64 (oracle/ itself is not edited: its ``F`` is swapped)."""
import contextlib
import types

import numpy as np
import torch
import torch.nn.functional as F


def bf16_round(x):
    """float64 tensor of x rounded to bf16, nearest even, computed on the float32 bits (independent of torch's own cast);
    every NaN becomes the NaN torch's cast gives (bf16 0xffff), +-Inf stay +-Inf."""
    a = np.ascontiguousarray(x.detach().cpu().float().numpy())
    u = a.view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    nan = np.isnan(a)
    r[nan] = 0xFFFF0000
    out = r.astype(np.uint32).view(np.float32).astype(np.float64)
    return torch.from_numpy(out.reshape(a.shape))


def bf16_ok(Ci, Co, k, padding):
    """conv_ops._bf16_ok, restated: C >= 16 input and K >= 16 output channels, k in {3, 5, 7}, padding k // 2 (stride 1)."""
    return Ci >= 16 and Co >= 16 and k in (3, 5, 7) and padding == k // 2


def _pad(p):
    return p[0] if isinstance(p, (tuple, list)) else p


def conv2d_bf16(x, w, b=None, stride=1, padding=0):
    """F.conv2d of the bf16-rounded operands in float64 (bias unrounded), back in x's dtype"""
    y = F.conv2d(bf16_round(x), bf16_round(w), None if b is None else b.detach().double(), stride=stride, padding=padding)
    return y.to(x.dtype)


def conv_transpose2d_bf16(x, w, b=None, stride=1, padding=0):
    y = F.conv_transpose2d(bf16_round(x), bf16_round(w), None if b is None else b.detach().double(), stride=stride, padding=padding)
    return y.to(x.dtype)


class _Counted(object):
    def __init__(self):
        self.taken, self.kept = [], []


def _emulating_F(count):
    shim = types.ModuleType('F_bf16')
    for name in dir(F):
        if not name.startswith('__'):
            setattr(shim, name, getattr(F, name))

    def conv2d(x, w, b=None, stride=1, padding=0, *a, **kw):
        s, p = stride if isinstance(stride, int) else stride[0], _pad(padding)
        if not a and not kw and s == 1 and w.shape[2] == w.shape[3] and bf16_ok(w.shape[1], w.shape[0], w.shape[2], p):
            count.taken.append(('conv2d', tuple(w.shape)))
            return conv2d_bf16(x, w, b, 1, p)
        count.kept.append(('conv2d', tuple(w.shape)))
        return F.conv2d(x, w, b, stride, padding, *a, **kw)

    def conv_transpose2d(x, w, b=None, stride=1, padding=0, *a, **kw):
        s, p = stride if isinstance(stride, int) else stride[0], _pad(padding)
        if not a and not kw and s == 1 and w.shape[2] == w.shape[3] and bf16_ok(w.shape[0], w.shape[1], w.shape[2], p):
            count.taken.append(('conv_transpose2d', tuple(w.shape)))
            return conv_transpose2d_bf16(x, w, b, 1, p)
        count.kept.append(('conv_transpose2d', tuple(w.shape)))
        return F.conv_transpose2d(x, w, b, stride, padding, *a, **kw)

    shim.conv2d = conv2d
    shim.conv_transpose2d = conv_transpose2d
    return shim


@contextlib.contextmanager
def bf16_oracle():
    """Within the block, oracle.tai_oracle computes every eligible convolution as the bf16 mode does.  Yields a record of the
    layers taken (``.taken``) and left in fp32 (``.kept``)."""
    from oracle import tai_oracle
    count = _Counted()
    saved = tai_oracle.F
    tai_oracle.F = _emulating_F(count)
    try:
        yield count
    finally:
        tai_oracle.F = saved
