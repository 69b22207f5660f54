"""The fused optimizer step's definition (include/tai_sepconv.h, ``tai_fused_step`` / ``tai_step_verdict``), restated in numpy and
independent of the package: numpy's float32 operations are single IEEE operations rounded to nearest even, which is the definition.

    scalars, for t' = 1 ... n, from Python floats rounded to fp32:
        step_size[t'] = f32(lr / (1 - beta1**t'))     bc2s[t'] = f32(sqrt(1 - beta2**t'))
        w1 = f32(1 - beta1)  b2 = f32(beta2)  w2 = f32(1 - beta2)  eps = f32(1e-8)  wE = f32(1 - d)
    per element, when the verdict is not "skipped":
        g1 = (c < 1) ? g * c : g
        m' = m + w1 * (g1 - m)
        v' = b2 * v + (w2 * g1) * g1
        s  = sqrt(v') / bc2s[t'] + eps
        p' = p - step_size[t'] * (m' / s)
        e' = e + wE * (p' - e)
    the verdict: nonfinite > 0 -> skipped; else c64 = X / (sqrt(total) + 1e-6) in float64, c = 1 if c64 >= 1 else f32(c64),
    clipped when c < 1.
"""
import math

import numpy as np

OK, CLIPPED, SKIPPED = 0, 1, 2
F = np.float32


def scalars(lr, beta1, beta2, n):
    """-> (step_size, bc2s): fp32 arrays, element t' - 1 for step t'."""
    return (np.array([F(lr / (1 - beta1 ** t)) for t in range(1, n + 1)], F),
            np.array([F(math.sqrt(1 - beta2 ** t)) for t in range(1, n + 1)], F))


def verdict(total, nonfinite, max_norm):
    """-> (verdict, c as numpy.float32)."""
    if nonfinite > 0:
        return SKIPPED, F(1)
    if max_norm is None:
        return OK, F(1)
    c64 = float(max_norm) / (math.sqrt(float(total)) + 1e-6)
    c = F(1) if c64 >= 1.0 else F(c64)
    return (CLIPPED if c < F(1) else OK), c


def step(p, g, m, v, e, c, t, lr, beta1, beta2, d=None):
    """One step t' = ``t`` on float32 arrays -> (p', m', v', e' or None); the inputs are left alone."""
    p, g, m, v = (np.asarray(x, F) for x in (p, g, m, v))
    c = F(c)
    step_size, bc2s = F(lr / (1 - beta1 ** t)), F(math.sqrt(1 - beta2 ** t))
    w1, b2, w2, eps = F(1 - beta1), F(beta2), F(1 - beta2), F(1e-8)
    with np.errstate(all='ignore'):
        g1 = g * c if c < 1 else g
        m1 = m + w1 * (g1 - m)
        v1 = b2 * v + (w2 * g1) * g1
        s = np.sqrt(v1) / bc2s + eps
        p1 = p - step_size * (m1 / s)
        e1 = None
        if e is not None:
            e = np.asarray(e, F)
            e1 = e + F(1 - d) * (p1 - e)
    assert p1.dtype == m1.dtype == v1.dtype == F
    return p1, m1, v1, e1


def ema_recurrence(e0, weights, d):
    """The average after the recorded weights ``weights[0], weights[1], ...`` from the start value e0."""
    e = np.asarray(e0, F)
    for p in weights:
        with np.errstate(all='ignore'):
            e = e + F(1 - d) * (np.asarray(p, F) - e)
    return e
