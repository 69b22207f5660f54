"""The fused step with a learning-rate schedule, a warm-up and decoupled weight decay (include/tai_sepconv.h, ``tai_fused_step_decay``),
restated in numpy and independent of the package.  tests/fused_step_ref.py restates the step without them and stays as it is.

    the schedule, Python floats, for t' = 1 ... n; L the base rate, N the steps the table is built for:
        warm(t')  = t' / W                                   if t' <= W, else 1.0
        constant:   s(t') = 1.0
        step:       s(t') = g ** ((t' - 1) // E)
        cosine:     s(t') = 1.0                              for t' <= W
                    u = min(1.0, (t' - W) / max(1, N - W))
                    s(t') = r + (1.0 - r) * (0.5 * (1.0 + math.cos(math.pi * u)))
        lr(t')    = (L * warm(t')) * s(t')
        step_size[t'] = f32(lr(t') / (1 - beta1**t'))    bc2s[t'] = f32(sqrt(1 - beta2**t'))    decay[t'] = f32(lr(t') * wd)
    per element, single IEEE fp32 operations:
        g1 = (c < 1) ? g * c : g
        m' = m + w1 * (g1 - m)
        v' = b2 * v + (w2 * g1) * g1
        s  = sqrt(v') / bc2s[t'] + eps
        p1 = p - (decay[t'] * p)         for entries whose flag says "decays"; p1 = p for the others
        p' = p1 - step_size[t'] * (m' / s)
        e' = e + wE * (p' - e)
"""
import math

import numpy as np

F = np.float32


def lr(t, L, kind='constant', W=0, E=1, g=1.0, r=0.01, N=1):
    """lr(t') as a Python float."""
    warm = t / W if t <= W else 1.0
    if kind == 'constant':
        s = 1.0
    elif kind == 'step':
        s = g ** ((t - 1) // E)
    elif kind == 'cosine':
        if t <= W:
            s = 1.0
        else:
            u = min(1.0, (t - W) / max(1, N - W))
            s = r + (1.0 - r) * (0.5 * (1.0 + math.cos(math.pi * u)))
    else:
        raise ValueError(kind)
    return (L * warm) * s


def scalars(L, beta1, beta2, n, wd=0.0, **schedule):
    """-> (step_size, bc2s, decay): fp32 arrays, element t' - 1 for step t'."""
    rates = [lr(t, L, **schedule) for t in range(1, n + 1)]
    return (np.array([F(rates[t - 1] / (1 - beta1 ** t)) for t in range(1, n + 1)], F),
            np.array([F(math.sqrt(1 - beta2 ** t)) for t in range(1, n + 1)], F),
            np.array([F(rates[t - 1] * wd) for t in range(1, n + 1)], F))


def step(p, g, m, v, e, c, step_size, bc2s, decay, beta1, beta2, d=None):
    """One step on float32 arrays with the table's scalars of its t' -> (p', m', v', e' or None); ``decay``: decay[t'] for an entry
    whose flag is set, None for the others.  The inputs are left alone."""
    p, g, m, v = (np.asarray(x, F) for x in (p, g, m, v))
    c, step_size, bc2s = F(c), F(step_size), F(bc2s)
    w1, b2, w2, eps = F(1 - beta1), F(beta2), F(1 - beta2), F(1e-8)
    with np.errstate(all='ignore'):
        g1 = g * c if c < 1 else g
        m1 = m + w1 * (g1 - m)
        v1 = b2 * v + (w2 * g1) * g1
        s = np.sqrt(v1) / bc2s + eps
        p1 = p - (F(decay) * p) if decay is not None else p
        p2 = p1 - step_size * (m1 / s)
        e1 = None
        if e is not None:
            e = np.asarray(e, F)
            e1 = e + F(1 - d) * (p2 - e)
    assert p2.dtype == m1.dtype == v1.dtype == F
    return p2, m1, v1, e1
