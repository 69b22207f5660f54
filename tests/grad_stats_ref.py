"""The definition of ``tai_grad_stats`` (include/tai_sepconv.h, csrc/grad_stats.hip.inc), restated in numpy from the header's text: what
pins the kernel and the host half of ``grad_guard.grad_stats``.  It shares no code with either.

    An entry x[0..n) is cut into segments of 16384 elements.  An element that is NaN or +-Inf adds 1 to `nonfinite` and contributes
    nothing else; a finite one contributes q = (double)x * (double)x to the sum and |x| to the maximum.  A segment has 1024 float64
    accumulators, +0.0 at first; accumulator j adds, in increasing i, the q of the elements with segment-relative index i = j (mod 1024);
    then for d = 1, 2, 4, ..., 512: a[j] <- a[j] + a[j xor d] for all j at once; the segment sum is the value every a[j] ends with.
    sumsq of the entry = the segment sums added one by one in segment order from +0.0; the table's total = the entries' sumsq added one
    by one in table order from +0.0.  The clip coefficient: norm = sqrt(total) in float64, c64 = X / (norm + 1e-6), c = 1 if c64 >= 1 else
    float32(c64); with a non-finite element nothing is scaled (c = 1).
"""
import math

import numpy as np

SEGMENT = 16384
ACCUMULATORS = 1024


def as_floats(entry):
    if hasattr(entry, 'detach'):
        entry = entry.detach().cpu().contiguous().numpy()
    a = np.ascontiguousarray(entry).reshape(-1)
    assert a.dtype == np.float32
    return a


def segment_sum(x):
    """The sum of one segment (at most 16384 float32 values): 1024 accumulators filled in index order, then the butterfly."""
    assert x.size <= SEGMENT
    a = np.zeros(ACCUMULATORS, np.float64)
    ok = np.isfinite(x)
    for start in range(0, x.size, ACCUMULATORS):                 # element start + j goes to accumulator j: increasing i per accumulator
        piece = x[start:start + ACCUMULATORS]
        d = piece.astype(np.float64)
        q = d * d
        keep = ok[start:start + ACCUMULATORS]
        idx = np.nonzero(keep)[0]
        a[idx] = a[idx] + q[idx]                                 # (non-finite elements are left out, not added as anything)
    d = 1
    while d <= 512:
        partner = np.arange(ACCUMULATORS) ^ d
        a = a + a[partner]
        d *= 2
    assert np.all(a == a[0])
    return a[0]


def entry_stats(entry):
    """-> (sumsq float64, maxabs float32, nonfinite int)"""
    x = as_floats(entry)
    ok = np.isfinite(x)
    total = np.float64(0.0)
    for start in range(0, x.size, SEGMENT):
        total = total + segment_sum(x[start:start + SEGMENT])
    biggest = np.float32(0.0)
    if ok.any():
        biggest = np.abs(x[ok]).max().astype(np.float32)
    return total, biggest, int(x.size - ok.sum())


def table_stats(entries):
    """-> (list of per-entry (sumsq, maxabs, nonfinite), (total sumsq, maxabs, nonfinite))"""
    per = [entry_stats(e) for e in entries]
    total = np.float64(0.0)
    for s, _, _ in per:
        total = total + s
    return per, (total, max([np.float32(0.0)] + [m for _, m, _ in per]), sum(b for _, _, b in per))


def coefficient(total_sumsq, nonfinite, max_norm):
    """1.0 (a Python float: do not scale) or the numpy.float32 the gradients are multiplied by."""
    if nonfinite > 0:
        return 1.0
    c64 = max_norm / (math.sqrt(total_sumsq) + 1e-6)
    if c64 >= 1.0:
        return 1.0
    return np.float32(c64)
