"""A guard around the optimizer steps (``train.py --guard [--clip_grad_norm X] [--guard_patience N]``): the norm of the generator's and of
the discriminator's gradients, clipping to a norm, and no step at all when a gradient holds a NaN or an Inf.

``grad_stats(tensors)`` reads a table of fp32 tensors where they live, in one launch (``tai_grad_stats``, csrc/grad_stats.hip.inc), and
brings back per tensor and for the table: the sum of squares (float64), the largest magnitude (float32), the number of non-finite
elements.  The sum is a FIXED-ORDER one, so that a clipped run stays inside the bit-exact resume contract (run_state.py):
    an entry is cut into segments of 16384 elements; NaN / +-Inf count as non-finite and contribute nothing else, a finite x contributes
    (double)x * (double)x; a segment has 1024 float64 accumulators, accumulator j adds the elements with segment-relative index
    i = j (mod 1024) in increasing i, then a[j] <- a[j] + a[j xor d] for d = 1, 2, ..., 512; an entry's sum adds its segment sums in
    order, the table's total adds the entries' sums in order, both from +0.0.
Tensors that live on the host are summed here with numpy by the same definition: the result is the same number wherever they live.

The clip coefficient is computed on the host from the total the read brought back (``clip_coefficient``): norm = sqrt(total) in float64,
c64 = X / (norm + 1e-6) (the formula of ``torch.nn.utils.clip_grad_norm_``), c = 1 if c64 >= 1 else float32(c64); the gradients are
multiplied by c (``tai_grad_scale``, one fp32 rounding per element) only when c < 1 and nothing is non-finite.

``GradGuard`` keeps the verdict per optimizer (ok / clipped / skipped), the counters and the last norms.  A skipped update is the update
without that optimizer's step: parameters, ``exp_avg``, ``exp_avg_sq`` and Adam's ``step`` stay exactly as they were.
"""
import math

import numpy as np
import torch

from . import parallel, run_state

SEG = 16384                     # elements per segment: a constant of the definition (csrc/grad_stats.hip.inc), not a tuning knob
LANES = 1024                    # accumulators per segment
OK, CLIPPED, SKIPPED = 0, 1, 2
VERDICTS = ('ok', 'clipped', 'skipped')


class GuardGaveUp(RuntimeError):
    """``guard_patience`` consecutive updates had a step skipped: the run is not going to recover by itself."""


class _Buffers(object):
    """Device buffers of one table shape, kept between calls: two launches per update allocate nothing after the first."""

    def __init__(self, n_entries, n_segments, device):
        from . import _native
        nbytes = _native.lib().tai_grad_stats_workspace_bytes(n_entries, n_segments)
        if nbytes < 0:
            raise ValueError('grad stats: bad table (%d entries, %d segments)' % (n_entries, n_segments))
        self.table = torch.empty(n_entries, 4, dtype=torch.int64, device=device)
        self.workspace = torch.empty(nbytes // 8 + 2, dtype=torch.int64, device=device)            # (torch allocations are 256-byte aligned)
        # sumsq (float64), nonfinite (int64), maxabs (float32), n_entries + 1 of each, in ONE buffer: one device-to-host read
        self.result = torch.zeros(5 * (n_entries + 1), dtype=torch.int32, device=device)
        self.rows = None        # the host rows the device table holds


_buffers = {}


def _check(tensors):
    tensors = [t.detach() for t in tensors]
    for t in tensors:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError('grad stats: an entry must be a contiguous float32 tensor, found %s %s' % (t.dtype, tuple(t.shape)))
    if not tensors:
        raise ValueError('grad stats: an empty table')
    on_device = [t.is_cuda for t in tensors]
    if any(on_device) and not all(on_device):
        raise ValueError('grad stats: the entries of a table live either all on the device or all on the host')
    return tensors, all(on_device)


def _segment_sums_host(x):
    """(segment sums, maxabs, nonfinite) of a float32 array by the definition, with numpy."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    finite = np.isfinite(x)
    bad = int(x.size - np.count_nonzero(finite))
    mx = np.float32(np.max(np.abs(x[finite]))) if x.size > bad else np.float32(0)
    n_seg = -(-x.size // SEG)
    q = np.zeros(n_seg * SEG, np.float64)
    q[:x.size] = np.where(finite, x, np.float32(0)).astype(np.float64)
    q *= q
    acc = np.zeros((n_seg, LANES), np.float64)
    for row in range(SEG // LANES):
        acc += q.reshape(n_seg, SEG // LANES, LANES)[:, row]
    j = np.arange(LANES)
    d = 1
    while d < LANES:
        acc = acc + acc[:, j ^ d]
        d *= 2
    return acc[:, 0], mx, bad


def _stats_host(tensors):
    n = len(tensors)
    sumsq, maxabs, nonfinite = np.zeros(n + 1, np.float64), np.zeros(n + 1, np.float32), np.zeros(n + 1, np.int64)
    for t, x in enumerate(tensors):
        seg, maxabs[t], nonfinite[t] = _segment_sums_host(x.numpy() if x.numel() else np.zeros(0, np.float32))
        e = np.float64(0)
        for s in seg:
            e = e + s
        sumsq[t] = e
    total = np.float64(0)
    for e in sumsq[:n]:
        total = total + e
    sumsq[n], maxabs[n], nonfinite[n] = total, (maxabs[:n].max() if n else 0), nonfinite[:n].sum()
    return sumsq, maxabs, nonfinite


def _device_table(tensors):
    rows, device, n_segments = run_state.build_table(tensors, SEG)
    key = (device, rows.shape[0], n_segments)
    if key not in _buffers:
        _buffers[key] = _Buffers(rows.shape[0], n_segments, device)
    bufs = _buffers[key]
    if bufs.rows is None or not np.array_equal(bufs.rows, rows):        # gradients keep their addresses from update to update
        bufs.table.copy_(torch.from_numpy(rows))                         # pageable memory: the copy has left `rows` when it returns
        bufs.rows = rows
    return bufs, rows, device, n_segments


def grad_stats(tensors, blocks=0):
    """-> ((sumsq float64 [n], maxabs float32 [n], nonfinite int64 [n]), (total sumsq, maxabs, nonfinite)) of a list of contiguous
    float32 tensors, all on one device (one launch, one read that synchronises) or all on the host (numpy).  ``blocks``: workgroups of
    the launch, 0 = the library's choice; the results do not depend on it."""
    tensors, on_device = _check(tensors)
    n = len(tensors)
    if not on_device:
        sumsq, maxabs, nonfinite = _stats_host(tensors)
    elif not any(t.numel() for t in tensors):
        sumsq, maxabs, nonfinite = np.zeros(n + 1, np.float64), np.zeros(n + 1, np.float32), np.zeros(n + 1, np.int64)
    else:
        from . import _native
        bufs, rows, device, n_segments = _device_table(tensors)
        with torch.cuda.device(device):
            base = bufs.result.data_ptr()
            _native.launch('tai_grad_stats', device, bufs.table, rows.ctypes.data, n, n_segments, int(blocks), bufs.workspace,
                           base, base + 16 * (n + 1), base + 8 * (n + 1))
            raw = bufs.result.cpu().numpy()                              # synchronises
        sumsq = raw[:2 * (n + 1)].view(np.float64)
        nonfinite = raw[2 * (n + 1):4 * (n + 1)].view(np.int64)
        maxabs = raw[4 * (n + 1):].view(np.float32)
    return (sumsq[:n], maxabs[:n], nonfinite[:n]), (float(sumsq[n]), float(maxabs[n]), int(nonfinite[n]))


def scale_(tensors, c, blocks=0):
    """x <- x * float32(c) in place over a list of contiguous float32 tensors (one launch, asynchronous; numpy on the host)."""
    tensors, on_device = _check(tensors)
    c = np.float32(c)
    if not np.isfinite(c):
        raise ValueError('grad scale: the factor must be finite, found %r' % c)
    if not on_device:
        for t in tensors:
            if t.numel():
                a = t.numpy()
                np.multiply(a, c, out=a)
        return
    if not any(t.numel() for t in tensors):
        return
    from . import _native
    bufs, rows, device, n_segments = _device_table(tensors)
    _native.launch('tai_grad_scale', device, bufs.table, rows.ctypes.data, len(tensors), n_segments, float(c), int(blocks), None)


def clip_coefficient(total_sumsq, nonfinite, max_norm):
    """The factor the gradients are multiplied by: 1.0 = leave them alone, otherwise a numpy.float32 below 1."""
    if max_norm is None or nonfinite > 0:
        return 1.0
    norm = math.sqrt(float(total_sumsq))
    c64 = float(max_norm) / (norm + 1e-6)
    return 1.0 if c64 >= 1.0 else np.float32(c64)


class GradGuard(object):
    """The guard of one training environment.  ``check(which, named_parameters)`` is called between a backward pass (and its gradient
    all-reduce) and the optimizer's step and says whether the step may be made; ``end_update()`` closes the update."""

    def __init__(self, clip_grad_norm=None, patience=8):
        if clip_grad_norm is not None and not (clip_grad_norm > 0 and math.isfinite(clip_grad_norm)):
            raise ValueError('--clip_grad_norm must be a positive number, found %r' % (clip_grad_norm,))
        if patience < 1:
            raise ValueError('--guard_patience must be at least 1, found %r' % (patience,))
        self.clip_grad_norm = None if clip_grad_norm is None else float(clip_grad_norm)
        self.patience = int(patience)
        self.skipped = {'G': 0, 'D': 0}
        self.consecutive = 0
        self.norm = {'G': 0.0, 'D': 0.0}            # of the last update, before clipping
        self.coefficient = {'G': 1.0, 'D': 1.0}
        self.verdict = {'G': OK, 'D': OK}
        self.message = ''
        self._skipped_in_update = False

    # ---- counters: what travels in a snapshot's run_state and enters the state digest
    def counters(self):
        return {'skipped_G': self.skipped['G'], 'skipped_D': self.skipped['D'], 'consecutive': self.consecutive}

    def load_counters(self, counters):
        self.skipped = {'G': int(counters['skipped_G']), 'D': int(counters['skipped_D'])}
        self.consecutive = int(counters['consecutive'])

    @property
    def skipped_G(self):
        return self.skipped['G']

    @property
    def skipped_D(self):
        return self.skipped['D']

    @staticmethod
    def agree(verdict):
        """The worst verdict of all ranks (one integer, max-reduced): no rank steps alone."""
        if parallel.world_size() == 1:
            return int(verdict)
        import torch.distributed as dist
        on_gpu = dist.get_backend() == 'nccl'
        t = torch.tensor([int(verdict)], dtype=torch.int32, device=torch.device('cuda', torch.cuda.current_device()) if on_gpu else 'cpu')
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return int(t.item())

    def judge(self, which, names, per_entry, totals):
        """The decision for optimizer ``which`` ('G' or 'D') from the statistics of its gradients -> (verdict, coefficient).  No GPU work."""
        total, _, bad = totals
        self.norm[which] = math.sqrt(total)
        c = clip_coefficient(total, bad, self.clip_grad_norm)
        mine = SKIPPED if bad > 0 else (CLIPPED if c < 1.0 else OK)
        if mine == SKIPPED:
            first = int(np.flatnonzero(np.asarray(per_entry[2]) > 0)[0])
            self.message = '%s: %d non-finite gradient element(s) in %s (%d in %d parameter(s) in all)' % (
                which, int(per_entry[2][first]), names[first], bad, int(np.count_nonzero(np.asarray(per_entry[2]) > 0)))
        verdict = self.agree(mine)
        if verdict == SKIPPED and mine != SKIPPED:
            self.message = '%s: non-finite gradients on another rank' % which
        self.verdict[which], self.coefficient[which] = verdict, (c if verdict == CLIPPED else 1.0)
        if verdict == SKIPPED:
            self.skipped[which] += 1
            self._skipped_in_update = True
        return verdict, self.coefficient[which]

    def check(self, which, named_parameters):
        """Statistics over the parameters that have a gradient, clip if asked -> True if the optimizer may step."""
        named = [(n, p.grad) for n, p in named_parameters if p.grad is not None]
        if not named:
            return True
        grads = [g for _, g in named]
        per_entry, totals = grad_stats(grads)
        verdict, c = self.judge(which, [n for n, _ in named], per_entry, totals)
        if verdict == CLIPPED and c < 1.0:
            scale_(grads, c)
        return verdict != SKIPPED

    def end_update(self):
        """After the last optimizer of an update.  Raises GuardGaveUp after ``patience`` consecutive updates with a skipped step."""
        self.consecutive = self.consecutive + 1 if self._skipped_in_update else 0
        self._skipped_in_update = False
        if self.consecutive >= self.patience:
            raise GuardGaveUp('%d consecutive updates had an optimizer step skipped (--guard_patience %d); the last one: %s'
                              % (self.consecutive, self.patience, self.message))

    def log_suffix(self):
        return ' gnorm_G=%.6e gnorm_D=%.6e skipped=%d' % (self.norm['G'], self.norm['D'], self.skipped['G'] + self.skipped['D'])


def first_nonfinite(named_tensors):
    """(name, count) of the first float32 tensor of ``named_tensors`` that holds a non-finite element, or None: what ``env.save`` asks
    before it writes a snapshot."""
    named = [(n, t.detach().contiguous()) for n, t in named_tensors if torch.is_tensor(t) and t.dtype == torch.float32]
    if not named:
        return None
    (_, _, bad), totals = grad_stats([t for _, t in named])
    if totals[2] == 0:
        return None
    first = int(np.flatnonzero(bad > 0)[0])
    return named[first][0], int(bad[first])
