"""The optimizer step as one HIP launch decided on the device (``train.py --fused_step [--ema_decay d]``): clip scaling, the Adam
update and the exponential moving average (EMA) of the generator's weights in ``tai_fused_step``, behind a verdict (ok / clipped /
skipped) that ``tai_step_verdict`` has put into device memory from ``tai_grad_stats``' results (csrc/fused_step.hip.inc).  The host
launches and goes on: it does not wait between ``backward()`` and the step.

The definition (include/tai_sepconv.h; restated in numpy in tests/fused_step_ref.py).  Every operation is one IEEE fp32 operation:
    g1 = (c < 1) ? g * c : g;  m' = m + w1 * (g1 - m);  v' = b2 * v + (w2 * g1) * g1;  s = sqrt(v') / bc2s[t'] + eps;
    p' = p - step_size[t'] * (m' / s);  e' = e + wE * (p' - e)
with ``scalar_table`` / ``constants`` computed once in Python floats and rounded to fp32, t' = t + 1 and t the optimizer's own counter
in the record.  A skipped step changes nothing.  Tensors that live on the host (the tests' CPU environment, gloo) take ``host_step``:
the same definition in numpy, the same bits.

``--lr_schedule / --warmup_updates / --weight_decay``: the schedule is the table and nothing else -- ``scheduled_table`` puts lr(t') of
``learning_rates`` where ``scalar_table`` has lr, so the rate follows the steps TAKEN (a skipped step does not advance t') and is saved
with the optimizer state -- and the decoupled decay is one line in front of p's, p1 = p - (decay[t'] * p) with decay[t'] =
f32(lr(t') wd), for the generator's parameters with two or more dimensions: ``tai_fused_step_decay`` in place of ``tai_fused_step``
exactly when an optimizer has such an entry (restated in tests/fused_step_decay_ref.py).

``FusedStep`` belongs to one training environment.  The optimizers stay ``torch.optim.Adam`` objects used as state containers
(``exp_avg``, ``exp_avg_sq``, ``step`` live where the parameters live; ``optimizer_state_dict`` writes ``step`` the way the eager
optimizer does, ``after_load`` converts it back).  The guard's counters live in the record; the record is copied into a pinned slot
after every update and read when the copy has finished, and waited for only where the run waits anyway (a printed line, validation,
``save``): ``read(wait=True)``.  ``GuardGaveUp`` is raised, with the message of the host-side guard, by whichever read sees the flag;
on the device every step after it is a skip, so the state stays where the host-side guard would have stopped the run.

One counter per optimizer: a parameter that receives its first gradient later than the others shares it (torch.optim.Adam would start
that parameter's bias correction at 1); no model of this package has such a parameter.
"""
import collections
import math

import numpy as np
import torch

from . import conv_ops, grad_guard, parallel
from .grad_guard import CLIPPED, OK, SEG, SKIPPED, GuardGaveUp

REC_WORDS = 32
(R_SKIPPED, R_CONSECUTIVE, R_GAVE_UP, R_IN_UPDATE, R_BAD_WHICH, R_BAD_FIRST, R_BAD_FIRST_COUNT, R_BAD_TOTAL, R_BAD_ENTRIES, R_VERDICT,
 R_COEFF, R_TOTAL, R_T, R_TPRIME, R_OVERFLOW, R_CLOSED, R_GAVE_UP_AT) = (0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16, 18, 20, 21, 22)
WHICH = {'G': 0, 'D': 1}
NT_LOADS = 0                    # non-temporal loads of g, m, v: no faster than plain loads (tools/fused_step_bench.py)
RING = 4                        # pinned slots the record is copied into, one per update in flight
NO_PATIENCE = 1 << 62

Constants = collections.namedtuple('Constants', 'w1 b2 w2 eps wE')


def scalar_table(lr, beta1, beta2, length):
    """(step_size, bc2s): fp32 arrays whose element t' - 1 belongs to step t' = 1 ... length."""
    step_size, bc2s = np.empty(length, np.float32), np.empty(length, np.float32)
    lr, beta1, beta2 = float(lr), float(beta1), float(beta2)
    for t in range(1, length + 1):
        step_size[t - 1] = np.float32(lr / (1.0 - beta1 ** t))
        bc2s[t - 1] = np.float32(math.sqrt(1.0 - beta2 ** t))
    return step_size, bc2s


SCHEDULES = ('constant', 'step', 'cosine')


class Schedule(collections.namedtuple('Schedule', 'kind warmup_updates decay_every gamma min_ratio')):
    """``--lr_schedule kind --warmup_updates W --lr_decay_every E --lr_gamma g --lr_min_ratio r``; the defaults are the constant rate."""
    __slots__ = ()

    def __new__(cls, kind='constant', warmup_updates=0, decay_every=10000, gamma=0.5, min_ratio=0.01):
        return super().__new__(cls, str(kind), int(warmup_updates), int(decay_every), float(gamma), float(min_ratio))

    @property
    def on(self):
        return self.kind != 'constant' or self.warmup_updates > 0

    def check(self):
        """Raises ValueError naming the flag whose value is refused."""
        if self.kind not in SCHEDULES:
            raise ValueError('--lr_schedule must be one of %s, found %r' % (', '.join(SCHEDULES), self.kind))
        if self.warmup_updates < 0:
            raise ValueError('--warmup_updates must not be negative, found %r' % (self.warmup_updates,))
        if self.decay_every < 1:
            raise ValueError('--lr_decay_every must be at least 1, found %r' % (self.decay_every,))
        if not 0.0 <= self.gamma <= 1.0:
            raise ValueError('--lr_gamma must lie in [0, 1], found %r' % (self.gamma,))
        if not 0.0 <= self.min_ratio <= 1.0:
            raise ValueError('--lr_min_ratio must lie in [0, 1], found %r' % (self.min_ratio,))


def check_weight_decay(wd):
    if not (float(wd) >= 0.0 and float(wd) != float('inf')):
        raise ValueError('--weight_decay must be finite and not negative, found %r' % (wd,))


def needs_fused_step(schedule, weight_decay):
    """The words with which a run without ``--fused_step`` is refused, or None."""
    schedule = schedule or Schedule()
    for on, flag in ((schedule.kind != 'constant', '--lr_schedule %s' % schedule.kind), (schedule.warmup_updates > 0, '--warmup_updates'),
                     (weight_decay > 0.0, '--weight_decay')):
        if on:
            return '%s needs --fused_step: the schedule is the fused optimizer step\'s scalar table, the decay a line of its kernel' % flag
    return None


def learning_rates(lr, length, schedule=None, n_steps=None):
    """lr(t') for t' = 1 ... length as Python floats (include/tai_sepconv.h); ``n_steps``: the N of the cosine, ``length`` by default."""
    sc = schedule or Schedule()
    L, W, N = float(lr), sc.warmup_updates, int(length if n_steps is None else n_steps)
    out = []
    for t in range(1, length + 1):
        warm = t / W if t <= W else 1.0
        if sc.kind == 'step':
            s = sc.gamma ** ((t - 1) // sc.decay_every)
        elif sc.kind == 'cosine' and t > W:
            u = min(1.0, (t - W) / max(1, N - W))
            s = sc.min_ratio + (1.0 - sc.min_ratio) * (0.5 * (1.0 + math.cos(math.pi * u)))
        else:
            s = 1.0
        out.append((L * warm) * s)
    return out


def scheduled_table(lr, beta1, beta2, length, schedule=None, weight_decay=0.0, n_steps=None):
    """(step_size, bc2s, decay): ``scalar_table`` with lr(t') of the schedule in place of lr, and decay[t'] = f32(lr(t') * wd).  With the
    constant schedule, no warm-up and no decay the first two are ``scalar_table``'s bit for bit."""
    step_size, bc2s, decay = np.empty(length, np.float32), np.empty(length, np.float32), np.empty(length, np.float32)
    beta1, beta2, wd = float(beta1), float(beta2), float(weight_decay)
    for t, rate in enumerate(learning_rates(lr, length, schedule, n_steps), 1):
        step_size[t - 1] = np.float32(rate / (1.0 - beta1 ** t))
        bc2s[t - 1] = np.float32(math.sqrt(1.0 - beta2 ** t))
        decay[t - 1] = np.float32(rate * wd)
    return step_size, bc2s, decay


def constants(beta1, beta2, ema_decay=None):
    d = 0.0 if ema_decay is None else float(ema_decay)
    return Constants(np.float32(1.0 - float(beta1)), np.float32(float(beta2)), np.float32(1.0 - float(beta2)), np.float32(1e-8),
                     np.float32(1.0 - d))


def check_ema_decay(d):
    if d is not None and not (0.0 < float(d) < 1.0):
        raise ValueError('--ema_decay must lie strictly between 0 and 1, found %r' % (d,))


def host_step(p, g, m, v, e, c, step_size, bc2s, k, decay=None):
    """The definition on float32 numpy arrays, in place (``e`` may be None; ``g`` is left alone).  ``decay``: decay[t'] for an entry
    that decays (p1 = p - (decay * p) first), None for one that does not: its p is multiplied by nothing."""
    c, step_size, bc2s = np.float32(c), np.float32(step_size), np.float32(bc2s)
    with np.errstate(all='ignore'):
        if decay is not None:
            np.subtract(p, np.multiply(np.float32(decay), p), out=p)
        g1 = np.multiply(g, c) if c < np.float32(1) else g
        d = np.subtract(g1, m)
        np.add(m, np.multiply(k.w1, d), out=m)
        wgg = np.multiply(np.multiply(k.w2, g1), g1)
        np.add(np.multiply(k.b2, v), wgg, out=v)
        s = np.add(np.divide(np.sqrt(v), bc2s), k.eps)
        np.subtract(p, np.multiply(step_size, np.divide(m, s)), out=p)
        if e is not None:
            np.add(e, np.multiply(k.wE, np.subtract(p, e)), out=e)


def host_verdict(rec, sumsq, nonfinite, max_norm, which, close_update, patience, table_len):
    """``tai_step_verdict`` on a numpy record (int64 [REC_WORDS]), in place.  sumsq / nonfinite: arrays of n + 1 elements, or None."""
    frozen = rec[R_GAVE_UP] != 0
    verdict, tprime, c = OK, 0, np.float32(1)
    if frozen:
        verdict = SKIPPED
    else:
        total = float(sumsq[-1]) if sumsq is not None else 0.0
        bad = int(nonfinite[-1]) if nonfinite is not None else 0
        if bad > 0:
            verdict = SKIPPED
            where = np.flatnonzero(np.asarray(nonfinite[:-1]) > 0)
            rec[R_SKIPPED + which] += 1
            rec[R_IN_UPDATE] = 1
            rec[R_BAD_WHICH], rec[R_BAD_FIRST], rec[R_BAD_FIRST_COUNT] = which, int(where[0]), int(nonfinite[where[0]])
            rec[R_BAD_TOTAL], rec[R_BAD_ENTRIES] = bad, where.size
        elif sumsq is not None and max_norm:
            c = np.float32(grad_guard.clip_coefficient(total, 0, max_norm))
            verdict = CLIPPED if c < np.float32(1) else OK
        rec[R_TOTAL + which] = np.array([total], np.float64).view(np.int64)[0]
        if verdict != SKIPPED:
            tprime = int(rec[R_T + which]) + 1
            if tprime > table_len:
                rec[R_OVERFLOW], verdict, tprime = 1, SKIPPED, 0
            else:
                rec[R_T + which] = tprime
    rec[R_VERDICT + which] = verdict
    rec[R_COEFF + which] = int(np.array([c], np.float32).view(np.uint32)[0])
    rec[R_TPRIME + which] = tprime
    if close_update and not frozen:
        run = int(rec[R_CONSECUTIVE]) + 1 if rec[R_IN_UPDATE] else 0
        rec[R_CONSECUTIVE], rec[R_IN_UPDATE] = run, 0
        rec[R_CLOSED] += 1
        if run >= patience:
            rec[R_GAVE_UP], rec[R_GAVE_UP_AT] = 1, rec[R_CLOSED]


def record_coefficient(rec, which):
    return np.array([int(rec[R_COEFF + which]) & 0xFFFFFFFF], np.uint32).view(np.float32)[0]


def record_total(rec, which):
    return float(np.array([rec[R_TOTAL + which]], np.int64).view(np.float64)[0])


def step_rows(params, grads, exp_avgs, exp_avg_sqs, steps, emas):
    """-> (rows int64 [n, 8] as ``tai_fused_step`` takes them, segments).  ``steps`` / ``emas``: tensors or None per entry."""
    rows, n_segments = [], 0
    for p, g, m, v, s, e in zip(params, grads, exp_avgs, exp_avg_sqs, steps, emas):
        n = p.numel()
        for t in (p, g, m, v) + ((e,) if e is not None else ()):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
                raise ValueError('fused step: an entry needs contiguous float32 tensors of one size, found %s %s' % (t.dtype, tuple(t.shape)))
        rows.append((p.data_ptr() if n else 0, g.data_ptr() if n else 0, m.data_ptr() if n else 0, v.data_ptr() if n else 0,
                     0 if s is None else s.data_ptr(), e.data_ptr() if (e is not None and n) else 0, n, n_segments))
        n_segments += -(-n // SEG)
    return np.array(rows, dtype=np.uint64).view(np.int64).reshape(len(rows), 8), n_segments


class _Tables(object):
    """Device buffers of one optimizer's tables (the statistics' rows of four, the step's rows of eight), filled through pinned memory so
    that a change of a gradient's address costs a copy the host does not wait for."""

    def __init__(self, n, n_segments, device, with_flags=False):
        from . import _native
        self.n, self.n_segments, self.with_flags = n, n_segments, bool(with_flags)
        words = (13 if with_flags else 12) * n           # with_flags: tai_fused_step_decay's word per entry behind the rows, one upload
        self.both = torch.empty(words, dtype=torch.int64, device=device)
        self.stats, self.rows, self.flags = self.both[:4 * n], self.both[4 * n:12 * n], self.both[12 * n:]
        self.pinned = [torch.empty(words, dtype=torch.int64).pin_memory() for _ in range(2)]
        self.events = [None, None]
        self.flip = 0
        self.host = None
        nbytes = _native.lib().tai_grad_stats_workspace_bytes(n, n_segments)
        self.workspace = torch.empty(nbytes // 8 + 2, dtype=torch.int64, device=device)
        self.result = torch.zeros(5 * (n + 1), dtype=torch.int32, device=device)      # grad_guard._Buffers' layout

    def upload(self, stats_rows, step_rows_, flags=None):
        host = np.concatenate([stats_rows.reshape(-1), step_rows_.reshape(-1)] + ([flags] if self.with_flags else []))
        if self.host is not None and np.array_equal(self.host, host):
            return
        i = self.flip
        if self.events[i] is not None:
            self.events[i].synchronize()                 # two uploads back: long finished
        self.pinned[i].numpy()[:] = host
        self.both.copy_(self.pinned[i], non_blocking=True)
        self.events[i] = torch.cuda.Event()
        self.events[i].record()
        self.flip ^= 1
        self.host = host


class _Optimizer(object):
    def __init__(self, module, optimizer, k, step_size, bc2s, device, decay=None, rates=None):
        self.module, self.optimizer, self.k = module, optimizer, k
        self.step_size, self.bc2s = step_size, bc2s
        self.decay = decay                           # decay[t' - 1] (fp32) of an optimizer whose weights decay, else None
        self.rates = rates                           # lr(t') as Python floats, for the printed line
        rows = [step_size, bc2s] + ([decay] if decay is not None else [])
        self.scalars = torch.from_numpy(np.concatenate(rows)).to(device) if device.type == 'cuda' else None
        self.names = []
        self.tables = None


class FusedStep(object):
    def __init__(self, device, max_steps, guard=None, ema_decay=None, schedule=None, weight_decay=0.0):
        check_ema_decay(ema_decay)
        self.schedule = schedule or Schedule()
        self.schedule.check()
        check_weight_decay(weight_decay)
        self.weight_decay = float(weight_decay)
        self.max_steps = int(max_steps)              # the N of the cosine
        self._base_lr = {}                           # optimizer -> the rate its table was built from
        self.last_rate = {}                          # optimizer -> lr(t') of its last taken step, as of the last record applied
        self.device = torch.device(device)
        self.on_device = self.device.type == 'cuda'
        self.guard = guard
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.table_len = int(max_steps) + 1
        self.rec = torch.zeros(REC_WORDS, dtype=torch.int64, device=self.device) if self.on_device else np.zeros(REC_WORDS, np.int64)
        self.ema = collections.OrderedDict()         # parameter name -> flat fp32 tensor, for the generator's parameters with a gradient
        self._ema_loaded = None                      # a snapshot's generator_ema, until the first step takes its tensors
        self._opt = {}
        self._ring = [[torch.zeros(REC_WORDS, dtype=torch.int64).pin_memory(), None, -1] for _ in range(RING)] if self.on_device else []
        self._updates = 0                            # updates closed since the record was last set
        self._applied = -1
        self.waits = 0                               # reads of the record the host waited for
        self.blocks = 0

    # ---- set-up
    def attach(self, which, module, optimizer):
        if len(optimizer.param_groups) != 1:
            raise ValueError('fused step: one parameter group per optimizer')
        group = optimizer.param_groups[0]
        if group['eps'] != 1e-8 or group['weight_decay'] != 0 or group['amsgrad'] or group.get('maximize') or group.get('capturable'):
            raise ValueError('fused step: the definition is plain Adam with eps 1e-8 (no weight decay, amsgrad, maximize, capturable)')
        beta1, beta2 = group['betas']
        k = constants(beta1, beta2, self.ema_decay if which == 'G' else None)
        self._base_lr[which] = float(group['lr'])
        if not self.scheduled:
            step_size, bc2s = scalar_table(group['lr'], beta1, beta2, self.table_len)
            self._opt[which] = _Optimizer(module, optimizer, k, step_size, bc2s, self.device)
            return
        # the decay is the generator's alone (the discriminator's weights are spectrally normalised); the torch optimizer's own
        # weight_decay stays 0: it is a state container here
        wd = self.weight_decay if which == 'G' else 0.0
        step_size, bc2s, decay = scheduled_table(group['lr'], beta1, beta2, self.table_len, self.schedule, wd, self.max_steps)
        self._opt[which] = _Optimizer(module, optimizer, k, step_size, bc2s, self.device, decay if wd > 0.0 else None,
                                      learning_rates(group['lr'], self.table_len, self.schedule, self.max_steps) if self.schedule.on else None)

    @property
    def scheduled(self):
        """A schedule, a warm-up or a decay is on: the tables are ``scheduled_table``'s and the run state records the settings."""
        return self.schedule.on or self.weight_decay > 0.0

    def settings(self):
        """What a continuation must repeat (run_state's ``lr_schedule``), or None without a schedule, a warm-up and a decay."""
        if not self.scheduled:
            return None
        sc = self.schedule
        out = {'lr_schedule': sc.kind, 'warmup_updates': sc.warmup_updates, 'lr_decay_every': sc.decay_every, 'lr_gamma': sc.gamma,
               'lr_min_ratio': sc.min_ratio, 'weight_decay': self.weight_decay, 'max_iter': self.max_steps}
        out.update(('lr' if which == 'G' else 'lr_D', lr) for which, lr in self._base_lr.items())
        return out

    def check_continues(self, saved):
        """Refuse (ValueError) a continuation whose settings are not those the snapshot's run recorded; both are named."""
        mine = self.settings()
        if saved != mine:
            show = lambda s: 'no schedule, warm-up or decay' if s is None else ' '.join('--%s %s' % kv for kv in sorted(s.items()))
            raise ValueError('the snapshot was written with %s, this run has %s: another schedule is another run, it cannot be continued '
                             'exactly' % (show(saved), show(mine)))

    def rates_suffix(self):
        """`` lr_G= lr_D=`` of the last taken steps for a printed line (after ``read``), '' without a schedule or a warm-up."""
        if not self.schedule.on:
            return ''
        return ''.join(' lr_%s=%.6g' % (which, self.last_rate.get(which, 0.0)) for which in 'GD' if which in self._opt)

    def _entries(self, which):
        o = self._opt[which]
        named = [(n, p) for n, p in o.module.named_parameters() if p.grad is not None]
        if not named:
            raise RuntimeError('fused step: no parameter of optimizer %s has a gradient' % which)
        state = o.optimizer.state
        for _, p in named:
            if len(state[p]) == 0:
                st = state[p]
                st['step'] = torch.zeros((), dtype=torch.float32, device=p.device)
                st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        with_ema = which == 'G' and self.ema_decay is not None
        if with_ema:
            for n, p in named:
                if n not in self.ema:
                    src = self._ema_loaded.get(n) if self._ema_loaded is not None else None
                    self.ema[n] = (p if src is None else src).detach().to(p.device, torch.float32).clone().reshape(-1)
        o.names = [n for n, _ in named]
        params = [p.detach() for _, p in named]
        # the entries that decay: the weights (two or more dimensions) of an optimizer with a decay table, never a bias
        flags = np.array([int(o.decay is not None and p.dim() >= 2) for _, p in named], np.int64)
        return (params, [p.grad.detach() for _, p in named], [state[p]['exp_avg'] for _, p in named],
                [state[p]['exp_avg_sq'] for _, p in named], [state[p]['step'] for _, p in named],
                [self.ema[n] if with_ema else None for n, _ in named], flags)

    # ---- the step
    def step(self, which, last):
        """The step of optimizer ``which`` ('G' or 'D') on the gradients its parameters hold now; ``last``: it is the update's last."""
        o, w = self._opt[which], WHICH[which]
        params, grads, ms, vs, steps, emas, flags = self._entries(which)
        decays = bool(flags.any())                       # tai_fused_step_decay exactly then; tai_fused_step otherwise
        guard = self.guard
        max_norm = 0.0 if guard is None or guard.clip_grad_norm is None else guard.clip_grad_norm
        patience = NO_PATIENCE if guard is None else guard.patience
        if not self.on_device:
            sumsq = nonfinite = None
            if guard is not None:
                sumsq, _, nonfinite = grad_guard._stats_host(grads)
            host_verdict(self.rec, sumsq, nonfinite, max_norm, w, last, patience, self.table_len)
            if self.rec[R_VERDICT + w] != SKIPPED:
                t, c = int(self.rec[R_TPRIME + w]), record_coefficient(self.rec, w)
                for p, g, m, v, s, e, f in zip(params, grads, ms, vs, steps, emas, flags):
                    if p.numel():
                        host_step(p.numpy().reshape(-1), g.numpy().reshape(-1), m.numpy().reshape(-1), v.numpy().reshape(-1),
                                  None if e is None else e.numpy(), c, o.step_size[t - 1], o.bc2s[t - 1], o.k,
                                  o.decay[t - 1] if f else None)
                    s.fill_(float(t))
        else:
            from . import _native
            rows, n_segments = step_rows(params, grads, ms, vs, steps, emas)
            n = rows.shape[0]
            stats_rows = np.ascontiguousarray(rows[:, [1, 6, 6, 7]])
            stats_rows[:, 2] = 0
            if o.tables is None or (o.tables.n, o.tables.n_segments, o.tables.with_flags) != (n, n_segments, decays):
                o.tables = _Tables(n, n_segments, self.device, with_flags=decays)
            tb = o.tables
            with torch.cuda.device(self.device):
                tb.upload(stats_rows, rows, flags)
                sumsq_ptr = bad_ptr = None
                if guard is not None:
                    base = tb.result.data_ptr()
                    sumsq_ptr, bad_ptr = base, base + 8 * (n + 1)
                    _native.launch('tai_grad_stats', self.device, tb.stats, stats_rows.ctypes.data, n, n_segments, 0, tb.workspace,
                                   base, base + 16 * (n + 1), bad_ptr)
                _native.launch('tai_step_verdict', self.device, sumsq_ptr, bad_ptr, n, float(max_norm), w, int(bool(last)), patience,
                               self.table_len, self.rec)
                if decays:
                    _native.launch('tai_fused_step_decay', self.device, tb.rows, rows.ctypes.data, tb.flags, flags.ctypes.data, n, n_segments,
                                   o.scalars, self.table_len, float(o.k.w1), float(o.k.b2), float(o.k.w2), float(o.k.eps), float(o.k.wE),
                                   self.rec, w, int(self.blocks), None)
                else:
                    _native.launch('tai_fused_step', self.device, tb.rows, rows.ctypes.data, n, n_segments, o.scalars, self.table_len,
                                   float(o.k.w1), float(o.k.b2), float(o.k.w2), float(o.k.eps), float(o.k.wE), self.rec, w, int(NT_LOADS),
                                   int(self.blocks), None)
        # the weights were written through raw pointers (numpy views on the host): no version counter moved.  Whatever the verdict --
        # the host does not know it -- no derived form of this module's weights stays valid; the other module's forms are left alone
        conv_ops.invalidate_derived(o.module)
        if last:
            self._end_update()

    def _end_update(self):
        self._updates += 1
        if not self.on_device:
            self._apply(self.rec)
            return
        slot = self._ring[self._updates % RING]
        if slot[1] is not None and not slot[1].query():
            slot[1].synchronize()                        # RING updates back
        if slot[2] > self._applied:
            self._apply_slot(slot)
        with torch.cuda.device(self.device):
            slot[0].copy_(self.rec, non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record()
        slot[2] = self._updates
        self.poll()

    def _apply_slot(self, slot):
        self._applied = slot[2]
        self._apply(slot[0].numpy().copy())

    def poll(self):
        """Take in the newest record whose copy has finished; never waits."""
        done = [s for s in self._ring if s[1] is not None and s[2] > self._applied and s[1].query()]
        if done:
            self._apply_slot(max(done, key=lambda s: s[2]))

    def read(self, wait=True, agree=False):
        """Bring the guard's host-side view up to the record.  ``wait``: up to the last launched update (synchronises).  ``agree``: a
        collective in a data-parallel run -- the counters are max- and min-reduced over the ranks and must not differ."""
        if not self.on_device:
            rec = self.rec
        elif wait:
            self.waits += 1
            rec = self.rec.cpu().numpy()                 # synchronises
            self._applied = self._updates
        else:
            self.poll()
            return
        if agree and parallel.world_size() > 1:
            self._agree(rec)
        self._apply(rec)

    def _agree(self, rec):
        import torch.distributed as dist
        mine = [int(rec[i]) for i in (R_SKIPPED, R_SKIPPED + 1, R_CONSECUTIVE, R_GAVE_UP, R_T, R_T + 1)]
        on_gpu = dist.get_backend() == 'nccl'
        t = torch.tensor(mine + [-x for x in mine], dtype=torch.int64, device=self.device if on_gpu else 'cpu')
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        t = t.tolist()
        if t[:6] != [-x for x in t[6:]]:
            raise RuntimeError('fused step: the ranks disagree on the guard counters (skipped_G, skipped_D, consecutive, gave_up, t_G, t_D): '
                               'largest %r, smallest %r' % (t[:6], [-x for x in t[6:]]))

    def _apply(self, rec):
        if rec[R_OVERFLOW]:
            raise RuntimeError('fused step: an optimizer was asked for more than the %d steps its scalar table holds (--max_iter)'
                               % self.table_len)
        if self.schedule.on:                             # the rate of the last taken step: t is the number of steps made
            for which, o in self._opt.items():
                t = int(rec[R_T + WHICH[which]])
                self.last_rate[which] = o.rates[t - 1] if t >= 1 else 0.0
        g = self.guard
        if g is None:
            return
        g.skipped = {'G': int(rec[R_SKIPPED]), 'D': int(rec[R_SKIPPED + 1])}
        g.consecutive = int(rec[R_CONSECUTIVE])
        for which, w in WHICH.items():
            if which not in self._opt:
                continue
            g.norm[which] = math.sqrt(record_total(rec, w))
            g.verdict[which] = int(rec[R_VERDICT + w])
            g.coefficient[which] = record_coefficient(rec, w) if g.verdict[which] == CLIPPED else 1.0
        if rec[R_BAD_TOTAL] > 0:
            which = 'GD'[int(rec[R_BAD_WHICH])]
            names = self._opt[which].names
            first = int(rec[R_BAD_FIRST])
            g.message = '%s: %d non-finite gradient element(s) in %s (%d in %d parameter(s) in all)' % (
                which, int(rec[R_BAD_FIRST_COUNT]), names[first] if first < len(names) else 'entry %d' % first, int(rec[R_BAD_TOTAL]),
                int(rec[R_BAD_ENTRIES]))
        if rec[R_GAVE_UP]:
            e = GuardGaveUp('%d consecutive updates had an optimizer step skipped (--guard_patience %d); the last one: %s'
                            % (g.consecutive, g.patience, g.message))
            e.updates_ago = self._updates - int(rec[R_GAVE_UP_AT])        # the update that gave up, counted back from the last launched
            raise e

    # ---- snapshots
    def optimizer_state_dict(self, optimizer):
        """``optimizer.state_dict()`` with ``step`` in the form the eager optimizer writes: a float32 scalar on the host."""
        sd = optimizer.state_dict()
        sd['state'] = {i: dict(st, step=st['step'].detach().to('cpu', torch.float32).reshape(()).clone()) if 'step' in st else dict(st)
                       for i, st in sd['state'].items()}
        return sd

    def after_load(self, snapshot, ema_names=None):
        """After the optimizers have loaded a snapshot's state: ``step`` moves to where the parameters live, the counters t enter the
        record, the EMA is the snapshot's ``generator_ema`` (or starts from the weights at the first step when there is none)."""
        rec = np.zeros(REC_WORDS, np.int64)
        for which, o in self._opt.items():
            ts = set()
            for p, st in o.optimizer.state.items():
                if 'step' in st:
                    st['step'] = torch.as_tensor(st['step'], dtype=torch.float32).detach().reshape(()).to(p.device).clone()
                    ts.add(float(st['step']))
            if len(ts) > 1:
                raise ValueError('fused step: the parameters of optimizer %s have made different numbers of steps: %s' % (which, sorted(ts)))
            rec[R_T + WHICH[which]] = int(ts.pop()) if ts else 0
            o.tables = None
        self.ema.clear()
        self._ema_loaded = snapshot.get('generator_ema') if self.ema_decay is not None else None
        if self._ema_loaded is not None and ema_names:
            for n in ema_names:
                self.ema[n] = self._ema_loaded[n].detach().to(self.device, torch.float32).clone().reshape(-1)
        self._set_record(rec)

    def push_counters(self):
        """The guard's host-side counters (a snapshot's, just loaded) into the record."""
        if self.guard is None:
            return
        rec = self.rec.copy() if not self.on_device else self.rec.cpu().numpy()
        c = self.guard.counters()
        rec[R_SKIPPED], rec[R_SKIPPED + 1], rec[R_CONSECUTIVE] = c['skipped_G'], c['skipped_D'], c['consecutive']
        self._set_record(rec)

    def _set_record(self, rec):
        if self.on_device:
            self.rec.copy_(torch.from_numpy(rec))
            for slot in self._ring:
                slot[1], slot[2] = None, -1
        else:
            self.rec[:] = rec
        self._updates, self._applied = 0, -1

    def ema_state_dict(self, generator):
        """A generator ``state_dict`` with the averaged values; buffers and parameters without an average as they are."""
        sd = collections.OrderedDict((k, v.detach().clone()) for k, v in generator.state_dict().items())
        for source in (self._ema_loaded or {}, self.ema):
            for n, e in source.items():
                if n in sd:
                    sd[n] = e.detach().to(sd[n].device).reshape(sd[n].shape).clone()
        return sd

    def named_ema(self):
        return [('generator_ema.' + n, e) for n, e in self.ema.items()]


def snapshot_ema_entries(snapshot):
    """The EMA entries of the digest's table of the run that wrote ``snapshot``, or None."""
    names = (snapshot.get('run_state') or {}).get('ema')
    if not names or snapshot.get('generator_ema') is None:
        return None
    return [snapshot['generator_ema'][n].detach().reshape(-1) for n in names]


class averaged_weights(object):
    """``with averaged_weights(env):`` -- the generator's parameters hold the EMA inside the block (``p.data`` is exchanged with the EMA
    tensor: the Parameter objects and their dispatch marks stay) and the weights again after it."""

    def __init__(self, env):
        from . import conv_ops
        self.env, self.conv_ops = env, conv_ops
        fused = getattr(env, 'fused', None)
        self.ema = fused.ema if fused is not None and fused.ema_decay is not None else {}
        self.active = bool(self.ema)

    def __enter__(self):
        self.kept = {}
        if self.active:
            for n, p in self.env.generator.named_parameters():
                if n in self.ema:
                    self.kept[n] = p.data
                    p.data = self.ema[n].view(p.shape)
            self.conv_ops.invalidate_derived()
        return self

    def __exit__(self, *exc):
        if self.active:
            for n, p in self.env.generator.named_parameters():
                if n in self.kept:
                    p.data = self.kept[n]
            self.conv_ops.invalidate_derived()
        return False
