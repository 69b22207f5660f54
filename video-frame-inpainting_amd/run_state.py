"""What a snapshot needs beyond the reference's keys for a resumed run to be THE SAME run (``train.py --resumable``), and the 64-bit
state digest that says whether two states are.

``capture(env)`` -> the ``run_state`` dict of a snapshot: plain tensors, numbers, strings and tuples, no pickled classes.
  version      FORMAT_VERSION
  world_size   ranks of the run; a run_state recorded at another world size is refused for exact resume (the clip order, the shards and
               the gradient sums all depend on it)
  u            {module name: the spectral-norm vector ``u`` of that discriminator layer, or None}: a non-persistent buffer, drawn on first
               use and folded into the weights by every forward since (``weight <- weight / sigma``); redrawn, it no longer belongs to them
  ktf          the (K, T, F) stream ``env._ktf_rng`` (identical on every rank)
  ranks        a list indexed by rank, gathered to rank 0: {'data': the clip order's position (train.py), 'numpy', 'torch_cpu',
               'torch_cuda': the global generators, 'digest': that rank's state digest}
  digest       rank 0's state digest
  guard        (only with train.py --guard) the guard's counters {'skipped_G', 'skipped_D', 'consecutive'} (grad_guard.GradGuard); they
               are the last entry of the digest's table then, and only then: a snapshot written without the guard loads with it (the
               counters start at zero) and the other way round, and digests of runs without the guard are what they were
  ema          (only with train.py --ema_decay) the names of the generator parameters that carry an average, in table order; the averaged
               values are the snapshot's ``generator_ema``, and they are the entries behind the guard's in the digest's table then, and
               only then
  lr_schedule  (only with train.py --lr_schedule / --warmup_updates / --weight_decay) the settings of the fused step's scalar table
               (fused_step.FusedStep.settings: both base rates, the schedule, W, E, g, r, wd and the N of --max_iter); a continuation
               with others is refused.  Nothing enters the digest: the schedule's position t' is the optimizer state's ``step``
``restore(env, run_state)`` puts all of it back, the generator states LAST, and returns this rank's 'data' entry.

The digest (``tai_state_digest``, csrc/state_digest.hip.inc) reads every tensor of the state once, where it lives: about 0.5 GB of
weights and Adam moments for TAI_gray that a host hash would have to copy first.  Its definition, on 32-bit words, uint64 arithmetic:
    mix(z):  z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31)
    E_t = sum_i mix((i << 32) + w_t[i])            for entry t with words w_t[0..n_t)
    D   = 0x243F6A8885A308D3;  for t in table order:  D = mix(D ^ E_t);  D = mix(D + n_t)
Entries that live on the host (Adam's ``step`` in the eager form, generator states) are summed here with numpy and take their place in
the table order: the result is the same number wherever an entry lives.
"""
import signal
import time

import numpy as np
import torch

from . import parallel

FORMAT_VERSION = 1
SEG_WORDS = 16384               # words per segment of the device launch (64 KiB); the result does not depend on it

_GOLD, _M1, _M2, _SEED = (np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB),
                          0x243F6A8885A308D3)
_MASK = (1 << 64) - 1


def _mix_array(z):
    z = z + _GOLD
    z = (z ^ (z >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def _mix(z):
    z = (z + 0x9E3779B97F4A7C15) & _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def entry_sum_host(words):
    """E_t of a uint32 array, with numpy."""
    words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
    total = 0
    for a in range(0, words.size, 1 << 20):
        w = words[a:a + (1 << 20)]
        pos = np.arange(a, a + w.size, dtype=np.uint64)
        total += int(np.sum(_mix_array((pos << np.uint64(32)) + w.astype(np.uint64)), dtype=np.uint64))
    return total & _MASK


def _chain(sums_and_counts):
    d = _SEED
    for e, n in sums_and_counts:
        d = _mix(d ^ e)
        d = _mix((d + n) & _MASK)
    return d


def _host_words(t):
    """The raw 32-bit words of a host tensor / array (byte length a multiple of 4)."""
    if torch.is_tensor(t):
        t = t.detach().contiguous().reshape(-1).view(torch.uint8).numpy() if t.numel() else np.zeros(0, np.uint8)
    raw = np.ascontiguousarray(t).reshape(-1).view(np.uint8)
    if raw.size % 4:
        raise ValueError('state digest: an entry of %d bytes is not a whole number of 32-bit words' % raw.size)
    return raw.view(np.uint32)


def bytes_entry(raw):
    """Arbitrary bytes (a generator state) as a digest entry: the length as one 64-bit number, then the bytes, zero-padded to a word."""
    raw = np.ascontiguousarray(raw).reshape(-1).view(np.uint8)
    out = np.zeros(8 + -(-raw.size // 4) * 4, np.uint8)
    out[:8] = np.array([raw.size], dtype='<u8').view(np.uint8)
    out[8:8 + raw.size] = raw
    return out.view(np.uint32)


class _DeviceTable(object):
    """The device-side buffers of one table shape (rows, segments), kept between calls: printing the digest every --print_freq updates
    allocates nothing after the first time."""

    def __init__(self, n_entries, n_segments, device):
        from . import _native
        nbytes = _native.lib().tai_state_digest_workspace_bytes(n_entries, n_segments)
        if nbytes < 0:
            raise ValueError('state digest: bad table (%d entries, %d segments)' % (n_entries, n_segments))
        self.table = torch.empty(n_entries, 4, dtype=torch.int64, device=device)
        self.workspace = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=device)
        self.result = torch.zeros(1, dtype=torch.int64, device=device)


_tables = {}


def build_table(entries, seg_words=SEG_WORDS):
    """-> (rows int64 [n, 4] on the host as ``tai_state_digest`` takes them, the device of the CUDA entries or None, segments)."""
    rows, device, n_segments = [], None, 0
    for e in entries:
        if torch.is_tensor(e) and e.is_cuda:
            if not e.is_contiguous() or e.element_size() not in (4, 8):
                raise ValueError('state digest: a device entry must be contiguous with 4- or 8-byte elements, found %s %s'
                                 % (e.dtype, tuple(e.shape)))
            if device is not None and e.device != device:
                raise ValueError('state digest: entries on %s and %s' % (device, e.device))
            device = e.device
            n = e.numel() * e.element_size() // 4
            addr = e.data_ptr() if n else 0
            rows.append((addr, n, 0, n_segments))
            n_segments += -(-n // seg_words) if addr else 0
        else:
            words = _host_words(e)
            rows.append((0, int(words.size), entry_sum_host(words), n_segments))
    if not rows:
        raise ValueError('state digest: an empty table')
    return np.array(rows, dtype=np.uint64).view(np.int64).reshape(len(rows), 4), device, n_segments


def digest_tensors(entries, seg_words=SEG_WORDS):
    """The digest of a table of entries, in order.  An entry is a CUDA tensor (contiguous, element size 4 or 8; read where it is), a host
    tensor or a numpy array (summed here).  With no CUDA entry nothing touches the GPU.  All CUDA entries live on one device."""
    entries = list(entries)                                 # (held until the launch has finished)
    host, device, n_segments = build_table(entries, seg_words)
    if device is None:
        return _chain((int(r[2]) & _MASK, int(r[1])) for r in host)
    from . import _native
    key = (device, host.shape[0], n_segments)
    if key not in _tables:
        _tables[key] = _DeviceTable(host.shape[0], n_segments, device)
    bufs = _tables[key]
    with torch.cuda.device(device):
        bufs.table.copy_(torch.from_numpy(host))          # pageable memory: the copy has left `host` when it returns
        _native.launch('tai_state_digest', device, bufs.table, host.ctypes.data, host.shape[0], n_segments, int(seg_words),
                       bufs.workspace, bufs.result)
        value = int(bufs.result.item())                    # synchronises
    return value & _MASK


def _rng_state_tuple(state):
    """numpy's ('MT19937', keys, pos, has_gauss, cached_gaussian) with the keys as a tensor."""
    name, keys, pos, has_gauss, cached = state
    return (str(name), torch.from_numpy(np.asarray(keys, dtype=np.uint32).astype(np.int64)), int(pos), int(has_gauss), float(cached))


def _rng_state_numpy(state):
    """... and back (the tensor may have been mapped to a device by the snapshot's ``torch.load``)."""
    name, keys, pos, has_gauss, cached = state
    return (str(name), np.asarray(keys.cpu().numpy() if torch.is_tensor(keys) else keys).astype(np.uint32), int(pos), int(has_gauss),
            float(cached))


def _rng_entry(state):
    name, keys, pos, has_gauss, cached = _rng_state_numpy(state)
    return bytes_entry(np.concatenate([keys.view(np.uint8), np.array([pos, has_gauss], dtype='<i8').view(np.uint8),
                                       np.array([cached], dtype='<f8').view(np.uint8)]))


_CURRENT = object()


def sn_vectors(discriminator):
    """{module name: u or None} of the spectrally normalised layers, in module order."""
    if discriminator is None:
        return {}
    return {name: m.u for name, m in discriminator.named_modules() if hasattr(m, 'Ip') and hasattr(m, 'u')}


def _optimizer_entries(optimizer):
    out = []
    for group in optimizer.param_groups:
        for p in group['params']:
            st = optimizer.state.get(p)
            if st:
                for k in ('step', 'exp_avg', 'exp_avg_sq'):
                    v = st[k]
                    out.append(v if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float32))
    return out


def _guard_counters(env):
    guard = getattr(env, 'guard', None)
    return None if guard is None else guard.counters()


def _ema_entries(env):
    fused = getattr(env, 'fused', None)
    return list(fused.ema.values()) if fused is not None and fused.ema_decay is not None and fused.ema else None


def state_entries(env, data_state=None, guard_counters=_CURRENT, ema=_CURRENT):
    """The digest's table for a training environment, in its fixed order: generator, discriminator (state-dict order), the two
    optimizers (per parameter: step, exp_avg, exp_avg_sq), the ``u`` vectors (None: an empty entry), then the generators -- the
    (K, T, F) stream, numpy's, torch's CPU and device generators -- and the clip order's position; with a guard (``env.guard``, or the
    counters of a snapshot written with one) its three counters are one more entry behind them; with a weight average (``env.fused``
    with --ema_decay, or the averages of a snapshot written with one) its tensors are the last entries."""
    if guard_counters is _CURRENT:
        guard_counters = _guard_counters(env)
    if ema is _CURRENT:
        ema = _ema_entries(env)
    entries = [t.detach() for t in env.generator.state_dict().values()]
    disc = getattr(env, 'discriminator', None)
    if disc is not None:
        entries += [t.detach() for t in disc.state_dict().values()]
    entries += _optimizer_entries(env.optimizer_G)
    if disc is not None:
        entries += _optimizer_entries(env.optimizer_D)
    for u in sn_vectors(disc).values():
        entries.append(np.zeros(0, np.uint32) if u is None else u.detach())
    entries.append(_rng_entry(env._ktf_rng.get_state()))
    entries.append(_rng_entry(np.random.get_state()))
    entries.append(bytes_entry(torch.get_rng_state().numpy()))
    if env.device.type == 'cuda':
        entries.append(bytes_entry(torch.cuda.get_rng_state(env.device).numpy()))
    entries.append(bytes_entry(np.frombuffer(repr(data_state).encode(), dtype=np.uint8)))
    if guard_counters is not None:
        entries.append(np.array([guard_counters[k] for k in ('skipped_G', 'skipped_D', 'consecutive')], dtype='<i8').view(np.uint32))
    if ema is not None:
        entries += [e.detach() for e in ema]
    return [e.contiguous() if torch.is_tensor(e) else e for e in entries]


def _data_state(env):
    source = getattr(env, 'data_state_source', None)
    return _plain(source()) if source is not None else None


def _plain(state):
    """numpy generator states inside a data state become tuples with tensors."""
    if isinstance(state, dict):
        return {k: _plain(v) for k, v in state.items()}
    if isinstance(state, tuple) and len(state) == 5 and state[0] == 'MT19937':
        return _rng_state_tuple(state)
    return state


def _printable(state):
    """A data state in a form whose repr depends on its values only (tensors spelled out)."""
    if isinstance(state, dict):
        return tuple((k, _printable(v)) for k, v in sorted(state.items()))
    if isinstance(state, (tuple, list)):
        return tuple(_printable(v) for v in state)
    if torch.is_tensor(state):
        return tuple(state.reshape(-1).tolist())
    if isinstance(state, np.ndarray):
        return tuple(state.reshape(-1).tolist())
    return state


def digest(env, data_state=_CURRENT, guard_counters=_CURRENT, ema=_CURRENT):
    """The 64-bit state digest of a training environment and of the clip order's position: the one train.py has attached
    (``env.data_state_source``), or ``data_state`` (a snapshot's, before train.py has positioned its clip order with it).
    ``guard_counters``: the guard entry of the table -- the environment's own guard by default, a snapshot's ``run_state.get('guard')``
    when the digest that snapshot was saved with is recomputed; ``ema``: the same for the weight average's entries."""
    return digest_tensors(state_entries(env, _printable(_data_state(env) if data_state is _CURRENT else data_state), guard_counters, ema))


def _gather(entry):
    world = parallel.world_size()
    if world == 1:
        return [entry]
    import torch.distributed as dist
    out = [None] * world
    dist.all_gather_object(out, entry)
    return out


def capture(env):
    """The ``run_state`` of a snapshot.  A collective in a data-parallel run: every rank calls it, rank 0's result is the one saved."""
    mine = {'data': _data_state(env),
            'numpy': _rng_state_tuple(np.random.get_state()),
            'torch_cpu': torch.get_rng_state().clone(),
            'torch_cuda': torch.cuda.get_rng_state(env.device).clone() if env.device.type == 'cuda' else None,
            'digest': digest(env)}
    ranks = _gather(mine)
    state = {'version': FORMAT_VERSION,
             'world_size': parallel.world_size(),
             'u': {name: (None if u is None else u.detach().clone()) for name, u in sn_vectors(getattr(env, 'discriminator', None)).items()},
             'ktf': _rng_state_tuple(env._ktf_rng.get_state()),
             'ranks': ranks,
             'digest': ranks[0]['digest']}
    if _guard_counters(env) is not None:
        state['guard'] = _guard_counters(env)
    if _ema_entries(env) is not None:
        state['ema'] = list(env.fused.ema)
    fused = getattr(env, 'fused', None)
    if fused is not None and fused.settings() is not None:
        state['lr_schedule'] = fused.settings()
    return state


class RunStateRefused(RuntimeError):
    """The run_state of a snapshot cannot be used for an exact resume."""


def check_usable(run_state):
    if run_state.get('version') != FORMAT_VERSION:
        raise RunStateRefused('run_state format version %r, this build reads version %d' % (run_state.get('version'), FORMAT_VERSION))
    world = parallel.world_size()
    if run_state['world_size'] != world:
        raise RunStateRefused('run_state was recorded with world size %d, this run has world size %d'
                              % (run_state['world_size'], world))


def restore(env, run_state):
    """Everything ``capture`` took, back in place: the ``u`` vectors on the device, the (K, T, F) stream, and LAST the global generator
    states, so that nothing draws between their restore and the first update.  -> this rank's 'data' entry (train.py positions the clip
    order with it; that consumes no draw).  Raises RunStateRefused before it touches anything."""
    check_usable(run_state)
    mine = run_state['ranks'][parallel.rank()]
    disc = getattr(env, 'discriminator', None)
    if disc is not None:
        modules = dict(disc.named_modules())
        for name, u in run_state['u'].items():
            modules[name].u = None if u is None else u.detach().clone().to(env.device)
    if run_state.get('guard') is not None and getattr(env, 'guard', None) is not None:
        env.guard.load_counters(run_state['guard'])
    env._ktf_rng.set_state(_rng_state_numpy(run_state['ktf']))
    np.random.set_state(_rng_state_numpy(mine['numpy']))
    torch.set_rng_state(mine['torch_cpu'].cpu())
    if mine.get('torch_cuda') is not None and env.device.type == 'cuda':
        torch.cuda.set_rng_state(mine['torch_cuda'].cpu(), env.device)
    return mine['data']


numpy_state = _rng_state_numpy


class StopRequest(object):
    """A request to end the run after the update in flight: SIGTERM, SIGINT, or the wall clock passing ``max_wall_minutes``.  The signal
    handler sets a flag and does nothing else -- no torch, no GPU, no I/O; the training loop asks ``agreed()`` once per update."""

    SIGNALS = (signal.SIGTERM, signal.SIGINT)

    def __init__(self, max_wall_minutes=None, clock=time.monotonic):
        self.flag = False
        self._clock = clock
        self._deadline = None if max_wall_minutes is None else clock() + 60.0 * float(max_wall_minutes)
        self._previous = {}

    def _handler(self, signum, frame):
        self.flag = True

    def install(self):
        for sig in self.SIGNALS:
            try:
                self._previous[sig] = signal.signal(sig, self._handler)
            except ValueError:           # not the main thread: signals cannot be handled here, the wall clock still can
                pass

    def uninstall(self):
        for sig, previous in self._previous.items():
            signal.signal(sig, previous if previous is not None else signal.SIG_DFL)
        self._previous = {}

    def requested(self):
        return self.flag or (self._deadline is not None and self._clock() >= self._deadline)

    def agreed(self):
        """True on every rank as soon as one rank has a request: one integer, max-reduced, so that all ranks stop after the same
        update."""
        mine = int(self.requested())
        if parallel.world_size() == 1:
            return bool(mine)
        import torch.distributed as dist
        on_gpu = dist.get_backend() == 'nccl'
        t = torch.tensor([mine], dtype=torch.int32, device=torch.device('cuda', torch.cuda.current_device()) if on_gpu else 'cpu')
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return bool(int(t.item()))
