"""The state digest's definition, restated in numpy: what pins ``tai_state_digest`` (csrc/state_digest.hip.inc) and the host half of
``run_state.digest_tensors``.  Written from the definition alone -- it shares no code with either.

On the raw 32-bit words of every entry (an 8-byte element is two words, low word first), uint64 arithmetic modulo 2^64:
    mix(z):  z += 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^ (z >> 31)
    E_t = sum over i of mix((i << 32) + w_t[i])
    D   = 0x243F6A8885A308D3;  for t in table order:  D = mix(D ^ E_t);  D = mix(D + n_t)
"""
import numpy as np

M64 = (1 << 64) - 1


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def words_of(entry):
    """uint32 words of a numpy array or a (host) torch tensor, in memory order."""
    if hasattr(entry, 'detach'):
        entry = entry.detach().cpu().contiguous().numpy()
    raw = np.ascontiguousarray(entry).reshape(-1).view(np.uint8)
    assert raw.size % 4 == 0
    return raw.view('<u4')


def entry_sum(words, chunk=None):
    """E_t; ``chunk`` cuts the words into pieces that are summed one by one (the result must not depend on it)."""
    words = np.asarray(words, dtype=np.uint64)
    n = words.size
    chunk = chunk or max(n, 1)
    total = 0
    with np.errstate(over='ignore'):
        for a in range(0, n, chunk):
            w = words[a:a + chunk]
            z = (np.arange(a, a + w.size, dtype=np.uint64) << np.uint64(32)) + w
            z = z + np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
            total = (total + int(np.add.reduce(z, dtype=np.uint64))) & M64
    return total


def digest(entries, chunk=None):
    d = 0x243F6A8885A308D3
    for e in entries:
        w = words_of(e)
        d = mix(d ^ entry_sum(w, chunk))
        d = mix((d + w.size) & M64)
    return d
