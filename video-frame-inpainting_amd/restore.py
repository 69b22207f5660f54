"""Repair a damaged video end to end (``restore.py``): find the damaged frames, plan the gaps, fill them with the model.

  source  ->  ``open_source``  ->  a reader and its ``present`` mask (which frames the source really holds)
  pass 1  ->  ``scan_frames`` per chunk (``tai_frame_scan``: s1, s2, sad, ndiff per frame)  ->  ``classify``  ->  ``plan_gaps``
  pass 2  ->  every frame at model resolution (``clip_pipeline.DeviceClipBuilder``: ``tai_clip_from_frames``), the ``fill`` gaps through
              ``env.forward_test`` grouped by (K, T, F), pixels by ``tai_frames_to_uint8``  ->  ``frame_%06d.png`` + ``report.json``

The flag byte of a frame (``classify``): MISSING = 1 the source has no such frame; DUPLICATE = 2 at most ``dup_share`` of its bytes differ
from the previous frame's by more than ``dup_tol`` (defaults 0, 0: an exact repeat, the signature of a dropped frame -- and of EVERY frame of
a static scene: that is the definition, not a fault of the detector); BLANK = 4 its variance is at most ``blank_var`` (default 0: a constant
frame); LISTED = 8 the caller named it.  Only the detectors asked for set their bit.  Every comparison is made in Python integers and
fractions: there is no rounding to argue about.

Partly damaged frames (opt-in: ``--detect_blocks``, ``--damage_map``).  Pass 1 also takes the four integers per block of
``--block_size`` source pixels (``block_scan``: ``tai_block_scan`` on the chunk the frame scan already uploaded).  ``classify_blocks``
raw-flags a block as ``blank`` (nb s2 - s1^2 <= block_blank_var nb^2, nb the bytes of THAT block) or ``dup`` (ndiff <= floor(block_dup_share
nb), never in frame 0); ``damage_runs`` keeps, at one block position, a maximal run of raw-flagged frames only if it has at most max_T
frames and touches neither the first nor the last frame of the video -- letterbox bars and static backgrounds are long runs or reach an
end, so they are content; a painted or concealed macroblock is a short run.  ``--damage_map`` is OR-ed in unfiltered.  A frame with
1 <= count <= floor(block_share Bh Bw) damaged blocks gets PARTIAL = 16, one with more MOSTLY = 32; the planner treats both as gap frames
(context frames are always wholly intact).  ``fill`` composites a position whose flag byte is exactly PARTIAL (``tai_damage_composite``:
the prediction where a model pixel's resize taps touch a damaged block, the pipeline's pixels elsewhere, a ramp of ``--feather`` pixels
between) and overwrites every other position whole, as before.

The planner's one rule (``plan_gaps``): maximal runs of flagged frames are gaps; two runs with exactly ONE intact frame between them are
merged into one gap over both runs and that frame (the model needs two context frames; one alone is no context) -- the frame between is
kept as it is and the prediction at its position is discarded; merging repeats until no such pair is left.  K = min(K, intact frames
immediately before the gap), F likewise behind it.  A gap is ``fill``, or it is left as the source delivered it: ``no_context_before``
(fewer than two intact frames in front, e.g. at the start of the video), ``no_context_after``, ``too_long`` (T > max_T), in this order of
precedence.  A missing frame that is not filled stays the repeat of the last present one.
"""
import json
import os
import re
from fractions import Fraction

import numpy as np
import torch

from . import _native

MISSING, DUPLICATE, BLANK, LISTED = 1, 2, 4, 8
PARTIAL, MOSTLY = 16, 32             # some / more than --block_share of the frame's blocks are damaged
DETECTORS = ('missing', 'dup', 'blank')
BLOCK_DETECTORS = ('dup', 'blank')
BLOCK_SIZES = (8, 16, 32)
MAX_FEATHER = 15
STATUSES = ('fill', 'no_context_before', 'no_context_after', 'too_long')
MIN_CONTEXT = 2                      # mcnet.py: the motion encoder takes frame differences, K >= 2 (and F >= 2 for the backward pass)


# ---------------------------------------------------------------------------------------------------------------- the scan

def _scan_numpy(v, tol):
    """The four integers of include/tai_sepconv.h (tai_frame_scan) for uint8 [n, bytes], in int64."""
    v = v.astype(np.int64)
    out = np.zeros((v.shape[0], 4), dtype=np.int64)
    out[:, 0] = v.sum(axis=1)
    out[:, 1] = (v * v).sum(axis=1)
    d = np.abs(v[1:] - v[:-1])
    out[1:, 2] = d.sum(axis=1)
    out[1:, 3] = (d > tol).sum(axis=1)
    return out


def scan_frames(frames_u8, tol=0):
    """uint8 tensor [n, ...] (contiguous; the trailing dimensions are one frame) -> int64 [n, 4] = (s1, s2, sad, ndiff) per frame, on the
    tensor's device.  A CUDA tensor goes through ``tai_frame_scan`` on the current stream (asynchronous); a CPU tensor is computed with
    numpy, the same integers, so planning and ``--dry_run`` need no GPU."""
    if not (torch.is_tensor(frames_u8) and frames_u8.dtype == torch.uint8 and frames_u8.dim() >= 2 and frames_u8.is_contiguous()):
        raise ValueError('scan_frames: expected a contiguous uint8 tensor [n, ...]')
    tol = int(tol)
    if not 0 <= tol <= 254:
        raise ValueError('scan_frames: tol must be in 0..254')
    n = int(frames_u8.shape[0])
    frame_bytes = frames_u8.numel() // max(n, 1)
    if n < 1 or frame_bytes < 1:
        raise ValueError('scan_frames: no frames, or empty frames')
    if not frames_u8.is_cuda:
        return torch.from_numpy(_scan_numpy(frames_u8.reshape(n, frame_bytes).numpy(), tol))
    need = _native.lib().tai_frame_scan_workspace_bytes(n, frame_bytes)
    if need < 0:
        raise ValueError('scan_frames: %d frames of %d bytes are refused by tai_frame_scan' % (n, frame_bytes))
    stats = torch.empty(n, 4, dtype=torch.int64, device=frames_u8.device)
    workspace = torch.empty(need // 8, dtype=torch.int64, device=frames_u8.device)
    _native.launch('tai_frame_scan', frames_u8.device, frames_u8, n, frame_bytes, tol, stats, workspace)
    return stats


def _block_scan_numpy(v, bs, tol):
    """The four integers of include/tai_sepconv.h (tai_block_scan) for uint8 [n, h, w, c], in int64 [n, Bh, Bw, 4].  The frame is padded
    with zeros up to whole blocks: a zero adds nothing to s1 and s2, and a zero against a zero nothing to sad and ndiff."""
    n, h, w, c = v.shape
    Bh, Bw = -(-h // bs), -(-w // bs)
    p = np.zeros((n, Bh * bs, Bw * bs, c), dtype=np.int64)
    p[:, :h, :w] = v
    cells = lambda a: a.reshape(a.shape[0], Bh, bs, Bw, bs, c).sum(axis=(2, 4, 5))
    out = np.zeros((n, Bh, Bw, 4), dtype=np.int64)
    out[..., 0] = cells(p)
    out[..., 1] = cells(p * p)
    d = np.abs(p[1:] - p[:-1])
    out[1:, ..., 2] = cells(d)
    out[1:, ..., 3] = cells((d > tol).astype(np.int64))
    return out


def block_scan(frames_u8, bs, tol=0):
    """uint8 tensor [n, h, w, c] (contiguous) -> int64 [n, Bh, Bw, 4] = (s1, s2, sad, ndiff) per block of bs x bs pixels, on the tensor's
    device.  A CUDA tensor goes through ``tai_block_scan`` on the current stream (asynchronous); a CPU tensor is computed with numpy,
    the same integers, so ``--dry_run`` needs no GPU."""
    if not (torch.is_tensor(frames_u8) and frames_u8.dtype == torch.uint8 and frames_u8.dim() == 4 and frames_u8.is_contiguous()):
        raise ValueError('block_scan: expected a contiguous uint8 tensor [n, h, w, c]')
    bs, tol = int(bs), int(tol)
    n, h, w, c = (int(k) for k in frames_u8.shape)
    if bs not in BLOCK_SIZES or not 0 <= tol <= 254 or not 1 <= c <= 4 or min(n, h, w) < 1:
        raise ValueError('block_scan: needs bs in %s, tol in 0..254, c in 1..4 and at least one non-empty frame' % (BLOCK_SIZES,))
    if not frames_u8.is_cuda:
        return torch.from_numpy(_block_scan_numpy(frames_u8.numpy(), bs, tol))
    need = _native.lib().tai_block_scan_workspace_bytes(n, h, w, c, bs)
    if need < 0:
        raise ValueError('block_scan: %d frames of %d x %d x %d are refused by tai_block_scan' % (n, h, w, c))
    stats = torch.empty(n, -(-h // bs), -(-w // bs), 4, dtype=torch.int64, device=frames_u8.device)
    workspace = torch.empty(need // 8, dtype=torch.int64, device=frames_u8.device) if need else None
    _native.launch('tai_block_scan', frames_u8.device, frames_u8, n, h, w, c, bs, tol, stats, workspace)
    return stats


# ---------------------------------------------------------------------------------------------------------------- flags

def parse_detect(text):
    """'missing,dup,blank' -> the set of detectors; '' or 'none' -> none."""
    names = [s.strip() for s in str(text).split(',') if s.strip()]
    if names == ['none']:
        names = []
    bad = [s for s in names if s not in DETECTORS]
    if bad:
        raise ValueError('--detect: unknown detector %r (choose from %s)' % (bad[0], ', '.join(DETECTORS)))
    return frozenset(names)


def parse_gaps(text, n_frames):
    """'a-b,c-d' (0-based, inclusive; 'a' alone is 'a-a') -> bool [n_frames].  A reversed range, a frame past the end and anything that
    is not a number are refused."""
    listed = np.zeros(n_frames, dtype=bool)
    for piece in [s.strip() for s in (text or '').split(',') if s.strip()]:
        m = re.fullmatch(r'(\d+)(?:-(\d+))?', piece)
        if not m:
            raise ValueError('--gaps: %r is not a-b with 0-based frame numbers' % piece)
        a = int(m.group(1))
        b = int(m.group(2)) if m.group(2) is not None else a
        if b < a:
            raise ValueError('--gaps: the range %r is reversed' % piece)
        if b >= n_frames:
            raise ValueError('--gaps: the range %r reaches past the last frame (%d)' % (piece, n_frames - 1))
        listed[a:b + 1] = True
    return listed


def classify(stats, frame_bytes, present, listed, detect, dup_share=0.0, blank_var=0.0):
    """stats [n, 4] (``scan_frames``), the source's ``present`` mask, the caller's ``listed`` mask -> uint8 [n] of flag bytes."""
    rows = np.asarray(stats.cpu() if torch.is_tensor(stats) else stats).tolist()
    n_bytes = int(frame_bytes)
    detect = frozenset(detect)
    if not detect <= set(DETECTORS):
        raise ValueError('classify: detect must be a subset of %s' % (DETECTORS,))
    share, var = Fraction(dup_share), Fraction(blank_var)
    if not 0 <= share <= 1 or var < 0:
        raise ValueError('classify: dup_share must be in [0, 1] and blank_var >= 0')
    dup_max = (share * n_bytes).__floor__()
    flags = np.zeros(len(rows), dtype=np.uint8)
    for i, (s1, s2, _, ndiff) in enumerate(rows):
        f = 0
        if 'missing' in detect and not present[i]:
            f |= MISSING
        if 'dup' in detect and i >= 1 and ndiff <= dup_max:
            f |= DUPLICATE
        if 'blank' in detect and n_bytes * s2 - s1 * s1 <= var * n_bytes * n_bytes:
            f |= BLANK
        if listed is not None and listed[i]:
            f |= LISTED
        flags[i] = f
    return flags


# ---------------------------------------------------------------------------------------------------------------- damaged blocks

def parse_detect_blocks(text):
    """'dup,blank' -> the set of block detectors; '' or 'none' -> none (the feature is off unless --damage_map is given)."""
    names = [s.strip() for s in str(text or '').split(',') if s.strip()]
    if names == ['none']:
        names = []
    bad = [s for s in names if s not in BLOCK_DETECTORS]
    if bad:
        raise ValueError('--detect_blocks: unknown detector %r (choose from %s)' % (bad[0], ', '.join(BLOCK_DETECTORS)))
    return frozenset(names)


def classify_blocks(bstats, h, w, c, bs, detect, block_dup_share=0.0, block_blank_var=0.0):
    """bstats [n, Bh, Bw, 4] (``block_scan`` of frames [h, w, c]) -> bool [n, Bh, Bw]: the RAW flags, before ``damage_runs``."""
    rows = np.asarray(bstats.cpu() if torch.is_tensor(bstats) else bstats)
    detect = frozenset(detect)
    if not detect <= set(BLOCK_DETECTORS):
        raise ValueError('classify_blocks: detect must be a subset of %s' % (BLOCK_DETECTORS,))
    share, var = Fraction(block_dup_share), Fraction(block_blank_var)
    if not 0 <= share <= 1 or var < 0:
        raise ValueError('classify_blocks: block_dup_share must be in [0, 1] and block_blank_var >= 0')
    n, Bh, Bw = rows.shape[:3]
    if (Bh, Bw) != (-(-h // bs), -(-w // bs)) or rows.shape[3] != 4:
        raise ValueError('classify_blocks: statistics of shape %s do not belong to frames of %d x %d in blocks of %d' % (rows.shape, h, w, bs))
    raw = np.zeros((n, Bh, Bw), dtype=bool)
    for by in range(Bh):
        for bx in range(Bw):
            nb = (min(h, (by + 1) * bs) - by * bs) * (min(w, (bx + 1) * bs) - bx * bs) * c        # the bytes of THIS block
            dup_max, var_max = (share * nb).__floor__(), var * nb * nb
            for i, (s1, s2, _, ndiff) in enumerate(rows[:, by, bx].tolist()):
                raw[i, by, bx] = ('dup' in detect and i >= 1 and ndiff <= dup_max) or ('blank' in detect and nb * s2 - s1 * s1 <= var_max)
    return raw


def damage_runs(raw, max_T):
    """The rule that tells damage from content: raw flags bool [n, Bh, Bw] -> damaged bool [n, Bh, Bw].  Along time, at one block
    position, a maximal run of raw-flagged frames is damage only if it has at most ``max_T`` frames and touches neither frame 0 nor
    frame n - 1."""
    raw = np.asarray(raw, dtype=bool)
    n = raw.shape[0]
    out = np.zeros_like(raw)
    for by, bx in zip(*np.nonzero(raw.any(axis=0))):
        col, i = raw[:, by, bx].tolist(), 0
        while i < n:
            if not col[i]:
                i += 1
                continue
            j = i
            while j + 1 < n and col[j + 1]:
                j += 1
            if j - i + 1 <= max_T and i > 0 and j < n - 1:
                out[i:j + 1, by, bx] = True
            i = j + 1
    return out


def load_damage_map(path, shape):
    """--damage_map FILE.npy: uint8 or bool [n, Bh, Bw], non-zero = damaged -> bool array; a wrong shape or type is refused."""
    m = np.load(path, allow_pickle=False)
    if m.dtype not in (np.uint8, np.bool_):
        raise ValueError('--damage_map: %s holds %s, expected uint8 or bool' % (path, m.dtype))
    if tuple(m.shape) != tuple(shape):
        raise ValueError('--damage_map: %s has shape %s, the video has %s blocks [n, Bh, Bw]' % (path, tuple(m.shape), tuple(shape)))
    return m != 0


def block_flags(damaged, block_share=0.5):
    """damaged bool [n, Bh, Bw] -> uint8 [n]: PARTIAL for 1 <= count <= floor(block_share Bh Bw) damaged blocks, MOSTLY above that."""
    damaged = np.asarray(damaged, dtype=bool)
    share = Fraction(block_share)
    if not 0 <= share <= 1:
        raise ValueError('--block_share must be in [0, 1]')
    most = (share * damaged.shape[1] * damaged.shape[2]).__floor__()
    counts = damaged.reshape(damaged.shape[0], -1).sum(axis=1).tolist()
    return np.array([0 if k == 0 else (PARTIAL if k <= most else MOSTLY) for k in counts], dtype=np.uint8)


def tap_tables(n_in, n_out):
    """int32 (i0, i1), each [n_out]: the source indices that ``data.resize_bilinear`` / the clip kernel's ``tap`` multiply by a NON-ZERO
    weight at output index i (i1 = i0 where the fraction is 0, so also for the identity).  The same float64 expression as theirs."""
    src = (np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / float(n_out)) - 0.5
    fl = np.floor(src)
    i0 = np.clip(fl.astype(np.int64), 0, n_in - 1)
    i1 = np.where(src - fl > 0, np.clip(fl.astype(np.int64) + 1, 0, n_in - 1), i0)
    return i0.astype(np.int32), i1.astype(np.int32)


def composite_device(pred, src, items, blocks, taps, bs, h, w, feather, rgb):
    """One ``tai_damage_composite`` launch on the current stream.  ``pred`` / ``src``: fp32 CUDA tensors whose storage holds the frames
    [C, Hs, Ws] the items point into (element offsets from the tensors' first element); ``items``: rows (pred offset, src offset, map, output
    frame); ``blocks``: uint8 [n_maps, Bh, Bw]; ``taps``: (r0, r1, c0, c1) int32 CUDA tensors.  -> uint8 CUDA [n_out, h, w, C]."""
    C, Hs, Ws = (int(k) for k in src.shape[-3:])
    table_host = torch.tensor(items, dtype=torch.int64).reshape(-1, 4)
    table = table_host.to(pred.device)
    blocks = torch.as_tensor(blocks).to(device=pred.device, dtype=torch.uint8).contiguous()
    n_maps, Bh, Bw = (int(k) for k in blocks.shape)
    n_out = int(table_host[:, 3].max()) + 1
    out = torch.empty(n_out, h, w, C, dtype=torch.uint8, device=pred.device)
    elems = lambda t: t.untyped_storage().nbytes() // 4 - t.storage_offset()
    _native.launch('tai_damage_composite', pred.device, pred, elems(pred), src, elems(src), table, table_host.data_ptr(), table_host.shape[0],
                   blocks, n_maps, Bh, Bw, int(bs), taps[0], taps[1], taps[2], taps[3], out, n_out, C, Hs, Ws, int(h), int(w), int(feather),
                   int(bool(rgb)))
    return out


# ---------------------------------------------------------------------------------------------------------------- the planner

def plan_gaps(flags, K, F, max_T):
    """flag bytes -> the gaps in order, each a dict: start, T (the span, kept frames between merged runs included), K, F, status, and
    positions = the flagged frames of the span (what a filled gap writes)."""
    flagged = [bool(f) for f in np.asarray(flags).tolist()]
    n = len(flagged)
    runs, i = [], 0
    while i < n:
        if flagged[i]:
            j = i
            while j + 1 < n and flagged[j + 1]:
                j += 1
            runs.append([i, j])
            i = j + 1
        else:
            i += 1
    merged = []
    for run in runs:                      # left to right: a merged gap is compared with the next run again, so chains close up
        if merged and run[0] - merged[-1][1] == 2:
            merged[-1][1] = run[1]
        else:
            merged.append(list(run))
    gaps = []
    for g, (a, b) in enumerate(merged):
        before = a - (merged[g - 1][1] + 1 if g > 0 else 0)
        after = (merged[g + 1][0] if g + 1 < len(merged) else n) - (b + 1)
        T = b - a + 1
        if before < MIN_CONTEXT:
            status = 'no_context_before'
        elif after < MIN_CONTEXT:
            status = 'no_context_after'
        elif T > max_T:
            status = 'too_long'
        else:
            status = 'fill'
        gaps.append({'start': a, 'T': T, 'K': min(int(K), before), 'F': min(int(F), after), 'status': status,
                     'positions': [p for p in range(a, b + 1) if flagged[p]]})
    return gaps


# ---------------------------------------------------------------------------------------------------------------- sources

_IMAGE_EXT = ('.png', '.jpg', '.jpeg', '.bmp')


class _Delivered(object):
    """A reader over ALL frame positions of a source: a frame the source does not hold is delivered as the last present one before
    it (what a player shows), or as the first present one when none precedes it."""

    def __init__(self, read, present, name):
        self._read, self.present, self._filename = read, np.asarray(present, dtype=bool), name
        if not self.present.any():
            raise IOError('%s: no frames' % name)
        first = int(np.argmax(self.present))
        self._from = np.maximum.accumulate(np.where(self.present, np.arange(len(self.present)), -1))
        self._from[self._from < 0] = first

    def get_length(self):
        return len(self.present)

    def get_data(self, index):
        if not 0 <= index < len(self.present):
            raise IndexError('frame %d of %d in %s' % (index, len(self.present), self._filename))
        return self._read(int(self._from[index]))


def _numbered_files(path):
    """{number: file name} when every image file of the directory ends in a number before its extension and no number repeats;
    else None (plain order, nothing missing)."""
    files = sorted(f for f in os.listdir(path) if f.lower().endswith(_IMAGE_EXT))
    if not files:
        raise IOError('%s: no image files' % path)
    numbers = {}
    for f in files:
        m = re.search(r'(\d+)\.[^.]+$', f)
        if not m or int(m.group(1)) in numbers:
            return None
        numbers[int(m.group(1))] = f
    return numbers


def open_source(path):
    """-> (reader, present): a reader with ``get_length()`` / ``get_data(i) -> [h, w, 3] uint8 RGB`` over every frame POSITION of the
    source and the bool mask of the positions it really holds.  A directory whose image names all end in a number is indexed by that number
    minus the smallest (absent numbers are missing frames); an AVI's zero-length chunks are missing frames; arrays and every other source
    have none."""
    from .data import open_frame_source
    from .video_io import AviVideo
    if os.path.isdir(path):
        numbers = _numbered_files(path)
        if numbers is not None:
            from PIL import Image
            lo, hi = min(numbers), max(numbers)
            present = np.array([k in numbers for k in range(lo, hi + 1)])

            def read(i):
                with Image.open(os.path.join(path, numbers[lo + i])) as img:
                    return np.asarray(img.convert('RGB'))
            return _Delivered(read, present, path), present
    reader = open_frame_source(path)
    if reader is None:
        raise IOError('%s: cannot be opened as a video' % path)
    n = reader.get_length()
    present = np.ones(n, dtype=bool)
    if isinstance(reader, AviVideo):
        present[reader.dropped_frames()] = False
    return _Delivered(reader.get_data, present, path), present


# ---------------------------------------------------------------------------------------------------------------- the driver

class Restorer(object):
    """Two passes over one source (decoding the context frames a second time is accepted: a decoded video rarely fits the host twice,
    the chunk in hand always does).  ``env`` may be None for a dry run (scan, plan, report)."""

    def __init__(self, env, opt):
        self.env, self.opt = env, opt
        self.detect = parse_detect(opt.detect)
        self.max_T = opt.T if getattr(opt, 'max_T', None) is None else int(opt.max_T)
        self.chunk = max(1, int(opt.chunk_frames))
        if not 0 <= int(opt.dup_tol) <= 254:
            raise ValueError('--dup_tol must be in 0..254')
        if min(opt.K, opt.F) < MIN_CONTEXT or opt.T < 1 or self.max_T < 1:
            raise ValueError('restore: needs K, F >= %d and T, max_T >= 1' % MIN_CONTEXT)
        # partly damaged frames: off unless --detect_blocks or --damage_map is given; then nothing below differs from before
        self.detect_blocks = parse_detect_blocks(getattr(opt, 'detect_blocks', ''))
        self.damage_map = getattr(opt, 'damage_map', None) or None
        self.blocks_on = bool(self.detect_blocks) or self.damage_map is not None
        self.block_size, self.feather = int(getattr(opt, 'block_size', 16)), int(getattr(opt, 'feather', 4))
        if self.blocks_on and (self.block_size not in BLOCK_SIZES or not 0 <= self.feather <= MAX_FEATHER):
            raise ValueError('--block_size must be one of %s and --feather in 0..%d' % (BLOCK_SIZES, MAX_FEATHER))
        self.block_stats = self.damaged = self.flags = self.source_size = None

    def _chunks(self, reader):
        """(first frame, uint8 [m, h, w, 3]) over the source, in order; all frames of a source share one size."""
        n, shape = reader.get_length(), None
        for a in range(0, n, self.chunk):
            frames = [np.asarray(reader.get_data(i)) for i in range(a, min(a + self.chunk, n))]
            for f in frames:
                if f.ndim != 3 or f.shape[2] != 3 or f.dtype != np.uint8 or (shape is not None and f.shape != shape):
                    raise IOError('restore: a frame is not [h, w, 3] uint8 of the size of the first one: %s %s' % (f.shape, f.dtype))
                shape = f.shape
            yield a, torch.from_numpy(np.stack(frames))

    def scan(self, reader, device):
        """Pass 1 -> int64 [n, 4] on the host, and the bytes of a frame.  Each chunk is placed behind the previous chunk's last frame, so
        the pair statistics cross the chunk boundaries."""
        n, tol = reader.get_length(), int(self.opt.dup_tol)
        rows, buf, frame_bytes = [], None, None
        brows = [] if self.detect_blocks else None                           # one more launch per chunk, on the same buffer
        for a, frames in self._chunks(reader):
            m = frames.shape[0]
            if buf is None:
                frame_bytes = frames[0].numel()
                self.source_size = (int(frames.shape[1]), int(frames.shape[2]))
                buf = torch.empty((self.chunk + 1,) + tuple(frames.shape[1:]), dtype=torch.uint8, device=device)
            buf[1:m + 1].copy_(frames, non_blocking=True)
            if brows is not None:
                part = block_scan(buf[1:m + 1] if a == 0 else buf[:m + 1], self.block_size, tol)
                brows.append((part if a == 0 else part[1:]).cpu())
            if a == 0:
                rows.append(scan_frames(buf[1:m + 1], tol).cpu())
            else:
                rows.append(scan_frames(buf[:m + 1], tol)[1:].cpu())        # .cpu() also orders the next chunk's upload behind this scan
            buf[0].copy_(buf[m])
        stats = torch.cat(rows)
        assert stats.shape == (n, 4)
        self.block_stats = torch.cat(brows) if brows is not None else None
        return stats, frame_bytes

    def plan(self, reader, present, device):
        stats, frame_bytes = self.scan(reader, device)
        listed = parse_gaps(getattr(self.opt, 'gaps', None), reader.get_length())
        flags = classify(stats, frame_bytes, present, listed, self.detect, self.opt.dup_share, self.opt.blank_var)
        if self.blocks_on:
            flags = flags | block_flags(self.damaged_blocks(reader.get_length()), self.opt.block_share)
        self.flags = flags
        return stats, flags, plan_gaps(flags, self.opt.K, self.opt.F, self.max_T)

    def damaged_blocks(self, n):
        """-> bool [n, Bh, Bw] (kept in ``self.damaged``): the detectors' raw flags through the run rule, OR the caller's map."""
        (h, w), bs = self.source_size, self.block_size
        damaged = np.zeros((n, -(-h // bs), -(-w // bs)), dtype=bool)
        if self.detect_blocks:
            raw = classify_blocks(self.block_stats, h, w, 3, bs, self.detect_blocks, self.opt.block_dup_share, self.opt.block_blank_var)
            damaged |= damage_runs(raw, self.max_T)
        if self.damage_map is not None:
            damaged |= load_damage_map(self.damage_map, damaged.shape)
        self.damaged = damaged
        return damaged

    def model_frames(self, reader):
        """Pass 2's way in -> fp32 [n, C, H + pad, W + pad] on the device: every frame as the models take it."""
        from . import clip_pipeline
        opt = self.opt
        builder = clip_pipeline.DeviceClipBuilder(opt.c_dim, opt.image_size, opt.padding_size, self.env.device)
        out = []
        for _, frames in self._chunks(reader):
            batch = {'items': [{'frames': frames, 'mirror': False}], 'B': 1, 'T': int(frames.shape[0])}
            out.append(builder.build(batch)[0])
        return torch.cat(out)

    def fill(self, video, gaps, out_u8):
        """Run the ``fill`` gaps through the model, grouped by (K, T, F) in batches of at most --batch_size, and write their pixels
        into ``out_u8`` [n, h, w, C] at the gaps' positions.  A position whose flag byte is exactly PARTIAL is composited
        (``tai_damage_composite``, one launch per batch); every other position is overwritten whole."""
        from . import clip_pipeline
        opt, env = self.opt, self.env
        (h, w), rgb = opt.image_size, opt.c_dim == 3
        partial = set(np.nonzero(self.flags == PARTIAL)[0].tolist()) if self.blocks_on else set()
        taps = None
        groups = {}
        for g in gaps:
            if g['status'] == 'fill':
                groups.setdefault((g['K'], g['T'], g['F']), []).append(g)
        for (K, T, F), members in sorted(groups.items()):
            for i in range(0, len(members), max(1, int(opt.batch_size))):
                batch = members[i:i + max(1, int(opt.batch_size))]
                preceding = torch.stack([video[g['start'] - K:g['start']] for g in batch])
                following = torch.stack([video[g['start'] + T:g['start'] + T + F] for g in batch])
                env.set_test_inputs(preceding, following)
                env.T = T
                env.eval()
                env.forward_test()
                pred = env.gen_output['pred']                                                     # [B, T, C, Hs, Ws]
                where = [(b, p) for b, g in enumerate(batch) for p in g['positions']]
                if any(p not in partial for _, p in where):
                    pixels = clip_pipeline.to_uint8_host(pred, h, w, rgb)                         # [B, T, h, w, C]
                    for b, p in where:
                        if p not in partial:
                            out_u8[p] = pixels[b, p - batch[b]['start']]
                mine = [(b, p) for b, p in where if p in partial]
                if mine:
                    # one launch for the batch's partly damaged frames; pred and video are read in place, by element offset
                    if taps is None:
                        taps = [torch.from_numpy(t).to(env.device) for n_in, n_out in zip(self.source_size, (h, w))
                                for t in tap_tables(n_in, n_out)]
                    if pred.dtype != torch.float32 or not pred[0, 0].is_contiguous():
                        pred = pred.float().contiguous()
                    if not video[0].is_contiguous():
                        video = video.contiguous()
                    items = [[b * pred.stride(0) + (p - batch[b]['start']) * pred.stride(1), p * video.stride(0), k, k]
                             for k, (b, p) in enumerate(mine)]
                    done = composite_device(pred, video, items, self.damaged[[p for _, p in mine]].astype(np.uint8), taps, self.block_size,
                                            h, w, self.feather, rgb).cpu().numpy()
                    for k, (_, p) in enumerate(mine):
                        out_u8[p] = done[k]

    def run(self, path, output_dir):
        from . import clip_pipeline
        opt = self.opt
        reader, present = open_source(path)
        dry = bool(getattr(opt, 'dry_run', False))
        device = torch.device('cpu') if dry else self.env.device
        stats, flags, gaps = self.plan(reader, present, device)
        os.makedirs(output_dir, exist_ok=True)
        if not dry:
            from PIL import Image
            (h, w), rgb = opt.image_size, opt.c_dim == 3
            video = self.model_frames(reader)
            out_u8 = np.concatenate([clip_pipeline.to_uint8_host(video[a:a + self.chunk], h, w, rgb)
                                     for a in range(0, video.shape[0], self.chunk)])
            self.fill(video, gaps, out_u8)
            for i, f in enumerate(out_u8):
                Image.fromarray(f[:, :, 0] if f.shape[2] == 1 else f).save(os.path.join(output_dir, 'frame_%06d.png' % i))
        report = {
            'input': path, 'n_frames': int(len(flags)), 'dry_run': dry,
            'settings': {'K': opt.K, 'T': opt.T, 'F': opt.F, 'max_T': self.max_T, 'detect': sorted(self.detect),
                         'gaps': getattr(opt, 'gaps', None) or '', 'dup_tol': int(opt.dup_tol), 'dup_share': float(opt.dup_share),
                         'blank_var': float(opt.blank_var), 'chunk_frames': self.chunk, 'batch_size': int(opt.batch_size),
                         'c_dim': opt.c_dim, 'image_size': list(opt.image_size), 'padding_size': list(opt.padding_size)},
            'frames': [{'index': i, 's1': r[0], 's2': r[1], 'sad': r[2], 'ndiff': r[3], 'flags': int(flags[i])}
                       for i, r in enumerate(stats.tolist())],
            'gaps': [{k: g[k] for k in ('start', 'T', 'K', 'F', 'status', 'positions')} for g in gaps],
        }
        if self.blocks_on:                   # with the feature off the report has exactly the keys it had before
            report['settings'].update({'detect_blocks': sorted(self.detect_blocks), 'block_size': self.block_size, 'feather': self.feather,
                                       'block_share': float(opt.block_share), 'block_dup_share': float(opt.block_dup_share),
                                       'block_blank_var': float(opt.block_blank_var), 'damage_map': self.damage_map or ''})
            for f in report['frames']:
                f['blocks'] = [[int(by), int(bx)] for by, bx in zip(*np.nonzero(self.damaged[f['index']]))]
            for g in report['gaps']:
                g['composited'] = [p for p in g['positions'] if g['status'] == 'fill' and int(flags[p]) == PARTIAL]
        with open(os.path.join(output_dir, 'report.json'), 'w') as f:
            json.dump(report, f, indent=1)
        return report
