"""The opt-in device clip pipeline (``--device_preprocess``): the host decodes and hands over raw uint8 frames, the GPU does the
rest -- bit-equal to the host path (data._ClipReader.clip on the way in, util.frames_to_uint8 on the way out), so the flag changes
throughput and nothing else.

  datasets with ``raw=True``  ->  ``collate_raw``  ->  ``DeviceClipBuilder.build``  ->  [B, T, C, H + pad, W + pad] fp32 on the device
  a predicted tensor          ->  ``to_uint8_host``                                  ->  uint8 [..., h, w, C] pixels on the host

A packed batch is ONE uint8 tensor: a header of N = B T frame descriptors (four int64 each: byte offset of the frame behind the
header, source height, source width, flags with bit 0 = mirror; ``HEADER_ALIGN``-byte aligned), then the frames [h, w, 3] of every
clip in playback order.  Frames of one batch may differ in source size.  ``collate_raw`` never touches CUDA (DataLoader workers run
it); the builder owns the pinned staging buffers, in the main process, and with a loader that has no workers (``collate_items``)
it packs straight into them.

Items that carry an augmentation record (``'aug'``; train.py --aug_*; data.ClipAugment) are packed by ``pack_clips_aug`` instead: the
header holds ``AUG_DESC_INTS`` int64 per frame (offset, h, w, flags with bit 1 = vflip, then the crop window top, left, ch, cw and the
index of the frame's level table), a section of fp32 [n_tables][4][256] level tables follows it (``augment_level_tables``: one table per
clip, one per frame with flicker), then the frames; the batch gains ``'n_tables'`` and the builder launches ``tai_clip_from_frames_aug``
for it.  Still ONE upload per batch, and nothing changes for a batch without records.
"""
import numpy as np
import torch

from . import _native
from .util import _GRAY_BGR, fore_transform

HEADER_ALIGN = 256
DESC_INTS = 4                     # int64 per frame: offset, h, w, flags
FLAG_MIRROR = 1
AUG_DESC_INTS = 9                 # int64 per frame of an augmented batch: offset, h, w, flags, top, left, ch, cw, table index
FLAG_VFLIP = 2
TABLE_BYTES = 4 * 256 * 4         # one fp32 [4][256] level table


def level_tables():
    """float32 [4, 256]: row 0 the value the host path gives a uint8 level (``.float().div(255)``, then ``fore_transform``), rows 1-3
    the three products of ``util.bgr2gray`` -- the host's own torch expressions, so the kernel's lookups are exact by construction."""
    level = fore_transform(torch.arange(256, dtype=torch.int64).to(torch.uint8).float().div(255))
    b, g, r = _GRAY_BGR
    return torch.stack([level, b * level, g * level, r * level]).contiguous()


def augment_level_tables(gamma=1.0, gain=1.0, offsets=(0.0,)):
    """float32 [len(offsets), 4, 256]: the level tables of frames whose levels go through x ** gamma, then gain about 0.5, then an
    additive offset (include/tai_sepconv.h, tai_clip_from_frames_aug): float64 throughout, clamped to [0, 1], rounded ONCE to float32 and
    only then mapped by the host path's own torch expressions, as ``level_tables`` forms its rows.  Neutral parameters (1, 1, 0) give
    ``level_tables()`` bit for bit."""
    x = np.arange(256, dtype=np.float64) / 255.0
    if gamma != 1.0:
        x = x ** np.float64(gamma)
    x = (x - 0.5) * np.float64(gain) + 0.5
    x = x[None, :] + np.asarray(offsets, dtype=np.float64)[:, None]
    x = np.minimum(np.maximum(x, 0.0), 1.0)
    level = fore_transform(torch.from_numpy(x.astype(np.float32)))
    b, g, r = _GRAY_BGR
    return torch.stack([level, b * level, g * level, r * level], dim=1).contiguous()


def tables_of_record(aug):
    """The level tables of one clip's augmentation record (data.ClipAugment.draw): [1, 4, 256] without flicker, [T, 4, 256] with it
    (the offset of the frame at playback position t is offset + flicker[t])."""
    flicker = aug['flicker']
    return augment_level_tables(aug['gamma'], aug['gain'], [aug['offset']] if flicker is None else [aug['offset'] + e for e in flicker])


def header_bytes(n_frames):
    return -(-n_frames * DESC_INTS * 8 // HEADER_ALIGN) * HEADER_ALIGN


def _as_clips(clips):
    clips = [c if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c)) for c in clips]
    if not clips:
        raise ValueError('pack_clips: an empty batch')
    T = clips[0].shape[0]
    for c in clips:
        if c.dtype != torch.uint8 or c.dim() != 4 or c.shape[3] != 3 or c.shape[0] != T or c.numel() == 0:
            raise ValueError('pack_clips: expected uint8 [%d, h, w, 3] clips, found %s %s' % (T, tuple(c.shape), c.dtype))
    return clips, T


def packed_bytes(clips):
    """Bytes of the packed form of these clips (header + frames)."""
    return header_bytes(len(clips) * clips[0].shape[0]) + sum(int(np.prod(c.shape)) for c in clips)


def pack_clips(clips, mirrors, out=None):
    """clips: uint8 tensors / arrays [T, h_i, w_i, 3] (one T); mirrors: one bool per clip -> the packed uint8 tensor; written into
    ``out`` (a uint8 buffer of at least ``packed_bytes``; a view of its head is returned) when given."""
    clips, T = _as_clips(clips)
    n = len(clips) * T
    head = header_bytes(n)
    need = head + sum(c.numel() for c in clips)
    if out is None:
        packed = torch.empty(need, dtype=torch.uint8)
    else:
        if out.dtype != torch.uint8 or out.dim() != 1 or out.numel() < need or not out.is_contiguous():
            raise ValueError('pack_clips: out must be a contiguous uint8 buffer of at least %d bytes' % need)
        packed = out[:need]
    packed[:head].zero_()
    table = packed[:n * DESC_INTS * 8].view(torch.int64).view(n, DESC_INTS)
    offset = 0
    for i, (c, mirror) in enumerate(zip(clips, mirrors)):
        _, h, w, _ = c.shape
        rows = table[i * T:(i + 1) * T]
        rows[:, 0] = offset + torch.arange(T, dtype=torch.int64) * (h * w * 3)
        rows[:, 1], rows[:, 2], rows[:, 3] = h, w, FLAG_MIRROR if mirror else 0
        packed[head + offset:head + offset + c.numel()].view(c.shape).copy_(c)
        offset += c.numel()
    return packed


def aug_header_bytes(n_frames):
    return -(-n_frames * AUG_DESC_INTS * 8 // HEADER_ALIGN) * HEADER_ALIGN


def _aug_tables(clips, augs, T):
    if len(augs) != len(clips):
        raise ValueError('pack_clips_aug: %d clips, %d augmentation records' % (len(clips), len(augs)))
    for a in augs:
        if a['flicker'] is not None and len(a['flicker']) != T:
            raise ValueError('pack_clips_aug: a clip of %d frames carries %d flicker offsets' % (T, len(a['flicker'])))
    return [tables_of_record(a) for a in augs]


def aug_packed_bytes(clips, augs):
    """Bytes of the augmented packed form of these clips (header + level tables + frames)."""
    T = clips[0].shape[0]
    n_tables = sum(1 if a['flicker'] is None else len(a['flicker']) for a in augs)
    return aug_header_bytes(len(clips) * T) + n_tables * TABLE_BYTES + sum(int(np.prod(c.shape)) for c in clips)


def pack_clips_aug(clips, mirrors, augs, out=None):
    """``pack_clips`` for clips with augmentation records (``augs``: one per clip, with 'window' = (top, left, ch, cw), 'vflip', 'gamma',
    'gain', 'offset', 'flicker') -> (the packed uint8 tensor, n_tables): header of ``AUG_DESC_INTS`` int64 per frame, the level tables,
    the frames.  No CUDA call."""
    clips, T = _as_clips(clips)
    tables = _aug_tables(clips, augs, T)
    n = len(clips) * T
    head = aug_header_bytes(n)
    n_tables = sum(t.shape[0] for t in tables)
    first = head + n_tables * TABLE_BYTES
    need = first + sum(c.numel() for c in clips)
    if out is None:
        packed = torch.empty(need, dtype=torch.uint8)
    else:
        if out.dtype != torch.uint8 or out.dim() != 1 or out.numel() < need or not out.is_contiguous():
            raise ValueError('pack_clips_aug: out must be a contiguous uint8 buffer of at least %d bytes' % need)
        packed = out[:need]
    packed[:head].zero_()
    table = packed[:n * AUG_DESC_INTS * 8].view(torch.int64).view(n, AUG_DESC_INTS)
    section = packed[head:first].view(torch.float32).view(n_tables, 4, 256)
    offset, k = 0, 0
    for i, (c, mirror, aug, tab) in enumerate(zip(clips, mirrors, augs, tables)):
        _, h, w, _ = c.shape
        top, left, ch, cw = (int(v) for v in aug['window'])
        if not (0 <= top and 0 <= left and 1 <= ch and 1 <= cw and top + ch <= h and left + cw <= w):
            raise ValueError('pack_clips_aug: the window %r lies outside a %d x %d frame' % ((top, left, ch, cw), h, w))
        rows = table[i * T:(i + 1) * T]
        rows[:, 0] = offset + torch.arange(T, dtype=torch.int64) * (h * w * 3)
        rows[:, 1], rows[:, 2] = h, w
        rows[:, 3] = (FLAG_MIRROR if mirror else 0) | (FLAG_VFLIP if aug['vflip'] else 0)
        rows[:, 4], rows[:, 5], rows[:, 6], rows[:, 7] = top, left, ch, cw
        rows[:, 8] = k + (torch.arange(T, dtype=torch.int64) if aug['flicker'] is not None else 0)
        section[k:k + tab.shape[0]].copy_(tab)
        k += tab.shape[0]
        packed[first + offset:first + offset + c.numel()].view(c.shape).copy_(c)
        offset += c.numel()
    return packed, n_tables


def _augs_of(items):
    """The augmentation records of a batch's items, or None when it carries none (all items of a batch come from one dataset)."""
    augs = [it.get('aug') for it in items]
    if all(a is None for a in augs):
        return None
    if any(a is None for a in augs):
        raise ValueError('a batch mixes items with and without an augmentation record')
    return augs


def collate_raw(items):
    """DataLoader ``collate_fn`` for raw-mode items -> ``{'packed': uint8 [bytes], 'B': int, 'T': int, 'clip_label': [str]}``; items with
    an augmentation record give the augmented packed form and ``'n_tables'`` beside it (the level tables are built here, in the worker).
    Ordinary memory, no CUDA call: this is what DataLoader workers run."""
    augs = _augs_of(items)
    if augs is not None:
        packed, n_tables = pack_clips_aug([it['frames'] for it in items], [it['mirror'] for it in items], augs)
        return {'packed': packed, 'n_tables': n_tables, 'B': len(items), 'T': int(items[0]['frames'].shape[0]),
                'clip_label': [it['clip_label'] for it in items]}
    return {'packed': pack_clips([it['frames'] for it in items], [it['mirror'] for it in items]),
            'B': len(items), 'T': int(items[0]['frames'].shape[0]), 'clip_label': [it['clip_label'] for it in items]}


def collate_items(items):
    """``collate_fn`` for a loader WITHOUT workers: the items stay as they are and ``DeviceClipBuilder.build`` packs them straight
    into its pinned staging buffer (one host copy less than ``collate_raw`` followed by the staging copy)."""
    return {'items': list(items), 'B': len(items), 'T': int(items[0]['frames'].shape[0]),
            'clip_label': [it['clip_label'] for it in items]}


def collate_for(num_workers):
    return collate_raw if num_workers > 0 else collate_items


def table_of(batch):
    """The descriptor table of a packed batch: an int64 [B T, 4] view of its header ([B T, 9] for an augmented batch)."""
    n = batch['B'] * batch['T']
    if 'n_tables' in batch:
        return batch['packed'][:n * AUG_DESC_INTS * 8].view(torch.int64).view(n, AUG_DESC_INTS)
    return batch['packed'][:n * DESC_INTS * 8].view(torch.int64).view(n, DESC_INTS)


class _Slot(object):
    def __init__(self):
        self.host = self.dev = self.event = None


class DeviceClipBuilder(object):
    """Packed raw batches -> model-ready clips on ``device`` (``tai_clip_from_frames``; ``tai_clip_from_frames_aug`` for a batch that
    carries augmentation records, and only for such a batch), on the current torch stream.

    Staging: two slots used in turn, each a pinned host buffer and a device buffer that grow to the largest batch seen.  ``build``
    copies (a packed batch from DataLoader workers) or packs (raw items from a loader without workers) the batch into the slot's
    pinned buffer, starts ONE ``non_blocking`` upload of it (header and frames together) and records
    an event behind the upload; a slot is refilled only after that event has completed, so a later batch never overwrites bytes an
    upload may still be reading, while the other slot lets the host pack batch i + 1 during the upload of batch i."""

    def __init__(self, c_dim, image_size, padding_size, device):
        if c_dim not in (1, 3):
            raise ValueError('DeviceClipBuilder: c_dim must be 1 or 3')
        self.c_dim = int(c_dim)
        self.image_size = (int(image_size[0]), int(image_size[1]))
        self.padding_size = (int(padding_size[0]), int(padding_size[1]))
        self.device = torch.device(device)
        self._levels = level_tables().to(self.device)
        self._slots, self._turn = (_Slot(), _Slot()), 0

    def _slot(self, n):
        """The next staging slot, free to be refilled and at least ``n`` bytes large."""
        slot = self._slots[self._turn]
        self._turn ^= 1
        if slot.event is not None:
            slot.event.synchronize()                 # the previous upload out of this slot has finished reading it
        if slot.host is None or slot.host.numel() < n:
            cap = max(n, 1 << 20)
            slot.host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
            slot.dev = torch.empty(cap, dtype=torch.uint8, device=self.device)
            slot.event = torch.cuda.Event()
        return slot

    def build(self, batch):
        """batch: what ``collate_raw`` (a packed batch) or ``collate_items`` (the raw items) made -> fp32
        [B, T, C, H + pad_h, W + pad_w] on the device; asynchronous (the caller's stream orders its consumers)."""
        B, T = int(batch['B']), int(batch['T'])
        n = B * T
        if 'n_tables' in batch or ('items' in batch and _augs_of(batch['items']) is not None):
            return self._build_augmented(batch, B, T)
        head = header_bytes(n)
        (H, W), (ph, pw) = self.image_size, self.padding_size
        with torch.cuda.device(self.device):
            if 'packed' in batch:
                packed = batch['packed']
                if packed.dtype != torch.uint8 or packed.dim() != 1 or packed.numel() <= head or not packed.is_contiguous():
                    raise ValueError('DeviceClipBuilder.build: not a packed batch')
                nbytes = packed.numel()
                slot = self._slot(nbytes)
                slot.host[:nbytes].copy_(packed)
            else:
                clips, _ = _as_clips([it['frames'] for it in batch['items']])
                nbytes = packed_bytes(clips)
                slot = self._slot(nbytes)
                pack_clips(clips, [it['mirror'] for it in batch['items']], out=slot.host)
            slot.dev[:nbytes].copy_(slot.host[:nbytes], non_blocking=True)
            slot.event.record(torch.cuda.current_stream(self.device))
            out = torch.empty(B, T, self.c_dim, H + ph, W + pw, dtype=torch.float32, device=self.device)
            # the descriptor table is validated on the host from the staging buffer's header before anything is launched
            _native.launch('tai_clip_from_frames', self.device, slot.dev.data_ptr() + head, nbytes - head, slot.dev, slot.host, self._levels,
                           out, n, self.c_dim, H, W, ph, pw)
        return out


    def _build_augmented(self, batch, B, T):
        """``build`` for a batch that carries augmentation records: the same staging and ONE upload (header, level tables and frames
        together), then ``tai_clip_from_frames_aug``."""
        n = B * T
        head = aug_header_bytes(n)
        (H, W), (ph, pw) = self.image_size, self.padding_size
        with torch.cuda.device(self.device):
            if 'packed' in batch:
                packed, n_tables = batch['packed'], int(batch['n_tables'])
                first = head + n_tables * TABLE_BYTES
                if packed.dtype != torch.uint8 or packed.dim() != 1 or n_tables < 1 or packed.numel() <= first or not packed.is_contiguous():
                    raise ValueError('DeviceClipBuilder.build: not an augmented packed batch')
                nbytes = packed.numel()
                slot = self._slot(nbytes)
                slot.host[:nbytes].copy_(packed)
            else:
                clips, _ = _as_clips([it['frames'] for it in batch['items']])
                augs = _augs_of(batch['items'])
                nbytes = aug_packed_bytes(clips, augs)
                slot = self._slot(nbytes)
                _, n_tables = pack_clips_aug(clips, [it['mirror'] for it in batch['items']], augs, out=slot.host)
                first = head + n_tables * TABLE_BYTES
            slot.dev[:nbytes].copy_(slot.host[:nbytes], non_blocking=True)
            slot.event.record(torch.cuda.current_stream(self.device))
            out = torch.empty(B, T, self.c_dim, H + ph, W + pw, dtype=torch.float32, device=self.device)
            # the descriptor table is validated on the host from the staging buffer's header before anything is launched
            _native.launch('tai_clip_from_frames_aug', self.device, slot.dev.data_ptr() + first, nbytes - first, slot.dev, slot.host,
                           slot.dev.data_ptr() + head, n_tables, self._levels, out, n, self.c_dim, H, W, ph, pw)
        return out


def frames_to_uint8_device(x, h=None, w=None, rgb=False, out=None):
    """The kernel of the way out (``tai_frames_to_uint8``) on the current stream: fp32 CUDA [..., C, Hs, Ws] -> uint8 CUDA
    [..., h, w, C] (top-left crop, ``util.frames_to_uint8``'s truncating map, channel order reversed when ``rgb``).  NaN -> 0.
    With ``out`` given nothing is allocated."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() >= 3):
        raise ValueError('frames_to_uint8_device: expected a CUDA tensor [..., C, Hs, Ws]')
    C, Hs, Ws = x.shape[-3:]
    h, w = Hs if h is None else int(h), Ws if w is None else int(w)
    x = x.detach().to(torch.float32).contiguous()
    N = x.numel() // max(C * Hs * Ws, 1)
    shape = tuple(x.shape[:-3]) + (h, w, C)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=x.device)
    if out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != x.device:
        raise ValueError('frames_to_uint8_device: out must be a contiguous uint8 %s tensor on %s' % (shape, x.device))
    _native.launch('tai_frames_to_uint8', x.device, x, out, N, C, Hs, Ws, h, w, int(bool(rgb)))
    return out


_pinned_out = None


def to_uint8_host(x, h=None, w=None, rgb=False):
    """fp32 CUDA [..., C, Hs, Ws] in [-1, 1] -> numpy uint8 [..., h, w, C]: the kernel, then a copy of ONE byte per value into
    pinned memory (the host form moves four bytes per value, then clips, scales and casts on one core)."""
    global _pinned_out
    dev = frames_to_uint8_device(x, h, w, rgb)
    n = dev.numel()
    if _pinned_out is None or _pinned_out.numel() < n:
        _pinned_out = torch.empty(max(n, 1 << 20), dtype=torch.uint8, pin_memory=True)
    _pinned_out[:n].copy_(dev.reshape(-1), non_blocking=True)
    torch.cuda.current_stream(dev.device).synchronize()
    return _pinned_out[:n].numpy().reshape(tuple(dev.shape)).copy()
