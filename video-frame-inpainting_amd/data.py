"""Clip I/O on the input side of the path: the reference's video-list datasets (src/data/base_dataset.py).

Same constructors, list-file formats, clip labels and per-frame pipeline -- resize to ``image_size`` (cv2.resize's
default bilinear), RGB -> BGR, optional horizontal flip, zero-pad bottom / right by ``padding_size``, scale to [0, 1]
(torchvision ``to_tensor``), map to [-1, 1] (``fore_transform``), gray if ``c_dim == 1`` (``bgr2gray``); optional
temporal reversal -- and the same ``{'targets': [T, C, H, W], 'clip_label': str}`` items.

What differs is where frames come from.  The reference opens every path with ``imageio.get_reader(path, 'ffmpeg')``
(:106-122); neither imageio nor cv2 exists in this image, so a "video" here is, in this order: a directory of image
files (sorted by name; PNG / JPEG / BMP through PIL), a ``.npy`` file or an ``.npz`` member ``frames`` holding
``[T, H, W, 3]`` uint8 RGB, then an imageio reader if imageio can be imported at run time, else video_io.py's own readers:
AVI files with intra-frame codecs (uncompressed, Motion-JPEG, PNG) and PIL frame sequences (GIF, TIFF, APNG, WebP).
Inter-frame codecs (DivX, H.264) are refused with the FourCC in the message.  The resize is a
numpy restatement of OpenCV's INTER_LINEAR (half-pixel centres, edge clamp, no antialiasing) rounded to nearest; OpenCV
computes it in 11-bit fixed point for uint8, so single pixels may differ from it by one grey level.
"""
import os
import random
import re
from warnings import warn

import struct

import numpy as np
import torch
import torch.utils.data as data

from .util import bgr2gray, fore_transform

_IMAGE_EXT = ('.png', '.jpg', '.jpeg', '.bmp')


class _ArrayVideo:
    def __init__(self, frames, name):
        if frames.ndim != 4 or frames.shape[3] != 3 or frames.dtype != np.uint8:
            raise IOError('%s: expected [T, H, W, 3] uint8 frames, found %s %s' % (name, frames.shape, frames.dtype))
        self._frames, self._filename = frames, name

    def get_length(self):
        return self._frames.shape[0]

    def get_data(self, index):
        if not 0 <= index < self._frames.shape[0]:
            raise IndexError('frame %d of %d in %s' % (index, self._frames.shape[0], self._filename))
        return self._frames[index]


class _ImageDirVideo:
    def __init__(self, path):
        self._filename = path
        self._files = sorted(f for f in os.listdir(path) if f.lower().endswith(_IMAGE_EXT))
        if not self._files:
            raise IOError('%s: no image files' % path)

    def get_length(self):
        return len(self._files)

    def get_data(self, index):
        from PIL import Image
        if not 0 <= index < len(self._files):
            raise IndexError('frame %d of %d in %s' % (index, len(self._files), self._filename))
        with Image.open(os.path.join(self._filename, self._files[index])) as img:
            return np.asarray(img.convert('RGB'))


def open_frame_source(path):
    """A reader with ``get_length()`` / ``get_data(i) -> [H, W, 3] uint8 RGB`` (the part of imageio's reader interface
    the reference uses, base_dataset.py:125-137), or None if the path cannot be opened."""
    try:
        if os.path.isdir(path):
            return _ImageDirVideo(path)
        if path.endswith('.npy'):
            return _ArrayVideo(np.load(path, mmap_mode='r'), path)
        if path.endswith('.npz'):
            return _ArrayVideo(np.load(path)['frames'], path)
        try:
            import imageio                                          # absent in this image; used when present
        except ImportError:
            from .video_io import open_video_file                   # AVI (uncompressed / Motion-JPEG / PNG), GIF, TIFF, ...
            return open_video_file(path)
        return imageio.get_reader(path, 'ffmpeg')
    except (IOError, OSError, ImportError, KeyError, ValueError, struct.error) as e:
        warn('Failed to open video %s: %s' % (path, e))
        return None


def resize_bilinear(frame, height, width):
    """cv2.resize(frame, (width, height)) with the default INTER_LINEAR, for [H, W, C] uint8."""
    h, w = frame.shape[:2]
    if (h, w) == (height, width):
        return frame
    def taps(n_out, n_in):
        src = (np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / float(n_out)) - 0.5
        i0 = np.floor(src).astype(np.int64)
        frac = src - i0
        return np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), frac
    y0, y1, fy = taps(height, h)
    x0, x1, fx = taps(width, w)
    f = frame.astype(np.float64)
    top = f[y0][:, x0] * (1 - fx)[None, :, None] + f[y0][:, x1] * fx[None, :, None]
    bot = f[y1][:, x0] * (1 - fx)[None, :, None] + f[y1][:, x1] * fx[None, :, None]
    out = top * (1 - fy)[:, None, None] + bot * fy[:, None, None]
    return np.clip(np.floor(out + 0.5), 0, 255).astype(np.uint8)


class ClipAugment(object):
    """The opt-in training augmentation (train.py --aug_crop / --aug_vflip / --aug_brightness / --aug_contrast / --aug_gamma /
    --aug_flicker; the definition is include/tai_sepconv.h's, at tai_clip_from_frames_aug).  ``on`` when any setting differs from its
    default; a dataset then draws N_CLIP_DRAWS + seq_len unit uniforms per clip in one fixed order -- all of them whichever flags are
    set, so switching one flag never shifts another's stream."""

    N_CLIP_DRAWS = 7                  # u_scale, u_top, u_left, u_vflip, u_gamma, u_gain, u_offset; then one per frame
    _FIELDS = ('crop', 'vflip', 'brightness', 'contrast', 'gamma', 'flicker')

    def __init__(self, crop=1.0, vflip=False, brightness=0.0, contrast=0.0, gamma=0.0, flicker=0.0):
        self.crop, self.vflip = float(crop), bool(vflip)
        self.brightness, self.contrast, self.gamma, self.flicker = float(brightness), float(contrast), float(gamma), float(flicker)
        for flag, ok, want in (('aug_crop', 0.0 < self.crop <= 1.0, 'in (0, 1]'),
                               ('aug_brightness', 0.0 <= self.brightness < 1.0, 'in [0, 1)'),
                               ('aug_contrast', 0.0 <= self.contrast < 1.0, 'in [0, 1)'),
                               ('aug_gamma', 0.0 <= self.gamma < float('inf'), 'finite and >= 0'),
                               ('aug_flicker', 0.0 <= self.flicker < 1.0, 'in [0, 1)')):
            if not ok:                # (a NaN fails every comparison)
                raise ValueError('--%s must be %s, found %r' % (flag, want, getattr(self, flag[4:])))

    @classmethod
    def from_options(cls, opt):
        return cls(opt.aug_crop, opt.aug_vflip, opt.aug_brightness, opt.aug_contrast, opt.aug_gamma, opt.aug_flicker)

    @property
    def on(self):
        return self.state() != ClipAugment().state()

    def state(self):
        """The settings as plain values: what a resumable run records (only when ``on``) and compares on a continuation."""
        return {k: getattr(self, k) for k in self._FIELDS}

    def check_continues(self, saved):
        """Refuse to continue a run whose saved data state carries other augmentation settings (``saved``: its 'augment' entry, None
        when it ran without augmentation), in the words of ``ResumableBatchSampler.load_state``."""
        mine = self.state() if self.on else None
        if saved != mine:
            raise ValueError('the saved clip order has augment = %r, this run has %r: it cannot be continued exactly' % (saved, mine))

    def draw(self, rng, seq_len):
        """One clip's record from N_CLIP_DRAWS + seq_len draws of ``rng``; the crop window waits for the frame size (``window``)."""
        u = [rng.random() for _ in range(self.N_CLIP_DRAWS + seq_len)]
        return {'u_crop': (u[0], u[1], u[2]), 'smin': self.crop,
                'vflip': bool(self.vflip and u[3] > 0.5),
                'gamma': (1.0 + self.gamma) ** (2.0 * u[4] - 1.0),
                'gain': 1.0 + self.contrast * (2.0 * u[5] - 1.0),
                'offset': self.brightness * (2.0 * u[6] - 1.0),
                'flicker': tuple(self.flicker * (2.0 * v - 1.0) for v in u[self.N_CLIP_DRAWS:]) if self.flicker > 0.0 else None}


def crop_window(h, w, smin, u_scale, u_top, u_left):
    """(top, left, ch, cw) of the crop window in an h x w frame, in float64 (Python floats)."""
    s = smin + u_scale * (1.0 - smin)
    ch, cw = max(1, int(np.floor(s * h))), max(1, int(np.floor(s * w)))
    top = min(int(np.floor(u_top * (h - ch + 1))), h - ch)
    left = min(int(np.floor(u_left * (w - cw + 1))), w - cw)
    return top, left, ch, cw


def with_window(aug, h, w):
    """The record with its crop window placed in an h x w frame."""
    return dict(aug, window=crop_window(h, w, aug['smin'], *aug['u_crop']))


class ClipRecord(object):
    """One parsed line of a video list.  Formats (reference base_dataset.py:147-156, :214-222), frame numbers 1-indexed and
    inclusive in the file, 0-indexed here:
        <path>                      the whole video                      spans = None
        <path> a-b                  one span                             spans = [(a-1, b-1)]
        <path> a-b c-d              preceding and following span         spans = [(a-1, b-1), (c-1, d-1)]"""

    _SPAN = re.compile(r'^(\d+)-(\d+)$')

    def __init__(self, line):
        fields = line.split()
        if not fields:
            raise RuntimeError('Empty line in video list')
        self.line = line
        self.path = fields[0]
        self.spans = None
        if len(fields) > 1:
            matches = [self._SPAN.match(f) for f in fields[1:]]
            if not all(matches):
                raise RuntimeError('Cannot parse frame ranges of video-list line "%s"' % line)
            self.spans = [(int(m.group(1)) - 1, int(m.group(2)) - 1) for m in matches]

    def label(self, spans):
        """``<basename>_a-b[_c-d]`` with 1-indexed inclusive numbers: the directory name predict.py writes into."""
        return '_'.join([os.path.basename(self.path)] + ['%d-%d' % (a + 1, b + 1) for a, b in spans])


class _ClipReader(object):
    """Frames of one clip -> the tensor the models take (base_dataset.py:50-103): resize, RGB -> BGR, optional horizontal
    flip, constant padding on the bottom / right, [-1, 1], gray if c_dim == 1, optional time reversal."""

    def __init__(self, c_dim, image_size, padding_size):
        self.c_dim, self.image_size, self.padding_size = c_dim, image_size, padding_size

    @staticmethod
    def frame(source, index):
        try:
            return np.asarray(source.get_data(index))
        except IndexError:
            raise
        except Exception as e:                                      # a decoder's read error (:129-137)
            warn('Failed to read frame %d in %s: %s' % (index, getattr(source, '_filename', '?'), e))
            return None

    def clip(self, source, indexes, mirror, reverse, aug=None):
        """``aug``: the clip's augmentation record (ClipAugment.draw) or None = the reference's pipeline, untouched."""
        if aug is not None:
            return self._augmented_clip(source, indexes, mirror, reverse, aug)
        frames = []
        for t in indexes:
            raw = self.frame(source, t)
            if raw is None:
                return None
            img = resize_bilinear(raw, self.image_size[0], self.image_size[1])[:, :, ::-1]      # RGB -> BGR (:81)
            if mirror:
                img = img[:, ::-1, :]
            # cv2.copyMakeBorder(..., BORDER_CONSTANT, -1) on uint8 saturates the -1 to 0, i.e. -1.0 after the [-1, 1] map
            img = np.pad(img, ((0, self.padding_size[0]), (0, self.padding_size[1]), (0, 0)), mode='constant')
            frames.append(torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).float().div(255))
        if reverse:
            frames.reverse()
        clip = fore_transform(torch.stack(frames))                  # T x C x H x W in [-1, 1]
        return bgr2gray(clip) if self.c_dim == 1 else clip

    def _augmented_clip(self, source, indexes, mirror, reverse, aug):
        """The host path of the augmented pipeline (include/tai_sepconv.h, tai_clip_from_frames_aug): crop, resize, BGR, flips, the
        frame's level table on the image area, then the neutral padding.  Bit-equal to the device path and to tests/clip_augment_ref.py."""
        from .clip_pipeline import level_tables, tables_of_record
        levels = []
        for t in indexes:
            raw = self.frame(source, t)
            if raw is None:
                return None
            if not levels:            # one window for the clip: the record's own if it was placed already (``with_window``)
                top, left, ch, cw = aug.get('window') or crop_window(raw.shape[0], raw.shape[1], aug['smin'], *aug['u_crop'])
            img = resize_bilinear(raw[top:top + ch, left:left + cw], self.image_size[0], self.image_size[1])[:, :, ::-1]
            if aug['vflip']:
                img = img[::-1]
            if mirror:
                img = img[:, ::-1]
            levels.append(torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).long())         # [3, H, W] levels, BGR
        if reverse:
            levels.reverse()
        tables, neutral = tables_of_record(aug), level_tables()
        H, W = self.image_size
        C = 3 if self.c_dim != 1 else 1
        pad = neutral[0, 0] if C == 3 else (neutral[1, 0] + neutral[2, 0]) + neutral[3, 0]
        clip = pad.repeat(len(levels), C, H + self.padding_size[0], W + self.padding_size[1])
        for i, q in enumerate(levels):                               # the frame at playback position i reads table i (flicker) or 0
            tab = tables[i if tables.shape[0] > 1 else 0]
            clip[i, :, :H, :W] = tab[0][q] if C == 3 else ((tab[1][q[0]] + tab[2][q[1]]) + tab[3][q[2]])[None]
        return clip

    def raw_clip(self, source, indexes, reverse):
        """The decoded frames of one clip as they are, uint8 RGB [T, h, w, 3] in playback order (``reverse`` applied): what the
        device clip pipeline (clip_pipeline.DeviceClipBuilder) takes in place of ``clip``'s tensor.  None on a read error, like
        ``clip``; frames of one clip must share one size."""
        frames = []
        for t in indexes:
            raw = self.frame(source, t)
            if raw is None:
                return None
            if raw.ndim != 3 or raw.shape[2] != 3 or raw.dtype != np.uint8 or (frames and raw.shape != frames[0].shape):
                warn('Frame %d in %s is not [h, w, 3] uint8 of the clip\'s size: %s %s'
                     % (t, getattr(source, '_filename', '?'), raw.shape, raw.dtype))
                return None
            frames.append(raw)
        if reverse:
            frames.reverse()
        return torch.from_numpy(np.stack(frames))


def position_key(tag, seed, rank, epoch, j):
    """One integer per (seed, rank, epoch, position): the seed of that position's private generator (tag 1) and of an epoch's
    permutation (tag 2).  The fields do not overlap, so two positions never share a stream."""
    return (int(tag) << 128) | ((int(seed) & 0xffffffff) << 96) | ((int(rank) & 0xffffffff) << 64) | ((int(epoch) & 0xffffffff) << 32) \
        | (int(j) & 0xffffffff)


class ResumableBatchSampler(data.Sampler):
    """A batch sampler whose order can be entered at any position (``train.py --resumable``).

    Epoch e visits the items in a permutation derived from (seed, rank, e) alone (the identity with ``serial``), in batches of
    ``batch_size`` (a ragged last batch is dropped, as train.py's loader does).  An item of a batch is ``(index, e, j)`` -- the line of the
    video list, the epoch and the position j inside the epoch -- and a dataset given such an item draws window, mirror, reversal and any
    replacement line from a generator seeded by (seed, rank, e, j): what a position yields depends on nothing that was read before it,
    on no worker count and on no worker.

    The position is (epoch, batches consumed) and moves only in ``took_batch``, which the consumer calls per batch it takes: what the
    loader's workers have prefetched beyond that is produced again after a resume.  Iterating yields the rest of the current epoch from
    the position at that moment, without touching the items it skips."""

    def __init__(self, n_items, batch_size, seed, rank=0, serial=False):
        self.n_items, self.batch_size, self.seed, self.rank, self.serial = int(n_items), int(batch_size), int(seed), int(rank), bool(serial)
        self.batches_per_epoch = self.n_items // self.batch_size
        if self.batches_per_epoch < 1:
            raise ValueError('ResumableBatchSampler: %d items do not fill one batch of %d' % (self.n_items, self.batch_size))
        self.epoch, self.consumed = 0, 0

    def permutation(self, epoch):
        order = list(range(self.n_items))
        if not self.serial:
            random.Random(position_key(2, self.seed, self.rank, epoch, 0)).shuffle(order)
        return order

    def __iter__(self):
        epoch, first = self.epoch, self.consumed
        order = self.permutation(epoch)
        for b in range(first, self.batches_per_epoch):
            yield [(order[j], epoch, j) for j in range(b * self.batch_size, (b + 1) * self.batch_size)]

    def __len__(self):
        return self.batches_per_epoch - self.consumed

    def took_batch(self):
        self.consumed += 1
        if self.consumed >= self.batches_per_epoch:
            self.epoch, self.consumed = self.epoch + 1, 0

    def state(self):
        return {'kind': 'sampler', 'seed': self.seed, 'rank': self.rank, 'serial': int(self.serial), 'n_items': self.n_items,
                'batch_size': self.batch_size, 'epoch': self.epoch, 'consumed': self.consumed}

    def load_state(self, state):
        mine = self.state()
        for k in ('kind', 'seed', 'rank', 'serial', 'n_items', 'batch_size'):
            if state.get(k) != mine[k]:
                raise ValueError('the saved clip order has %s = %r, this run has %r: it cannot be continued exactly'
                                 % (k, state.get(k), mine[k]))
        self.epoch, self.consumed = int(state['epoch']), int(state['consumed'])


class ContiguousVideoClipDataset(data.Dataset):
    """base_dataset.py:17-202: one line per video, ``<path>`` or ``<path> <a>-<b>``; an item is a random window of
    ``seq_length`` consecutive frames of that range, optionally mirrored / reversed; a video that cannot be opened, is too
    short or fails to decode is replaced by another random line when ``resample_on_fail`` (else RuntimeError).

    Every random draw (window start, augmentation coin flips, replacement line) comes from a PRIVATE generator seeded per
    dataset (``seed``; reseeded per DataLoader worker by ``worker_init``): the reference draws from the global ``random``
    and ``numpy.random`` modules, which in a data-parallel run is also where (K, T, F) used to come from -- one rank's
    decode retry would desynchronise every rank's model shapes.

    ``augment`` (a ``ClipAugment`` that is on; train.py --aug_*): after those three draws a clip draws its augmentation record -- a fixed
    number of uniforms, before any frame is read -- and the clip is cropped, flipped and photometrically changed by it; a raw item carries
    the record as ``'aug'`` for the device path, which gives the same bits.  Window start, mirror and reversal stay those of the same
    run without it.

    ``raw=True`` (the device clip pipeline, clip_pipeline.py): an item is ``{'frames': uint8 [T, h, w, 3] RGB as decoded, in
    playback order, 'mirror': bool, 'clip_label': str}`` -- the same draws in the same order pick the same window, mirror and
    reversal; the resize, flip, padding, range map and gray conversion are left to the GPU.

    Indexed with an item of ``ResumableBatchSampler``, ``(index, epoch, j)``, every draw for that item comes from a generator of its own,
    seeded by (``seed``, ``rank``, epoch, j) -- the dataset's generator is left alone -- and the item carries ``'window'``, an int64
    [start frame, mirror, reverse], for whoever wants to compare orders."""

    def __init__(self, c_dim, video_list_path, seq_length, backwards, flip, image_size, resample_on_fail, padding_size,
                 seed=0, raw=False, rank=0, augment=None):
        super().__init__()
        with open(video_list_path, 'r') as f:
            self.files = [line.strip() for line in f.readlines()]
        self.seq_len = seq_length
        self.backwards, self.flip, self.resample_on_fail = backwards, flip, resample_on_fail
        self.reader = _ClipReader(c_dim, image_size, padding_size)
        self._seed = int(seed)
        self._rank = int(rank)
        self.raw = bool(raw)
        self.augment = augment if augment is not None and augment.on else None      # a ClipAugment that is on, else nothing is drawn
        self.rng = random.Random(self._seed)

    def worker_init(self, worker_id):
        """DataLoader ``worker_init_fn``.  Inside a worker ``torch.initial_seed()`` is the loader's base seed + worker id,
        and the base seed is drawn afresh from the loader's generator every time the loader is iterated -- so, as in the
        reference (whose workers reseed the global ``random`` from that same base seed), every epoch and every worker
        gets its own stream, reproducible from the loader's generator and this dataset's seed."""
        self.rng = random.Random(int(torch.initial_seed()) ^ (self._seed << 20))

    def __len__(self):
        return len(self.files)

    def open_video(self, vid_path):
        return open_frame_source(vid_path)

    def _try(self, record, rng=None):
        """-> (item, None) or (None, reason); the draws come from ``rng`` (default: the dataset's generator)."""
        positional, rng = rng is not None, rng or self.rng
        source = self.open_video(record.path)
        if source is None:
            return None, 'Video at %s could not be opened' % record.path
        first, last = record.spans[0] if record.spans else (0, source.get_length() - 1)
        if last - first + 1 < self.seq_len:
            return None, 'Interval %s in video %s is too short' % (str((first, last)), record.path)
        start = rng.randint(first, last - self.seq_len + 1)
        mirror = self.flip and rng.random() > 0.5
        reverse = self.backwards and rng.random() > 0.5
        # the augmentation's draws: after the three above, from the same generator, all of them, before any frame is read
        aug = self.augment.draw(rng, self.seq_len) if self.augment is not None else None
        if self.raw:
            frames = self.reader.raw_clip(source, range(start, start + self.seq_len), reverse)
            if frames is None:
                return None, 'Failed to sample frames starting at %d in %s' % (start, record.path)
            item = {'frames': frames, 'mirror': bool(mirror), 'clip_label': record.label([(first, last)])}
            if aug is not None:
                item['aug'] = with_window(aug, frames.shape[1], frames.shape[2])
        else:
            clip = self.reader.clip(source, range(start, start + self.seq_len), mirror, reverse, **({} if aug is None else {'aug': aug}))
            if clip is None:
                return None, 'Failed to sample frames starting at %d in %s' % (start, record.path)
            item = {'targets': clip, 'clip_label': record.label([(first, last)])}
        if positional:
            item['window'] = torch.tensor([start, int(bool(mirror)), int(bool(reverse))], dtype=torch.int64)
        return item, None

    def __getitem__(self, index):
        rng = None
        if isinstance(index, (tuple, list)):                       # an item of ResumableBatchSampler: a generator of its own
            index, epoch, j = index
            rng = random.Random(position_key(1, self._seed, self._rank, epoch, j))
        item, reason = self._try(ClipRecord(self.files[index]), rng)
        while item is None:
            if not self.resample_on_fail:
                raise RuntimeError(reason)
            item, reason = self._try(ClipRecord(self.files[(rng or self.rng).randrange(len(self.files))]), rng)
        return item


class DisjointVideoClipDataset(ContiguousVideoClipDataset):
    """base_dataset.py:205-248: ``<path> <a>-<b> <c>-<d>``: the preceding frames a..b and the following frames c..d,
    nothing in between; no augmentation, no resampling."""

    def __init__(self, c_dim, video_list_path, K, F, image_size, padding_size, raw=False):
        super().__init__(c_dim, video_list_path, None, False, False, image_size, False, padding_size, raw=raw)
        self.K, self.F = K, F

    def __getitem__(self, index):
        try:
            record = ClipRecord(self.files[index])
        except RuntimeError:
            record = None
        if record is None or record.spans is None or len(record.spans) != 2:
            raise RuntimeError('Expected line from video list to have format "<video_path> <A-B> <C-D>", '
                               'but found line "%s")' % self.files[index])
        source = self.open_video(record.path)
        if source is None:
            raise RuntimeError('Video at %s could not be opened' % record.path)
        indexes = [t for a, b in record.spans for t in range(a, b + 1)]
        if self.raw:
            frames = self.reader.raw_clip(source, indexes, False)
            if frames is None:
                raise RuntimeError('Failed to sample frames %s in %s' % (record.label(record.spans), record.path))
            return {'frames': frames, 'mirror': False, 'clip_label': record.label(record.spans)}
        clip = self.reader.clip(source, indexes, False, False)
        if clip is None:
            raise RuntimeError('Failed to sample frames %s in %s' % (record.label(record.spans), record.path))
        return {'targets': clip, 'clip_label': record.label(record.spans)}
