"""The opt-in training augmentation without a GPU (train.py --aug_*; data.ClipAugment; include/tai_sepconv.h at tai_clip_from_frames_aug):
the level tables, the host path against the numpy restatement (tests/clip_augment_ref.py) with tolerance zero, the draws and what they
leave untouched, the options, the resume refusal, the packed form, and what the new entry refuses through the C ABI with no device."""
import ctypes
import json
import os
import random
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))          # (for the child process of the refusal test)
import clip_augment_ref as ref  # noqa: E402

from video_frame_inpainting_amd import _native, clip_pipeline  # noqa: E402
from video_frame_inpainting_amd.data import (ClipAugment, ClipRecord, ContiguousVideoClipDataset, ResumableBatchSampler,  # noqa: E402
                                             _ArrayVideo, _ClipReader, crop_window)
from video_frame_inpainting_amd.options import TrainOptions  # noqa: E402

SEQ = 5
FULL = dict(crop=0.5, vflip=True, brightness=0.2, contrast=0.3, gamma=0.5, flicker=0.1)


# ---------------------------------------------------------------------------------------------------------------- level tables

def test_neutral_parameters_give_the_level_tables_bit_for_bit():
    neutral = clip_pipeline.augment_level_tables()
    assert neutral.dtype == torch.float32 and tuple(neutral.shape) == (1, 4, 256)
    for row in range(4):
        assert torch.equal(neutral[0, row], clip_pipeline.level_tables()[row]), row
    assert np.array_equal(ref.NEUTRAL, clip_pipeline.level_tables().numpy())
    record = ClipAugment(**FULL).draw(random.Random(1), SEQ)
    assert torch.equal(clip_pipeline.tables_of_record(dict(record, gamma=1.0, gain=1.0, offset=0.0, flicker=None))[0],
                       clip_pipeline.level_tables())


@pytest.mark.parametrize('gamma,gain,offsets', [(1.0, 1.0, [0.0]), (0.5, 1.3, [0.2, -0.2]), (2.0, 0.7, [-0.3]), (1.5, 1.99, [0.99, -0.99]),
                                                (1.0, 0.01, [0.5])])
def test_tables_are_monotone_inside_the_range_and_equal_the_restatement(gamma, gain, offsets):
    t = clip_pipeline.augment_level_tables(gamma, gain, offsets)
    assert tuple(t.shape) == (len(offsets), 4, 256)
    assert (t[:, 0, 1:] >= t[:, 0, :-1]).all()                       # a gain > 0 keeps the order of the levels
    assert t[:, 0].min() >= -1.0 and t[:, 0].max() <= 1.0
    for i, off in enumerate(offsets):
        assert np.array_equal(t[i].numpy(), ref.level_table(gamma, gain, off))


# ---------------------------------------------------------------------------------------------------------------- host path

SOURCES = [(37, 53), (64, 48), (240, 320)]


def _windows(h, w):
    return {'full': (0, 0, h, w), 'one': (h // 2, w // 3, 1, 1), 'tl': (0, 0, 2, 2), 'tr': (0, w - 2, 2, 2), 'bl': (h - 2, 0, 2, 2),
            'br': (h - 2, w - 2, 2, 2), 'edge': (h - 17, w - 21, 17, 21), 'inner': (5, 7, h // 2, w // 2)}


def _ring(frames, window, value):
    """The frames with the one-pixel ring just outside the window set to ``value`` (where the frame has such pixels)."""
    top, left, ch, cw = window
    h, w = frames.shape[1:3]
    out = frames.copy()
    y0, y1, x0, x1 = max(top - 1, 0), min(top + ch + 1, h), max(left - 1, 0), min(left + cw + 1, w)
    inside = out[:, top:top + ch, left:left + cw].copy()
    out[:, y0:y1, x0:x1] = value
    out[:, top:top + ch, left:left + cw] = inside
    return out


@pytest.mark.parametrize('c_dim', [1, 3])
@pytest.mark.parametrize('src', SOURCES, ids=['%dx%d' % s for s in SOURCES])
@pytest.mark.parametrize('size,pad', [((32, 32), (0, 0)), ((30, 33), (3, 5))], ids=['32x32', '30x33p'])
def test_host_path_equals_the_restatement(src, size, pad, c_dim):
    rng = np.random.RandomState(src[0] + size[1] + c_dim)
    T = 3
    frames = rng.randint(0, 201, (T,) + src + (3,)).astype(np.uint8)
    reader = _ClipReader(c_dim, list(size), list(pad))
    record = ClipAugment(**FULL).draw(random.Random(src[1]), T)
    for k, (name, window) in enumerate(sorted(_windows(*src).items())):
        mirror, reverse = bool(k & 1), bool(k & 2)
        aug = dict(record, window=window, vflip=bool(k & 4))
        if k % 3 == 0:
            aug.update(flicker=None)
        loud = _ring(frames, window, 255)
        got = reader.clip(_ArrayVideo(loud, 'loud'), range(T), mirror, reverse, aug)
        playback = loud[::-1] if reverse else loud
        want = ref.clip(playback, c_dim, size, pad, window, mirror, aug['vflip'], aug['gamma'], aug['gain'], aug['offset'], aug['flicker'])
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
        assert torch.equal(got, torch.from_numpy(want)), (name, window)
        # a pixel outside the window never contributes: 255-level outliers around it change nothing
        quiet = reader.clip(_ArrayVideo(_ring(frames, window, 0), 'quiet'), range(T), mirror, reverse, aug)
        assert torch.equal(got, quiet), (name, window)
        # and neutral photometry over the full frame is the reference's pipeline itself
        if name == 'full':
            plain = dict(aug, vflip=False, gamma=1.0, gain=1.0, offset=0.0, flicker=None)
            assert torch.equal(reader.clip(_ArrayVideo(frames, 'f'), range(T), mirror, reverse, plain),
                               reader.clip(_ArrayVideo(frames, 'f'), range(T), mirror, reverse))


def test_padding_is_the_neutral_level_whatever_the_tables():
    frames = np.full((2, 9, 9, 3), 128, dtype=np.uint8)
    neutral = clip_pipeline.level_tables()
    aug = dict(ClipAugment(brightness=0.9).draw(random.Random(0), 2), window=(0, 0, 9, 9), offset=0.9)
    for c_dim, value in ((3, -1.0), (1, ((neutral[1, 0] + neutral[2, 0]) + neutral[3, 0]).item())):
        got = _ClipReader(c_dim, [8, 8], [2, 4]).clip(_ArrayVideo(frames, 'x'), range(2), False, False, aug)
        assert (got[..., 8:, :] == value).all() and (got[..., :, 8:] == value).all() and (got[..., :8, :8] > 0.9).all()


def test_crop_window_is_the_written_formula():
    assert crop_window(240, 320, 1.0, 0.3, 0.9, 0.9) == (0, 0, 240, 320)
    assert crop_window(240, 320, 0.5, 0.0, 0.999999, 0.0) == (120, 0, 120, 160)
    assert crop_window(3, 3, 0.1, 0.0, 0.5, 0.99) == (1, 2, 1, 1)                  # ch = max(1, floor(0.3)) = 1
    r = random.Random(4)
    for _ in range(200):
        h, w, smin, us, ut, ul = r.randint(1, 300), r.randint(1, 300), r.uniform(0.01, 1.0), r.random(), r.random(), r.random()
        top, left, ch, cw = crop_window(h, w, smin, us, ut, ul)
        assert (top, left, ch, cw) == ref.crop_window(h, w, smin, us, ut, ul)
        assert 0 <= top and 0 <= left and ch >= 1 and cw >= 1 and top + ch <= h and left + cw <= w


# ---------------------------------------------------------------------------------------------------------------- draws

def _videos(tmp_path, bad=False):
    rng = np.random.RandomState(5)
    specs = {'a': (14, 24, 32), 'b': (11, 30, 20), 'c': (9, 24, 32), 'd': (12, 26, 18)}
    for name, (t, h, w) in specs.items():
        np.save(str(tmp_path / (name + '.npy')), rng.randint(0, 256, (t, h, w, 3), dtype=np.uint8))
    lines = ['%s' % (tmp_path / 'a.npy'), '%s 2-10' % (tmp_path / 'b.npy'), '%s' % (tmp_path / 'c.npy'), '%s' % (tmp_path / 'd.npy')]
    path = tmp_path / 'list.txt'
    path.write_text('\n'.join(lines) + '\n')
    return str(path)


def _dataset(path, c_dim=1, raw=False, augment=None, seed=11):
    return ContiguousVideoClipDataset(c_dim, path, SEQ, True, True, [16, 20], True, [2, 1], seed=seed, raw=raw, augment=augment)


def test_smin_one_and_no_other_flag_leaves_the_items_as_they_were(tmp_path):
    path = _videos(tmp_path)
    assert not ClipAugment().on and not ClipAugment(crop=1.0, brightness=0.0).on and ClipAugment(flicker=0.01).on and ClipAugment(vflip=True).on
    for raw in (False, True):
        plain, off = _dataset(path, raw=raw), _dataset(path, raw=raw, augment=ClipAugment(crop=1.0))
        assert off.augment is None
        for epoch in range(2):
            for i in range(len(plain)):
                a, b = plain[i], off[i]
                assert sorted(a) == sorted(b)
                assert torch.equal(a['frames' if raw else 'targets'], b['frames' if raw else 'targets'])
        assert plain.rng.getstate() == off.rng.getstate()


@pytest.mark.parametrize('raw', [False, True])
def test_window_mirror_and_reversal_are_those_of_the_run_without_flags(tmp_path, raw):
    path = _videos(tmp_path)
    plain, on = _dataset(path, raw=raw), _dataset(path, raw=raw, augment=ClipAugment(**FULL))
    differs = 0
    for epoch in range(2):
        for j in range(len(plain)):
            a, b = plain[(j, epoch, j)], on[(j, epoch, j)]
            assert torch.equal(a['window'], b['window']) and a['clip_label'] == b['clip_label']
            if raw:
                assert torch.equal(a['frames'], b['frames']) and a['mirror'] == b['mirror'] and 'aug' in b and 'aug' not in a
                h, w = b['frames'].shape[1:3]
                assert b['aug']['window'] == crop_window(h, w, 0.5, *b['aug']['u_crop']) and len(b['aug']['flicker']) == SEQ
            else:
                differs += int(not torch.equal(a['targets'], b['targets']))
    assert raw or differs == 2 * len(plain)
    # one flag alone draws the same record fields as all flags together: no flag shifts another's stream
    some = _dataset(path, raw=True, augment=ClipAugment(crop=0.5))
    full = _dataset(path, raw=True, augment=ClipAugment(**FULL))
    for j in range(len(some)):
        a, b = some[(j, 0, j)]['aug'], full[(j, 0, j)]['aug']
        assert a['u_crop'] == b['u_crop'] and a['window'] == b['window']
        assert (a['vflip'], a['gamma'], a['gain'], a['offset'], a['flicker']) == (False, 1.0, 1.0, 0.0, None)


def test_the_host_item_equals_the_raw_item_put_through_the_host_path(tmp_path):
    path = _videos(tmp_path)
    for c_dim in (1, 3):
        host = _dataset(path, c_dim, augment=ClipAugment(**FULL))
        raw = _dataset(path, c_dim, raw=True, augment=ClipAugment(**FULL))
        for j in range(len(host)):
            a, b = host[(j, 1, j)], raw[(j, 1, j)]
            again = _ClipReader(c_dim, [16, 20], [2, 1]).clip(_ArrayVideo(b['frames'].numpy(), 'x'), range(SEQ), b['mirror'], False, b['aug'])
            assert torch.equal(a['targets'], again)


def test_position_keyed_items_do_not_depend_on_the_worker_count(tmp_path):
    path = _videos(tmp_path)
    got = {}
    for workers in (0, 2):
        dataset = _dataset(path, augment=ClipAugment(**FULL))
        sampler = ResumableBatchSampler(len(dataset), 2, 3)
        loader = torch.utils.data.DataLoader(dataset, batch_sampler=sampler, num_workers=workers, worker_init_fn=dataset.worker_init,
                                             generator=torch.Generator().manual_seed(1))
        got[workers] = [(b['targets'], b['window']) for b in loader]
    assert len(got[0]) == 2
    for (a, wa), (b, wb) in zip(got[0], got[2]):
        assert torch.equal(a, b) and torch.equal(wa, wb)


class _Failing(object):
    """A video whose frame ``bad`` cannot be read."""
    def __init__(self, frames, bad):
        self._frames, self._bad, self._filename = frames, bad, 'failing'

    def get_length(self):
        return self._frames.shape[0]

    def get_data(self, index):
        if index == self._bad:
            raise ValueError('unreadable')
        return self._frames[index]


def test_a_failed_read_consumes_a_fixed_number_of_draws(tmp_path):
    path = _videos(tmp_path)
    frames = np.random.RandomState(0).randint(0, 256, (SEQ, 24, 32, 3), dtype=np.uint8)       # exactly SEQ frames: the window starts at 0
    states, items = [], []
    for bad in (0, SEQ - 1):
        dataset = _dataset(path, augment=ClipAugment(**FULL))
        real = dataset.open_video
        dataset.open_video = lambda p, real=real, bad=bad: _Failing(frames, bad) if p.endswith('a.npy') else real(p)
        before = dataset.rng.getstate()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            items.append(dataset[0])                                    # line 0 fails wherever the bad frame is, a replacement is drawn
        states.append(dataset.rng.getstate())
        # the failed attempt alone: start, mirror, reversal, then 7 + SEQ draws of the augmentation, whichever frame failed
        probe = random.Random()
        probe.setstate(before)
        probe.randint(0, 0), probe.random(), probe.random()
        [probe.random() for _ in range(ClipAugment.N_CLIP_DRAWS + SEQ)]
        fresh = _dataset(path, augment=ClipAugment(**FULL))
        fresh.rng.setstate(probe.getstate())
        fresh.open_video = dataset.open_video
        replacement = None
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            while replacement is None:                                  # (the replacement line may be the failing one again)
                replacement = fresh._try(ClipRecord(fresh.files[fresh.rng.randrange(len(fresh.files))]))[0]
        assert torch.equal(replacement['targets'], items[-1]['targets']) and fresh.rng.getstate() == states[-1]
    assert states[0] == states[1] and torch.equal(items[0]['targets'], items[1]['targets'])
    # position-keyed: the position after a failing one yields what it yields in a run where nothing fails
    healthy, failing = _dataset(path, augment=ClipAugment(**FULL)), _dataset(path, augment=ClipAugment(**FULL))
    real = failing.open_video
    failing.open_video = lambda p: _Failing(frames, 2) if p.endswith('a.npy') else real(p)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        failing[(0, 0, 0)]
    assert torch.equal(healthy[(1, 0, 1)]['targets'], failing[(1, 0, 1)]['targets'])


# ---------------------------------------------------------------------------------------------------------------- options, resume

BASE = ['--K', '2', '--T', '1', '--F', '2', '--model_key', 'TAI_gray']


def test_options_parse_with_every_flag_off_by_default():
    opt = TrainOptions().parse(BASE, require_gpu=False)
    assert (opt.aug_crop, opt.aug_vflip, opt.aug_brightness, opt.aug_contrast, opt.aug_gamma, opt.aug_flicker) == (1.0, False, 0.0, 0.0, 0.0, 0.0)
    assert not ClipAugment.from_options(opt).on
    opt = TrainOptions().parse(BASE + ['--aug_crop', '0.5', '--aug_vflip', '--aug_brightness', '0.1', '--aug_contrast', '0.2', '--aug_gamma',
                                       '0.3', '--aug_flicker', '0.05'], require_gpu=False)
    assert ClipAugment.from_options(opt).state() == {'crop': 0.5, 'vflip': True, 'brightness': 0.1, 'contrast': 0.2, 'gamma': 0.3,
                                                     'flicker': 0.05}


@pytest.mark.parametrize('flag,value', [('--aug_crop', '0'), ('--aug_crop', '1.01'), ('--aug_crop', '-0.5'), ('--aug_crop', 'nan'),
                                        ('--aug_brightness', '1'), ('--aug_brightness', '-0.1'), ('--aug_brightness', 'inf'),
                                        ('--aug_contrast', '1'), ('--aug_contrast', '-0.1'), ('--aug_contrast', 'nan'),
                                        ('--aug_gamma', '-0.1'), ('--aug_gamma', 'inf'), ('--aug_gamma', 'nan'),
                                        ('--aug_flicker', '1'), ('--aug_flicker', '-1e-3'), ('--aug_flicker', 'nan')])
def test_options_outside_their_range_are_refused_at_parse_time_with_the_flag_named(flag, value, capsys):
    with pytest.raises(SystemExit) as e:
        TrainOptions().parse(BASE + [flag, value], require_gpu=False)
    assert e.value.code not in (0, None) and flag in capsys.readouterr().err
    with pytest.raises(ValueError, match=flag):
        ClipAugment(**{flag[6:]: float(value)})


def test_a_continuation_with_other_settings_is_refused_with_both_values_named():
    on = ClipAugment(crop=0.5, flicker=0.1)
    on.check_continues(on.state())
    ClipAugment().check_continues(None)
    with pytest.raises(ValueError, match=r"augment = .*'crop': 0\.5.*this run has .*'crop': 0\.75.*cannot be continued exactly"):
        ClipAugment(crop=0.75, flicker=0.1).check_continues(on.state())
    with pytest.raises(ValueError, match=r"augment = None, this run has .*'flicker': 0\.1"):
        on.check_continues(None)
    with pytest.raises(ValueError, match=r"'crop': 0\.5.*this run has None"):
        ClipAugment().check_continues(on.state())
    # what the run records: the sampler's own state, with the settings beside it only when augmentation is on
    state = dict(ResumableBatchSampler(8, 2, 1).state(), augment=on.state())
    ResumableBatchSampler(8, 2, 1).load_state(state)


# ---------------------------------------------------------------------------------------------------------------- packed form

def _items(flicker=True):
    rng = np.random.RandomState(1)
    shapes = [(3, 5, 7), (3, 4, 4), (3, 9, 2)]
    aug = ClipAugment(**dict(FULL, flicker=0.1 if flicker else 0.0))
    items = []
    for i, (s, m) in enumerate(zip(shapes, (False, True, False))):
        record = aug.draw(random.Random(i), 3)
        items.append({'frames': torch.from_numpy(rng.randint(0, 256, s + (3,), dtype=np.uint8)), 'mirror': m, 'clip_label': 'v%d' % i,
                      'aug': dict(record, window=crop_window(s[1], s[2], 0.5, *record['u_crop']))})
    return items, shapes


@pytest.mark.parametrize('flicker', [False, True])
def test_collate_packs_descriptors_tables_and_frames(flicker):
    items, shapes = _items(flicker)
    batch = clip_pipeline.collate_raw(items)
    n_tables = 9 if flicker else 3
    assert batch['B'] == 3 and batch['T'] == 3 and batch['n_tables'] == n_tables
    packed, head = batch['packed'], clip_pipeline.aug_header_bytes(9)
    first = head + n_tables * clip_pipeline.TABLE_BYTES
    assert head % clip_pipeline.HEADER_ALIGN == 0 and head >= 9 * 9 * 8 and clip_pipeline.AUG_DESC_INTS == 9
    assert packed.dtype == torch.uint8 and packed.numel() == first + sum(t * h * w * 3 for t, h, w in shapes) and not packed.is_pinned()
    table = clip_pipeline.table_of(batch)
    assert tuple(table.shape) == (9, 9)
    tables = packed[head:first].view(torch.float32).view(n_tables, 4, 256)
    offset = 0
    for i, (t, h, w) in enumerate(shapes):
        want = clip_pipeline.tables_of_record(items[i]['aug'])
        for k in range(t):
            row = table[i * t + k].tolist()
            flags = (1 if items[i]['mirror'] else 0) | (2 if items[i]['aug']['vflip'] else 0)
            assert row[:4] == [offset, h, w, flags] and tuple(row[4:8]) == items[i]['aug']['window']
            assert row[8] == (i * t + k if flicker else i)
            assert torch.equal(tables[row[8]], want[k if flicker else 0])
            assert torch.equal(packed[first + offset:first + offset + h * w * 3].view(h, w, 3), items[i]['frames'][k])
            offset += h * w * 3
    buf = torch.full((packed.numel() + 64,), 7, dtype=torch.uint8)
    view, n = clip_pipeline.pack_clips_aug([it['frames'] for it in items], [it['mirror'] for it in items], [it['aug'] for it in items], out=buf)
    assert n == n_tables and view.data_ptr() == buf.data_ptr() and torch.equal(view, packed) and (buf[packed.numel():] == 7).all()
    assert clip_pipeline.aug_packed_bytes([it['frames'] for it in items], [it['aug'] for it in items]) == packed.numel()
    # without records the batch is today's, key for key
    plain = clip_pipeline.collate_raw([{k: v for k, v in it.items() if k != 'aug'} for it in items])
    assert sorted(plain) == ['B', 'T', 'clip_label', 'packed'] and tuple(clip_pipeline.table_of(plain).shape) == (9, 4)
    with pytest.raises(ValueError, match='mixes'):
        clip_pipeline.collate_raw([items[0], {k: v for k, v in items[1].items() if k != 'aug'}])
    with pytest.raises(ValueError, match='outside'):
        clip_pipeline.collate_raw([dict(items[0], aug=dict(items[0]['aug'], window=(0, 0, 6, 7)))])


# ---------------------------------------------------------------------------------------------------------------- C ABI refusals

P = 4096                         # a 16-byte aligned address that a refused call never follows
GOOD = [0, 4, 4, 0, 0, 0, 4, 4, 0]


def _call(frames=P, nbytes=100, table=P, host=GOOD, tables=P, n_tables=1, levels=P, out=P, N=1, c_dim=1, H=4, W=4, pad=(0, 0)):
    return (frames, nbytes, table, host, tables, n_tables, levels, out, N, c_dim, H, W) + tuple(pad)


def _row(**kw):
    names = ('off', 'h', 'w', 'flags', 'top', 'left', 'ch', 'cw', 'tab')
    return [kw.get(k, v) for k, v in zip(names, GOOD)]


REFUSALS = [
    (_call(frames=None), 'null pointer'), (_call(table=None), 'null pointer'), (_call(host=None), 'null pointer'),
    (_call(tables=None), 'null pointer'), (_call(levels=None), 'null pointer'), (_call(out=None), 'null pointer'),
    (_call(c_dim=2), 'c_dim must be 1 or 3'), (_call(c_dim=0), 'c_dim must be 1 or 3'), (_call(c_dim=4), 'c_dim must be 1 or 3'),
    (_call(N=0), '> 0'), (_call(H=0), '> 0'), (_call(W=-1), '> 0'), (_call(nbytes=0), '> 0'), (_call(n_tables=0), '> 0'),
    (_call(pad=(-1, 0)), '>= 0'),
    (_call(N=1 << 15, H=1 << 8, W=1 << 8), '2^31'), (_call(N=1, c_dim=3, H=1 << 15, W=1 << 15), '2^31'), (_call(H=1 << 24), '2^31'),
    (_call(nbytes=1 << 40), '2^31'),
    (_call(tables=P + 4), '16-byte aligned'),
    (_call(host=_row(h=0)), 'source size'), (_call(host=_row(w=1 << 24)), 'source size'),
    (_call(host=_row(off=60)), 'past the stated length'), (_call(host=_row(off=101, h=1, w=1, ch=1, cw=1)), 'past the stated length'),
    (_call(host=_row(off=-1)), 'past the stated length'), (_call(nbytes=47), 'past the stated length'),
    (_call(N=2, host=GOOD + _row(off=53)), 'past the stated length'),
    (_call(host=_row(ch=0)), 'ch or cw < 1'), (_call(host=_row(cw=0)), 'ch or cw < 1'), (_call(host=_row(ch=-3)), 'ch or cw < 1'),
    (_call(host=_row(top=1)), 'outside its frame'), (_call(host=_row(left=1)), 'outside its frame'), (_call(host=_row(ch=5)), 'outside its frame'),
    (_call(host=_row(top=-1, ch=2)), 'outside its frame'), (_call(host=_row(left=3, cw=2)), 'outside its frame'),
    (_call(host=_row(top=1 << 62, ch=1)), 'outside its frame'),
    (_call(host=_row(tab=1)), 'level-table index'), (_call(host=_row(tab=-1)), 'level-table index'),
    (_call(n_tables=3, host=_row(tab=3)), 'level-table index'), (_call(N=2, n_tables=2, host=_row(tab=1) + _row(off=48, tab=2)), 'level-table index'),
]
N_MESSAGES = 10
EINVAL = -1


def _answers(lib_path):
    """Run in a child process that sees no device: [(return code, message)] for REFUSALS, calls that end before any launch."""
    L = ctypes.CDLL(lib_path)
    for name, (restype, argtypes) in _native.signatures().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    out = []
    for args, _ in REFUSALS:
        host = None if args[3] is None else (ctypes.c_longlong * len(args[3]))(*args[3])
        rc = L.tai_clip_from_frames_aug(args[0], args[1], args[2], None if host is None else ctypes.cast(host, ctypes.c_void_p), *args[4:], None)
        out.append([rc, L.tai_sepconv_last_error().decode()])
    return out


def test_every_refusal_returns_the_error_and_its_message_without_a_device():
    import re
    assert 'tai_clip_from_frames_aug' in _native.declared_symbols()
    _native.verify(_native.LIB_PATH)
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1')
    child = subprocess.run([sys.executable, os.path.abspath(__file__), '--answers', _native.LIB_PATH], env=env, capture_output=True, text=True,
                           timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    got = json.loads(child.stdout)
    assert len(got) == len(REFUSALS)
    for (args, word), (rc, message) in zip(REFUSALS, got):
        assert rc == EINVAL and message.startswith('clip_from_frames_aug: ') and word in message, (args, rc, message)
    # every message the launcher can give is reached, and the launcher itself holds none (they are returned by the check)
    said = {m for _, m in got}
    source = open(os.path.join(_native.CSRC, 'clip_augment.hip.inc')).read()
    assert len(said) == N_MESSAGES and set(re.findall(r'return "(clip_from_frames_aug: [^"]*)";', source)) == said
    assert '"clip_from_frames_aug: ' not in open(os.path.join(_native.CSRC, 'capi_image.inc')).read()
    assert _native.lib().tai_sepconv_version() >= 860


if __name__ == '__main__':
    assert sys.argv[1:2] == ['--answers'] and len(sys.argv) == 3
    assert os.environ.get('HIP_VISIBLE_DEVICES') == '-1'
    print(json.dumps(_answers(sys.argv[2])))
