"""The host side of the device clip pipeline (--device_preprocess): raw-mode datasets make the same draws as the default mode, the
collate packs ragged batches as the kernel's descriptor table says, the flag parses, and the library declares and exports the two
entry points.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from video_frame_inpainting_amd import _native, clip_pipeline
from video_frame_inpainting_amd.data import (ContiguousVideoClipDataset, DisjointVideoClipDataset, resize_bilinear)
from video_frame_inpainting_amd.options import TestOptions as PredictOptions, TrainOptions
from video_frame_inpainting_amd.util import bgr2gray, fore_transform

SEQ = 6


def _videos(tmp_path):
    """Three .npy videos of two sizes and one that is too short for a SEQ-frame window; a list that mixes whole videos and spans."""
    rng = np.random.RandomState(5)
    specs = {'a': (14, 24, 32), 'b': (11, 30, 20), 'short': (4, 24, 32), 'c': (9, 24, 32)}
    for name, (t, h, w) in specs.items():
        np.save(str(tmp_path / (name + '.npy')), rng.randint(0, 256, (t, h, w, 3), dtype=np.uint8))
    lines = ['%s' % (tmp_path / 'a.npy'), '%s 2-10' % (tmp_path / 'b.npy'), '%s' % (tmp_path / 'short.npy'),
             '%s' % (tmp_path / 'c.npy'), '%s 3-14' % (tmp_path / 'a.npy')]
    path = tmp_path / 'list.txt'
    path.write_text('\n'.join(lines) + '\n')
    return str(path)


def host_clip(frames, mirror, c_dim, image_size, padding_size):
    """_ClipReader.clip's arithmetic on already selected, already ordered frames [T, h, w, 3] uint8 RGB."""
    out = []
    for raw in frames.numpy():
        img = resize_bilinear(raw, image_size[0], image_size[1])[:, :, ::-1]
        if mirror:
            img = img[:, ::-1, :]
        img = np.pad(img, ((0, padding_size[0]), (0, padding_size[1]), (0, 0)), mode='constant')
        out.append(torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).float().div(255))
    clip = fore_transform(torch.stack(out))
    return bgr2gray(clip) if c_dim == 1 else clip


class _quiet(object):
    def __enter__(self):
        import warnings
        self._c = warnings.catch_warnings()
        self._c.__enter__()
        warnings.simplefilter('ignore')

    def __exit__(self, *a):
        return self._c.__exit__(*a)


@pytest.mark.parametrize('c_dim', [1, 3])
def test_raw_mode_makes_the_same_draws_as_the_default_mode(tmp_path, c_dim):
    path = _videos(tmp_path)
    size, pad = [16, 20], [2, 1]
    args = (c_dim, path, SEQ, True, True, size, True, pad)
    default = ContiguousVideoClipDataset(*args, seed=11)
    raw = ContiguousVideoClipDataset(*args, seed=11, raw=True)
    mirrors = set()
    with _quiet():                                 # the too-short video warns on every visit
        for epoch in range(3):                     # the generators run on: later epochs draw other windows and coins
            for i in range(len(default)):
                a, b = default[i], raw[i]          # index 2 is too short: both take the resample path
                assert sorted(b) == ['clip_label', 'frames', 'mirror']
                assert a['clip_label'] == b['clip_label']
                assert b['frames'].dtype == torch.uint8 and b['frames'].shape[0] == SEQ and b['frames'].shape[3] == 3
                assert isinstance(b['mirror'], bool)
                mirrors.add(b['mirror'])
                assert torch.equal(host_clip(b['frames'], b['mirror'], c_dim, size, pad), a['targets'])
    assert mirrors == {False, True}
    assert default.rng.getstate() == raw.rng.getstate()


def test_raw_mode_without_resampling_raises_like_the_default_mode(tmp_path):
    path = _videos(tmp_path)
    raw = ContiguousVideoClipDataset(1, path, SEQ, False, False, [16, 16], False, [0, 0], raw=True)
    with pytest.raises(RuntimeError, match='too short'):
        raw[2]


def test_disjoint_raw_mode_reads_the_same_frames(tmp_path):
    _videos(tmp_path)
    path = tmp_path / 'disjoint.txt'
    path.write_text('%s 1-3 7-9\n%s 2-4 6-8\n' % (tmp_path / 'a.npy', tmp_path / 'b.npy'))
    default = DisjointVideoClipDataset(3, str(path), 3, 3, [16, 16], [0, 4])
    raw = DisjointVideoClipDataset(3, str(path), 3, 3, [16, 16], [0, 4], raw=True)
    for i in range(2):
        a, b = default[i], raw[i]
        assert a['clip_label'] == b['clip_label'] and b['mirror'] is False
        assert torch.equal(host_clip(b['frames'], False, 3, [16, 16], [0, 4]), a['targets'])


def test_collate_packs_a_ragged_batch():
    rng = np.random.RandomState(1)
    shapes = [(3, 5, 7), (3, 4, 4), (3, 9, 2)]
    items = [{'frames': torch.from_numpy(rng.randint(0, 256, s + (3,), dtype=np.uint8)), 'mirror': m, 'clip_label': 'v%d' % i}
             for i, (s, m) in enumerate(zip(shapes, (False, True, False)))]
    batch = clip_pipeline.collate_raw(items)
    assert batch['B'] == 3 and batch['T'] == 3 and batch['clip_label'] == ['v0', 'v1', 'v2']
    packed = batch['packed']
    head = clip_pipeline.header_bytes(9)
    assert head % clip_pipeline.HEADER_ALIGN == 0 and head >= 9 * 32
    assert packed.dtype == torch.uint8 and packed.dim() == 1 and not packed.is_pinned()
    assert packed.numel() == head + sum(t * h * w * 3 for t, h, w in shapes)
    table = clip_pipeline.table_of(batch)
    assert table.dtype == torch.int64 and tuple(table.shape) == (9, 4)
    offset = 0
    for i, (t, h, w) in enumerate(shapes):
        for k in range(t):
            off, hh, ww, flags = table[i * t + k].tolist()
            assert (off, hh, ww, flags) == (offset, h, w, 1 if items[i]['mirror'] else 0)
            frame = packed[head + off:head + off + h * w * 3].view(h, w, 3)
            assert torch.equal(frame, items[i]['frames'][k])
            offset += h * w * 3
    assert offset == packed.numel() - head
    # packed into a caller's buffer (the builder's staging): the same bytes, as a view of the buffer's head
    buf = torch.full((packed.numel() + 100,), 7, dtype=torch.uint8)
    view = clip_pipeline.pack_clips([it['frames'] for it in items], [it['mirror'] for it in items], out=buf)
    assert view.data_ptr() == buf.data_ptr() and torch.equal(view, packed) and (buf[packed.numel():] == 7).all()
    assert clip_pipeline.packed_bytes([it['frames'] for it in items]) == packed.numel()
    kept = clip_pipeline.collate_items(items)
    assert kept['B'] == 3 and kept['T'] == 3 and kept['clip_label'] == batch['clip_label'] and kept['items'][1] is items[1]
    assert clip_pipeline.collate_for(0) is clip_pipeline.collate_items and clip_pipeline.collate_for(2) is clip_pipeline.collate_raw
    with pytest.raises(ValueError):
        clip_pipeline.pack_clips([items[0]['frames']], [False], out=buf[:10])
    with pytest.raises(ValueError):
        clip_pipeline.collate_raw([items[0], {'frames': items[1]['frames'][:2], 'mirror': False, 'clip_label': 'x'}])


def test_level_tables_are_the_host_expressions():
    t = clip_pipeline.level_tables()
    assert t.dtype == torch.float32 and tuple(t.shape) == (4, 256)
    k = torch.arange(256).to(torch.uint8).view(256, 1, 1, 1).expand(256, 3, 1, 1).contiguous()
    clip = fore_transform(k.float().div(255))
    assert torch.equal(t[0], clip[:, 0, 0, 0])
    assert torch.equal((t[1] + t[2]) + t[3], bgr2gray(clip)[:, 0, 0, 0])
    assert t[0, 0].item() == -1.0 and abs(((t[1] + t[2]) + t[3])[0].item() + 0.99990004) < 1e-7


def test_options_parse_the_flag_default_off():
    base = ['--K', '2', '--T', '2', '--F', '2', '--model_key', 'TAI_gray']
    for cls, extra in ((TrainOptions, []), (PredictOptions, ['--qual_result_root', 'r'])):
        assert cls().parse(base + extra, require_gpu=False).device_preprocess is False
        assert cls().parse(base + extra + ['--device_preprocess'], require_gpu=False).device_preprocess is True


def test_header_declares_and_library_exports_the_entry_points():
    declared = _native.declared_symbols()
    assert 'tai_clip_from_frames' in declared and 'tai_frames_to_uint8' in declared
    assert os.path.exists(_native.LIB_PATH)
    _native.verify(_native.LIB_PATH)
    L = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(L, 'tai_clip_from_frames') and hasattr(L, 'tai_frames_to_uint8')
    L.tai_sepconv_version.restype = ctypes.c_int
    assert L.tai_sepconv_version() >= 600
