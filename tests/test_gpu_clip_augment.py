"""The augmented way into the clip pipeline on the GPU (tai_clip_from_frames_aug, csrc/clip_augment.hip.inc) against the host path of this
repository (data._ClipReader.clip with an augmentation record), and train.py --aug_* end to end.  Tolerance: zero (torch.equal) throughout."""
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from video_frame_inpainting_amd import _native, clip_pipeline  # noqa: E402
from video_frame_inpainting_amd.data import ClipAugment, _ArrayVideo, _ClipReader, crop_window  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FULL = dict(crop=0.5, vflip=True, brightness=0.2, contrast=0.3, gamma=0.5, flicker=0.1)
SENTINEL = 12345.0


def _frames(rng, t, h, w):
    return rng.randint(0, 256, (t, h, w, 3), dtype=np.uint8)


def _record(seed, T, window, vflip, flicker=True):
    r = ClipAugment(**FULL).draw(random.Random(seed), T)
    return dict(r, window=tuple(window), vflip=bool(vflip), flicker=r['flicker'] if flicker else None)


def host_clip(frames, c_dim, size, pad, mirror, reverse, aug):
    return _ClipReader(c_dim, list(size), list(pad)).clip(_ArrayVideo(frames, 'test'), range(frames.shape[0]), mirror, reverse, aug)


def raw_item(frames, mirror, reverse, aug=None):
    f = _ClipReader(1, None, None).raw_clip(_ArrayVideo(frames, 'test'), range(frames.shape[0]), reverse)
    item = {'frames': f, 'mirror': mirror, 'clip_label': 'test'}
    if aug is not None:
        item['aug'] = aug
    return item


def _windows(h, w):
    return {'full': (0, 0, h, w), 'one': (h // 2, w // 3, 1, 1), 'tl': (0, 0, 2, 2), 'tr': (0, w - 2, 2, 2), 'bl': (h - 2, 0, 2, 2),
            'br': (h - 2, w - 2, 2, 2), 'edge': (h - 17, w - 21, 17, 21), 'inner': (5, 7, h // 2, w // 2)}


# (source h, w) -> (output H, W), padding: the CPU test's shapes (38 columns: ten lanes on a row, 25 rows in flight, six lanes idle), then
# one whose rows hold more than 256 four-column runs (a lane's column loop runs twice) in bands of four rows
CASES = [((37, 53), (32, 32), (0, 0)), ((37, 53), (30, 33), (3, 5)), ((64, 48), (32, 32), (0, 0)), ((64, 48), (30, 33), (3, 5)),
         ((240, 320), (32, 32), (0, 0)), ((240, 320), (30, 33), (3, 5)), ((40, 37), (3, 1100), (2, 0))]


@pytest.mark.parametrize('c_dim', [1, 3])
@pytest.mark.parametrize('src,size,pad', CASES, ids=['%dx%d-%dx%d' % (c[0] + c[1]) for c in CASES])
def test_device_equals_the_host_path(src, size, pad, c_dim):
    rng = np.random.RandomState(src[0] * 7 + size[1] + c_dim)
    T = 3
    frames = _frames(rng, T, *src)
    builder = clip_pipeline.DeviceClipBuilder(c_dim, size, pad, DEV)
    for k, (name, window) in enumerate(sorted(_windows(*src).items())):          # windows that are up- and down-scaled
        mirror, vflip, reverse = bool(k & 1), bool(k & 2), bool(k & 4)           # all four mirror x vflip combinations, twice
        aug = _record(k, T, window, vflip, flicker=k % 3 != 0)
        want = host_clip(frames, c_dim, size, pad, mirror, reverse, aug)
        got = builder.build(clip_pipeline.collate_raw([raw_item(frames, mirror, reverse, aug)]))
        assert tuple(got.shape) == (1, T, c_dim, size[0] + pad[0], size[1] + pad[1]) and got.dtype == torch.float32
        assert torch.equal(got[0].cpu(), want), (name, window, mirror, vflip, reverse)


@pytest.mark.parametrize('c_dim', [1, 3])
def test_ragged_batch_equals_per_clip_results(c_dim):
    rng = np.random.RandomState(3)
    size, pad, T = (32, 48), (4, 8), 4
    clips = [(_frames(rng, T, 60, 80), True, False, _record(1, T, (7, 9, 41, 33), True)),
             (_frames(rng, T, 17, 23), False, True, _record(2, T, (0, 0, 17, 23), False, flicker=False)),
             (_frames(rng, T, 32, 48), True, True, _record(3, T, (30, 1, 2, 40), True))]
    items = [raw_item(*c) for c in clips]
    builder = clip_pipeline.DeviceClipBuilder(c_dim, size, pad, DEV)
    together = builder.build(clip_pipeline.collate_raw(items)).cpu()
    for i, (frames, mirror, reverse, aug) in enumerate(clips):
        assert torch.equal(together[i], host_clip(frames, c_dim, size, pad, mirror, reverse, aug))
        assert torch.equal(builder.build(clip_pipeline.collate_raw([items[i]])).cpu()[0], together[i])        # batch independence
    assert torch.equal(builder.build(clip_pipeline.collate_items(items)).cpu(), together)       # packed straight into pinned staging
    # a batch without records takes the existing entry, on the same builder
    plain = builder.build(clip_pipeline.collate_raw([raw_item(clips[0][0], True, False)])).cpu()
    assert torch.equal(plain[0], _ClipReader(c_dim, list(size), list(pad)).clip(_ArrayVideo(clips[0][0], 't'), range(T), True, False))


def test_the_neutral_setting_equals_the_existing_entry_bit_for_bit():
    rng = np.random.RandomState(8)
    for c_dim in (1, 3):
        for src, size, pad in (((60, 80), (32, 48), (4, 8)), ((37, 53), (30, 33), (3, 5)), ((128, 128), (128, 128), (0, 0))):
            frames = _frames(rng, 3, *src)
            neutral = dict(_record(0, 3, (0, 0) + src, False, flicker=False), gamma=1.0, gain=1.0, offset=0.0)
            builder = clip_pipeline.DeviceClipBuilder(c_dim, size, pad, DEV)
            for mirror in (False, True):
                old = builder.build(clip_pipeline.collate_raw([raw_item(frames, mirror, False)]))
                new = builder.build(clip_pipeline.collate_raw([raw_item(frames, mirror, False, neutral)]))
                assert torch.equal(old, new), (c_dim, src, size, mirror)


class _Direct(object):
    """One augmented batch launched through the C ABI into a caller's buffer: the output sits ``shift`` floats behind a 16-byte boundary,
    inside guard bands of SENTINEL."""

    def __init__(self, items, c_dim, size, pad, shift=0, guard=256):
        self.batch = clip_pipeline.collate_raw(items)
        self.n = self.batch['B'] * self.batch['T']
        self.n_tables = self.batch['n_tables']
        self.head = clip_pipeline.aug_header_bytes(self.n)
        self.first = self.head + self.n_tables * clip_pipeline.TABLE_BYTES
        self.host = self.batch['packed']
        self.dev = self.host.to(DEV)
        self.levels = clip_pipeline.level_tables().to(DEV)
        self.c_dim, (self.H, self.W), (self.ph, self.pw) = c_dim, size, pad
        self.shape = (self.batch['B'], self.batch['T'], c_dim, self.H + self.ph, self.W + self.pw)
        self.numel = int(np.prod(self.shape))
        self.buf = torch.full((guard + shift + self.numel + guard,), SENTINEL, device=DEV)
        assert self.buf.data_ptr() % 16 == 0 and guard % 4 == 0
        self.lo = guard + shift

    def launch(self, stream=None):
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        rc = _native.lib().tai_clip_from_frames_aug(self.dev.data_ptr() + self.first, self.dev.numel() - self.first, self.dev.data_ptr(),
                                                    self.host.data_ptr(), self.dev.data_ptr() + self.head, self.n_tables,
                                                    self.levels.data_ptr(), self.buf.data_ptr() + 4 * self.lo, self.n, self.c_dim, self.H,
                                                    self.W, self.ph, self.pw, s)
        _native.check(rc, 'tai_clip_from_frames_aug')

    def out(self):
        torch.cuda.synchronize()
        b = self.buf.cpu()
        assert (b[:self.lo] == SENTINEL).all() and (b[self.lo + self.numel:] == SENTINEL).all()          # the guard bands stand
        return b[self.lo:self.lo + self.numel].view(self.shape).clone()

    def device_table(self):
        return self.dev[:self.n * clip_pipeline.AUG_DESC_INTS * 8].view(torch.int64).view(self.n, clip_pipeline.AUG_DESC_INTS)


@pytest.mark.parametrize('c_dim', [1, 3])
@pytest.mark.parametrize('size,pad,shift', [((30, 33), (3, 5), 0), ((30, 33), (3, 5), 1), ((32, 32), (0, 0), 1), ((32, 32), (0, 0), 3),
                                            ((32, 32), (0, 0), 0), ((5, 3), (0, 0), 2)])
def test_guard_bands_misaligned_output_and_row_tails(size, pad, shift, c_dim):
    # W + pad_w = 38 or 3: single words at the row tails; shift != 0: an output base that is not 16-byte aligned takes single words too
    rng = np.random.RandomState(shift + c_dim)
    clips = [(_frames(rng, 2, 37, 53), True, False, _record(4, 2, (3, 4, 30, 40), True)),
             (_frames(rng, 2, 20, 16), False, True, _record(5, 2, (0, 0, 20, 16), False))]
    d = _Direct([raw_item(*c) for c in clips], c_dim, size, pad, shift)
    d.launch()
    got = d.out()
    for i, (frames, mirror, reverse, aug) in enumerate(clips):
        assert torch.equal(got[i], host_clip(frames, c_dim, size, pad, mirror, reverse, aug))


@pytest.mark.parametrize('c_dim', [1, 3])
def test_more_items_than_the_grid_cap(c_dim):
    # 4 x 4 outputs: one (frame, band) item per frame; 2050 frames against a grid cap of 2048, so two workgroups walk a second item
    T = 2050
    frames = _frames(np.random.RandomState(2), T, 5, 6)
    aug = _record(6, T, (1, 1, 3, 4), True)
    d = _Direct([raw_item(frames, True, False, aug)], c_dim, (4, 4), (0, 0))
    d.launch()
    assert torch.equal(d.out()[0], host_clip(frames, c_dim, (4, 4), (0, 0), True, False, aug))


@pytest.mark.parametrize('c_dim', [1, 3])
def test_frame_i_of_a_flicker_clip_reads_table_i_and_padding_is_the_neutral_level(c_dim):
    T, size, pad = 4, (9, 10), (2, 3)
    rng = np.random.RandomState(1)
    items = [raw_item(_frames(rng, T, 12, 14), False, False, _record(7, T, (0, 0, 12, 14), False)),
             raw_item(_frames(rng, T, 8, 8), True, False, _record(8, T, (1, 1, 6, 6), True))]
    d = _Direct(items, c_dim, size, pad)
    assert d.n_tables == 2 * T
    # every table maps every level to one constant of its own: row 0 for colour; (c + 0) + 0 for gray
    consts = torch.arange(1, 2 * T + 1, dtype=torch.float32) / 16
    tables = torch.zeros(2 * T, 4, 256)
    tables[:, 0] = consts[:, None]
    tables[:, 1] = consts[:, None]
    d.dev[d.head:d.first].copy_(tables.view(-1).view(torch.uint8).to(DEV))
    d.launch()
    got = d.out().view(2 * T, c_dim, size[0] + pad[0], size[1] + pad[1])
    neutral = clip_pipeline.level_tables()
    padding = -1.0 if c_dim == 3 else ((neutral[1, 0] + neutral[2, 0]) + neutral[3, 0]).item()
    for i in range(2 * T):
        assert (got[i, :, :size[0], :size[1]] == consts[i]).all(), i
        assert (got[i, :, size[0]:, :] == padding).all() and (got[i, :, :, size[1]:] == padding).all()


def test_graph_replay_equals_eager_and_a_descriptor_spoilt_under_the_graph_gives_padding_for_its_frame_only():
    rng = np.random.RandomState(9)
    c_dim, size, pad, T = 3, (16, 20), (1, 3), 3
    clips = [(_frames(rng, T, 24, 30), True, False, _record(9, T, (2, 3, 20, 21), True)),
             (_frames(rng, T, 18, 18), False, True, _record(10, T, (0, 0, 18, 18), False))]
    d = _Direct([raw_item(*c) for c in clips], c_dim, size, pad)
    d.launch()                                                                     # warm-up outside the capture
    eager = d.out()
    for i, (frames, mirror, reverse, aug) in enumerate(clips):
        assert torch.equal(eager[i], host_clip(frames, c_dim, size, pad, mirror, reverse, aug))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d.launch(torch.cuda.current_stream().cuda_stream)
    d.buf.fill_(SENTINEL)
    graph.replay()
    assert torch.equal(d.out(), eager)
    # the host copy was validated at capture; the device copy changes afterwards.  Frame 4 (clip 1, t = 1): h x w = 18 x 18, 6 tables
    table, good = d.device_table(), d.device_table()[4].clone()
    frames_bytes = d.dev.numel() - d.first
    padded = eager.clone().view(2 * T, c_dim, 17, 23)
    padded[4] = -1.0
    spoilt = {0: frames_bytes - 10, 1: 1 << 23, 2: 0, 4: 1, 5: -1, 6: 0, 7: 19, 8: 2 * T}
    for field, value in sorted(spoilt.items()) + [(0, -8), (4, 1 << 40), (8, -1), (6, 1 << 33)]:
        table[4] = good
        table[4, field] = value
        d.buf.fill_(SENTINEL)
        graph.replay()
        assert torch.equal(d.out().view(2 * T, c_dim, 17, 23), padded), (field, value)
    table[4] = good
    graph.replay()
    assert torch.equal(d.out(), eager)


# ---------------------------------------------------------------------------------------------------------------- train.py

SPEC = '{"class": "TAIFillInModel", "args": [4, 1, 3, 51], "kwargs": {"num_block": 5, "kf_dim": 2}}'
AUG = ['--aug_crop', '0.5', '--aug_vflip', '--aug_brightness', '0.2', '--aug_contrast', '0.3', '--aug_gamma', '0.5', '--aug_flicker', '0.1']


def _video_list(tmp_path):
    rng = np.random.RandomState(21)
    lines = []
    for i in range(5):                      # two batches of two per epoch: update 3 enters epoch 1
        base = rng.randint(0, 256, (40 + i, 48, 3)).astype(np.uint8)
        np.save(tmp_path / ('clip%d.npy' % i), np.stack([np.roll(base, 2 * t, axis=1) for t in range(10 + i)]))
        lines.append(str(tmp_path / ('clip%d.npy' % i)))
    (tmp_path / 'list.txt').write_text('\n'.join(lines) + '\n')
    return str(tmp_path / 'list.txt')


def _train(tmp_path, capsys, name, max_iter, extra):
    import train
    capsys.readouterr()
    train.main(['--name', name, '--K', '3', '--T', '2', '--F', '3', '--c_dim', '1', '--image_size', '32', '--model_key', SPEC,
                '--checkpoints_dir', str(tmp_path / 'ckpt'), '--batch_size', '2', '--max_iter', str(max_iter), '--print_freq', '1',
                '--df_dim', '8', '--resumable', '--train_video_list_path', _video_list(tmp_path), '--num_threads', '0'] + list(extra))
    return capsys.readouterr().out


def _states(out):
    return dict((int(i), s) for i, s in re.findall(r'^iter (\d+) .* state=([0-9a-f]{16})$', out, re.M))


def _losses(out):
    return re.findall(r'^iter \d+ \S+ \S+  (.*) state=', out, re.M)


def test_train_host_and_device_pipeline_print_the_same_states_and_the_flags_reach_the_data(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    calls = []
    L = _native.lib()
    real = L.tai_clip_from_frames_aug
    monkeypatch.setattr(L, 'tai_clip_from_frames_aug', lambda *a: calls.append(a[5]) or real(*a))
    host = _train(tmp_path, capsys, 'host', 4, AUG)
    assert not calls
    dev = _train(tmp_path, capsys, 'dev', 4, AUG + ['--device_preprocess'])
    assert calls == [2 * 8] * 4                                              # one launch per update, a table per frame (flicker)
    assert sorted(_states(host)) == [1, 2, 3, 4] and _states(host) == _states(dev) and _losses(host) == _losses(dev)
    plain = _train(tmp_path, capsys, 'plain', 4, ['--device_preprocess'])
    assert len(calls) == 4                                                   # flags off: the existing entry, nothing new launched
    assert len(_losses(plain)) == 4 and all(a != b for a, b in zip(_losses(plain), _losses(dev)))
    assert set(_states(plain).values()).isdisjoint(_states(dev).values())
    # the saved data state carries the settings only when augmentation is on
    load = lambda name: torch.load(str(tmp_path / 'ckpt' / name / 'model_latest.ckpt'), map_location='cpu', weights_only=False)
    assert load('dev')['run_state']['ranks'][0]['data']['augment'] == ClipAugment(**FULL).state()
    assert 'augment' not in load('plain')['run_state']['ranks'][0]['data']


@pytest.mark.parametrize('extra', [['--device_preprocess'],
                                   ['--guard', '--clip_grad_norm', '1', '--fused_step', '--ema_decay', '0.99', '--census_weight', '0.5']],
                         ids=['device', 'host-guard-fused-ema-census'])
def test_train_cut_in_two_ends_with_the_digest_of_the_straight_run(tmp_path, capsys, monkeypatch, extra):
    monkeypatch.chdir(tmp_path)
    straight = _states(_train(tmp_path, capsys, 'A', 4, AUG + extra))
    first = _states(_train(tmp_path, capsys, 'B', 2, AUG + extra))
    out = _train(tmp_path, capsys, 'B', 4, AUG + extra)
    assert 'carries no run_state' not in out and 'falling back' not in out
    assert sorted(first) == [1, 2] and sorted(_states(out)) == [3, 4] and straight == {**first, **_states(out)}
    assert len(set(straight.values())) == 4
    # a continuation with other settings is refused, both values named
    with pytest.raises(ValueError, match=r"augment = .*'crop': 0\.5.*this run has .*'crop': 0\.75"):
        _train(tmp_path, capsys, 'B', 6, ['--aug_crop', '0.75'] + AUG[2:] + extra)
