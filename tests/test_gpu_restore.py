"""restore.py end to end on a small damaged video: the report flags the damage with the right bits, every gap frame is, byte for byte, what
``env.forward_test`` gives on that gap's context called directly, and every other frame is the pipeline's own pixels of the source frame."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import clip_pipeline  # noqa: E402
from video_frame_inpainting_amd.environments import create_eval_environment  # noqa: E402
from video_frame_inpainting_amd.restore import BLANK, DUPLICATE, LISTED, MISSING  # noqa: E402

pytestmark = pytest.mark.gpu

K, T, F, SIZE, N = 3, 2, 3, 32, 40
SPEC = {1: '{"class": "TAIFillInModel", "args": [4, 1, 3, 51], "kwargs": {"num_block": 5, "kf_dim": 2}}',
        3: '{"class": "TAIFillInModel", "args": [4, 3, 3, 51], "kwargs": {"num_block": 5, "kf_dim": 2}}'}
DEV = torch.device('cuda:0')


def _smooth(rng, t, h, w):
    """The moving blobs plus noise of tests/test_gpu_device_preprocess_drivers.py."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    frames = np.zeros((t, h, w, 3))
    for c in range(3):
        cx, cy, vx, vy = rng.uniform(0.2, 0.8) * w, rng.uniform(0.2, 0.8) * h, rng.uniform(-2, 2), rng.uniform(-2, 2)
        for k in range(t):
            frames[k, :, :, c] = 255 * np.exp(-((x - cx - vx * k) ** 2 + (y - cy - vy * k) ** 2) / (2 * (0.2 * w) ** 2))
    return np.clip(frames + rng.uniform(0, 20, frames.shape), 0, 255).astype(np.uint8)


def _write_dir(root, frames, skip=()):
    os.makedirs(str(root))
    for i, f in enumerate(frames):
        if i not in skip:
            Image.fromarray(f).save(os.path.join(str(root), '%04d.png' % i))


def _damage(frames):
    """-> (the frames on disk, the frames as the source delivers them): 10-11 copies of 9, 20 constant, 30 and 31 absent (delivered as 29)."""
    disk = frames.copy()
    disk[10] = disk[11] = disk[9]
    disk[20] = 77
    delivered = disk.copy()
    delivered[30] = delivered[31] = disk[29]
    return disk, delivered


def _restore(tmp_path, src, out, c_dim=1, extra=()):
    import restore as cli
    report = cli.main(['--name', 'r', '--K', str(K), '--T', str(T), '--F', str(F), '--c_dim', str(c_dim), '--image_size', str(SIZE),
                       '--model_key', SPEC[c_dim], '--checkpoints_dir', str(tmp_path / 'ckpt'), '--random_init', '--input', str(src),
                       '--output_dir', str(out)] + list(extra))
    names = sorted(f for f in os.listdir(str(out)) if f.endswith('.png'))
    assert names == ['frame_%06d.png' % i for i in range(report['n_frames'])] and os.path.isfile(str(out / 'report.json'))
    frames = np.stack([np.asarray(Image.open(str(out / f))) for f in names])
    return report, frames if frames.ndim == 4 else frames[..., None]


class Direct(object):
    """The model restore.py builds (same seed, same constructor), the pipeline's frames of a delivered video and the forward called
    directly on a batch of gaps."""

    def __init__(self, tmp_path, delivered, c_dim=1):
        torch.manual_seed(0)
        self.env = create_eval_environment(vfi.create_model(SPEC[c_dim]), str(tmp_path / 'ckpt'), 'r', 'model_best.ckpt', [0, 0], device=DEV,
                                           load_snapshot=False)
        builder = clip_pipeline.DeviceClipBuilder(c_dim, [SIZE, SIZE], [0, 0], DEV)
        batch = {'items': [{'frames': torch.from_numpy(delivered), 'mirror': False}], 'B': 1, 'T': len(delivered)}
        self.video = builder.build(batch)[0]
        self.rgb = c_dim == 3
        self.pixels = clip_pipeline.to_uint8_host(self.video, SIZE, SIZE, self.rgb)

    def forward(self, starts, k, t, f):
        env = self.env
        env.set_test_inputs(torch.stack([self.video[s - k:s] for s in starts]), torch.stack([self.video[s + t:s + t + f] for s in starts]))
        env.T = t
        env.eval()
        env.forward_test()
        return clip_pipeline.to_uint8_host(env.gen_output['pred'], SIZE, SIZE, self.rgb)


FLAGS = {5: LISTED, 10: DUPLICATE, 11: DUPLICATE, 20: BLANK, 30: MISSING | DUPLICATE, 31: MISSING | DUPLICATE}
GAPS = [(5, 1), (10, 2), (20, 1), (30, 2)]
ALL = ['--detect', 'missing,dup,blank', '--gaps', '5-5']


@pytest.mark.parametrize('c_dim', [1, 3])
def test_every_gap_frame_is_the_direct_forward_and_every_other_frame_the_pipelines_pixels(tmp_path, c_dim):
    disk, delivered = _damage(_smooth(np.random.RandomState(5), N, SIZE, SIZE))
    _write_dir(tmp_path / 'video', disk, skip=(30, 31))
    report, frames = _restore(tmp_path, tmp_path / 'video', tmp_path / 'out', c_dim, ALL + ['--batch_size', '1', '--chunk_frames', '16'])
    assert [f['flags'] for f in report['frames']] == [FLAGS.get(i, 0) for i in range(N)]
    assert [(g['start'], g['T'], g['K'], g['F'], g['status']) for g in report['gaps']] == [(s, t, K, F, 'fill') for s, t in GAPS]
    direct = Direct(tmp_path, delivered, c_dim)
    assert frames.shape == direct.pixels.shape == (N, SIZE, SIZE, c_dim)
    for s, t in GAPS:
        want = direct.forward([s], K, t, F)[0]
        for p in range(s, s + t):
            assert np.array_equal(frames[p], want[p - s]), p
            assert not np.array_equal(frames[p], direct.pixels[p])
    for p in set(range(N)) - set(FLAGS):
        assert np.array_equal(frames[p], direct.pixels[p]), p


def test_two_gaps_of_one_shape_are_the_direct_forward_on_that_batch_of_two(tmp_path):
    disk, delivered = _damage(_smooth(np.random.RandomState(5), N, SIZE, SIZE))
    _write_dir(tmp_path / 'video', disk, skip=(30, 31))
    report, frames = _restore(tmp_path, tmp_path / 'video', tmp_path / 'out', 1, ALL + ['--batch_size', '2'])
    assert [g['status'] for g in report['gaps']] == ['fill'] * 4
    direct = Direct(tmp_path, delivered)
    for starts, t in (([5, 20], 1), ([10, 30], 2)):        # the groups (K, T, F) = (3, 1, 3) and (3, 2, 3), each one batch
        want = direct.forward(starts, K, t, F)
        for b, s in enumerate(starts):
            for p in range(s, s + t):
                assert np.array_equal(frames[p], want[b, p - s]), p
    for p in set(range(N)) - set(FLAGS):
        assert np.array_equal(frames[p], direct.pixels[p]), p
    # a .npy source has no missing frames: the repeats at 30-31 are found as duplicates, and the frames written are the same
    np.save(str(tmp_path / 'video.npy'), delivered)
    report_npy, frames_npy = _restore(tmp_path, tmp_path / 'video.npy', tmp_path / 'out_npy', 1, ALL + ['--batch_size', '2'])
    assert [f['flags'] for f in report_npy['frames']] == [FLAGS.get(i, 0) & ~MISSING for i in range(N)]
    assert [[f[k] for k in ('s1', 's2', 'sad', 'ndiff')] for f in report_npy['frames']] == \
        [[f[k] for k in ('s1', 's2', 'sad', 'ndiff')] for f in report['frames']]
    assert np.array_equal(frames_npy, frames)


def test_what_is_not_filled_is_left_as_the_source_delivered_it(tmp_path):
    clean = _smooth(np.random.RandomState(5), N, SIZE, SIZE)
    _write_dir(tmp_path / 'clean', clean)
    direct_clean = Direct(tmp_path, clean)
    # an undamaged video: no gaps, the output is the input through the pipeline
    report, frames = _restore(tmp_path, tmp_path / 'clean', tmp_path / 'out_clean', 1, ['--detect', 'missing,dup,blank'])
    assert report['gaps'] == [] and not any(f['flags'] for f in report['frames']) and np.array_equal(frames, direct_clean.pixels)
    # a gap at frames 0-1 has nothing in front of it
    report, frames = _restore(tmp_path, tmp_path / 'clean', tmp_path / 'out_start', 1, ['--gaps', '0-1'])
    assert [(g['start'], g['T'], g['K'], g['status']) for g in report['gaps']] == [(0, 2, 0, 'no_context_before')]
    assert np.array_equal(frames, direct_clean.pixels)
    # --max_T 1: the two-frame gaps are too long and stay the repeats they were; the one-frame gaps are filled
    disk, delivered = _damage(clean)
    _write_dir(tmp_path / 'video', disk, skip=(30, 31))
    report, frames = _restore(tmp_path, tmp_path / 'video', tmp_path / 'out_short', 1, ALL + ['--max_T', '1'])
    assert [(g['start'], g['status']) for g in report['gaps']] == [(5, 'fill'), (10, 'too_long'), (20, 'fill'), (30, 'too_long')]
    direct = Direct(tmp_path, delivered)
    for p in set(range(N)) - {5, 20}:
        assert np.array_equal(frames[p], direct.pixels[p]), p
    assert np.array_equal(frames[30], direct.pixels[29]) and np.array_equal(frames[11], direct.pixels[9])
    for p in (5, 20):
        assert not np.array_equal(frames[p], direct.pixels[p])
