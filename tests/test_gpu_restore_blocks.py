"""restore.py --detect_blocks end to end on a small video with damaged blocks: the report flags the planted blocks and nothing else (not the
letterbox), every composited frame is, byte for byte, the restatement applied to the direct forward's fp32 frames, the pipeline's fp32
frames and the block map, and every other frame is the pipeline's own pixels."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from damage_composite_ref import alpha_ref, core_ref, damage_composite_ref  # noqa: E402

import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import clip_pipeline  # noqa: E402
from video_frame_inpainting_amd.environments import create_eval_environment  # noqa: E402
from video_frame_inpainting_amd.restore import MOSTLY, PARTIAL, tap_tables  # noqa: E402

pytestmark = pytest.mark.gpu

K, T, F, SIZE, N, SH, SW, BS = 3, 2, 3, 32, 40, 48, 64, 16
SPEC = {1: '{"class": "TAIFillInModel", "args": [4, 1, 3, 51], "kwargs": {"num_block": 5, "kf_dim": 2}}',
        3: '{"class": "TAIFillInModel", "args": [4, 3, 3, 51], "kwargs": {"num_block": 5, "kf_dim": 2}}'}
DEV = torch.device('cuda:0')
PLANTED = {10: [[1, 2]], 11: [[1, 2]], 20: [[2, 0]]}
GAPS = [(10, 2), (20, 1)]
TAPS = tap_tables(SH, SIZE) + tap_tables(SW, SIZE)


def _video():
    """Moving blobs plus noise (tests/test_gpu_restore.py), 8 black rows at the top of EVERY frame; frames 10-11: block (1, 2) painted 77;
    frame 20: block (2, 0) copied from frame 19."""
    rng = np.random.RandomState(5)
    y, x = np.mgrid[0:SH, 0:SW].astype(np.float64)
    frames = np.zeros((N, SH, SW, 3))
    for c in range(3):
        cx, cy, vx, vy = rng.uniform(0.2, 0.8) * SW, rng.uniform(0.2, 0.8) * SH, rng.uniform(-2, 2), rng.uniform(-2, 2)
        for k in range(N):
            frames[k, :, :, c] = 255 * np.exp(-((x - cx - vx * k) ** 2 + (y - cy - vy * k) ** 2) / (2 * (0.2 * SW) ** 2))
    frames = np.clip(frames + rng.uniform(0, 20, frames.shape), 0, 255).astype(np.uint8)
    frames[:, :8] = 0
    frames[10:12, 16:32, 32:48] = 77
    frames[20, 32:48, 0:16] = frames[19, 32:48, 0:16]
    return frames


def _maps():
    maps = np.zeros((N, SH // BS, SW // BS), dtype=np.uint8)
    for i, blocks in PLANTED.items():
        for by, bx in blocks:
            maps[i, by, bx] = 1
    return maps


def _restore(tmp_path, out, c_dim=1, extra=()):
    import restore as cli
    src = tmp_path / 'video'
    if not os.path.isdir(str(src)):
        os.makedirs(str(src))
        for i, f in enumerate(_video()):
            Image.fromarray(f).save(os.path.join(str(src), '%04d.png' % i))
    report = cli.main(['--name', 'r', '--K', str(K), '--T', str(T), '--F', str(F), '--c_dim', str(c_dim), '--image_size', str(SIZE),
                       '--model_key', SPEC[c_dim], '--checkpoints_dir', str(tmp_path / 'ckpt'), '--random_init', '--input', str(src),
                       '--output_dir', str(out), '--block_size', str(BS)] + list(extra))
    names = sorted(f for f in os.listdir(str(out)) if f.endswith('.png'))
    assert names == ['frame_%06d.png' % i for i in range(N)]
    frames = np.stack([np.asarray(Image.open(str(out / f))) for f in names])
    return report, frames if frames.ndim == 4 else frames[..., None]


class Direct(object):
    """The model restore.py builds (same seed, same constructor), the pipeline's fp32 frames and pixels of the video, and the forward
    called directly on one gap: fp32 frames [T, C, H, W] and their pixels."""

    def __init__(self, tmp_path, c_dim=1):
        torch.manual_seed(0)
        self.env = create_eval_environment(vfi.create_model(SPEC[c_dim]), str(tmp_path / 'ckpt'), 'r', 'model_best.ckpt', [0, 0], device=DEV,
                                           load_snapshot=False)
        builder = clip_pipeline.DeviceClipBuilder(c_dim, [SIZE, SIZE], [0, 0], DEV)
        self.video = builder.build({'items': [{'frames': torch.from_numpy(_video()), 'mirror': False}], 'B': 1, 'T': N})[0]
        self.rgb = c_dim == 3
        self.pixels = clip_pipeline.to_uint8_host(self.video, SIZE, SIZE, self.rgb)

    def forward(self, s, t):
        env = self.env
        env.set_test_inputs(self.video[s - K:s][None], self.video[s + t:s + t + F][None])
        env.T = t
        env.eval()
        env.forward_test()
        pred = env.gen_output['pred'][0]
        return pred.float().cpu().numpy(), clip_pipeline.to_uint8_host(pred, SIZE, SIZE, self.rgb)


def _check_composited(tmp_path, report, frames, c_dim, feather):
    assert [f['flags'] for f in report['frames']] == [PARTIAL if i in PLANTED else 0 for i in range(N)]
    assert [f['blocks'] for f in report['frames']] == [PLANTED.get(i, []) for i in range(N)]
    assert [(g['start'], g['T'], g['K'], g['F'], g['status'], g['positions'], g['composited']) for g in report['gaps']] == [
        (s, t, K, F, 'fill', list(range(s, s + t)), list(range(s, s + t))) for s, t in GAPS]
    direct, maps = Direct(tmp_path, c_dim), _maps()
    video = direct.video.float().cpu().numpy()
    assert frames.shape == direct.pixels.shape == (N, SIZE, SIZE, c_dim)
    for s, t in GAPS:
        pred, pred_pixels = direct.forward(s, t)
        for p in range(s, s + t):
            want = damage_composite_ref(pred[p - s], video[p], maps[p], TAPS, BS, SIZE, SIZE, feather, direct.rgb)
            assert np.array_equal(frames[p], want), p
            D = core_ref(maps[p], TAPS, BS, SIZE, SIZE)
            A = alpha_ref(D, feather)
            assert D.any() and (A == 0).any()
            assert np.array_equal(frames[p][A == 0], direct.pixels[p][A == 0])           # untouched pixels are the pipeline's
            assert np.array_equal(frames[p][D], pred_pixels[p - s][D])                   # core pixels are the direct forward's
            assert not np.array_equal(frames[p][D], direct.pixels[p][D])
    for p in set(range(N)) - set(PLANTED):
        assert np.array_equal(frames[p], direct.pixels[p]), p
    return direct


@pytest.mark.parametrize('c_dim', [1, 3])
def test_planted_blocks_are_found_and_composited_and_the_letterbox_is_not(tmp_path, c_dim):
    report, frames = _restore(tmp_path, tmp_path / 'out', c_dim, ['--detect_blocks', 'dup,blank', '--chunk_frames', '16'])
    assert report['settings']['detect_blocks'] == ['blank', 'dup'] and report['settings']['feather'] == 4
    _check_composited(tmp_path, report, frames, c_dim, 4)


def test_feather_0_is_a_hard_replace(tmp_path):
    report, frames = _restore(tmp_path, tmp_path / 'out', 1, ['--detect_blocks', 'dup,blank', '--feather', '0', '--batch_size', '2'])
    _check_composited(tmp_path, report, frames, 1, 0)


def test_block_share_0_overwrites_the_frames_whole_and_a_damage_map_alone_composites_the_named_blocks(tmp_path):
    report, frames = _restore(tmp_path, tmp_path / 'out', 1, ['--detect_blocks', 'dup,blank', '--block_share', '0'])
    assert [f['flags'] for f in report['frames']] == [MOSTLY if i in PLANTED else 0 for i in range(N)]
    assert [g['composited'] for g in report['gaps']] == [[], []] and [(g['start'], g['T'], g['status']) for g in report['gaps']] == [
        (10, 2, 'fill'), (20, 1, 'fill')]
    direct = Direct(tmp_path, 1)
    for s, t in GAPS:
        _, pred_pixels = direct.forward(s, t)
        for p in range(s, s + t):
            assert np.array_equal(frames[p], pred_pixels[p - s]), p
    for p in set(range(N)) - set(PLANTED):
        assert np.array_equal(frames[p], direct.pixels[p]), p
    np.save(str(tmp_path / 'map.npy'), _maps())
    report, frames = _restore(tmp_path, tmp_path / 'out_map', 1, ['--damage_map', str(tmp_path / 'map.npy')])
    assert report['settings']['detect_blocks'] == [] and report['settings']['damage_map'].endswith('map.npy')
    _check_composited(tmp_path, report, frames, 1, 4)
