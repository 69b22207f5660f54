"""--device_preprocess through the drivers: train.py hands env.train_step the same tensors, predict.py writes the same files and
prints the same scores, and a list-backed validation pass scores the same table -- on a small list of .npy / frame-directory
"videos" of two source sizes, gray and colour."""
import argparse
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import video_frame_inpainting_amd as vfi
from video_frame_inpainting_amd import validation
from video_frame_inpainting_amd.environments import create_eval_environment

pytestmark = pytest.mark.gpu

K, T, F, SIZE = 3, 2, 3, 32
SPEC = {1: '{"class": "TAIFillInModel", "args": [4, 1, 3, 51], "kwargs": {"num_block": 5, "kf_dim": 2}}',
        3: '{"class": "TAIFillInModel", "args": [4, 3, 3, 51], "kwargs": {"num_block": 5, "kf_dim": 2}}'}


def _smooth(rng, t, h, w):
    """Moving blobs rather than noise, so that predictions and PSNR values are ordinary numbers."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    frames = np.zeros((t, h, w, 3))
    for c in range(3):
        cx, cy, vx, vy = rng.uniform(0.2, 0.8) * w, rng.uniform(0.2, 0.8) * h, rng.uniform(-2, 2), rng.uniform(-2, 2)
        for k in range(t):
            frames[k, :, :, c] = 255 * np.exp(-((x - cx - vx * k) ** 2 + (y - cy - vy * k) ** 2) / (2 * (0.2 * w) ** 2))
    return np.clip(frames + rng.uniform(0, 20, frames.shape), 0, 255).astype(np.uint8)


def _write_videos(root, exact_spans):
    """Two .npy videos (40x56, 32x32) and a directory of 24x40 PNG frames -> the list file.  ``exact_spans``: every line names a span of
    exactly K + T + F frames (the form of the reference's test lists: the dataset draws nothing)."""
    rng = np.random.RandomState(21)
    n = K + T + F
    np.save(str(root / 'wide.npy'), _smooth(rng, 14, 40, 56))
    np.save(str(root / 'same.npy'), _smooth(rng, 12, SIZE, SIZE))
    os.makedirs(str(root / 'dir'))
    for i, f in enumerate(_smooth(rng, 11, 24, 40)):
        Image.fromarray(f).save(str(root / 'dir' / ('%04d.png' % i)))
    if exact_spans:
        lines = ['%s 2-%d' % (root / 'wide.npy', 1 + n), '%s 1-%d' % (root / 'same.npy', n), '%s 3-%d' % (root / 'dir', 2 + n),
                 '%s 5-%d' % (root / 'wide.npy', 4 + n), '%s 4-%d' % (root / 'same.npy', 3 + n)]
    else:
        lines = [str(root / 'wide.npy'), '%s 2-12' % (root / 'same.npy'), str(root / 'dir'), '%s 3-14' % (root / 'wide.npy')]
    path = root / ('list_%s.txt' % ('exact' if exact_spans else 'free'))
    path.write_text('\n'.join(lines) + '\n')
    return str(path)


def _common(tmp_path, name, c_dim):
    return ['--name', name, '--K', str(K), '--T', str(T), '--F', str(F), '--c_dim', str(c_dim), '--image_size', str(SIZE),
            '--model_key', SPEC[c_dim], '--checkpoints_dir', str(tmp_path / 'ckpt'), '--num_threads', '0']


@pytest.mark.parametrize('c_dim', [1, 3])
def test_train_hands_over_the_same_tensors(tmp_path, monkeypatch, c_dim):
    import train
    monkeypatch.chdir(tmp_path)
    video_list = _write_videos(tmp_path, exact_spans=False)
    real = train.create_training_environment

    def run(name, extra):                   # a name of its own: the second run must not resume the first one's snapshot
        seen = []

        def create(*a, **k):
            env = real(*a, **k)
            step = env.train_step

            def train_step(preceding, following, middle):
                seen.append([x.detach().cpu().clone() for x in (preceding, following, middle)])
                return step(preceding, following, middle)
            env.train_step = train_step
            return env
        monkeypatch.setattr(train, 'create_training_environment', create)
        train.main(_common(tmp_path, name, c_dim) + ['--batch_size', '2', '--max_iter', '3', '--df_dim', '8', '--train_video_list_path', video_list,
                                                                 '--save_latest_freq', '1000'] + extra)
        return seen

    host, device = run('host', []), run('device', ['--device_preprocess'])
    assert len(host) == len(device) == 3
    for a, b in zip(host, device):
        for x, y in zip(a, b):
            assert x.shape == y.shape and x.dtype == y.dtype == torch.float32
            assert torch.equal(x, y)
    assert not torch.equal(host[0][0], host[1][0])          # the updates saw different clips


def _predict(tmp_path, capsys, name, c_dim, video_list, out, extra=()):
    import predict
    capsys.readouterr()
    predict.main(_common(tmp_path, name, c_dim) + ['--batch_size', '2', '--test_video_list_path', video_list, '--qual_result_root',
                                                   str(out), '--random_init', '--intermediate_preds'] + list(extra))
    text = capsys.readouterr().out
    files = {}
    for d, _, names in os.walk(str(out)):
        for f in names:
            files[os.path.relpath(os.path.join(d, f), str(out))] = open(os.path.join(d, f), 'rb').read()
    return text, files


@pytest.mark.parametrize('c_dim,pad', [(1, 0), (3, 0), (3, 32)])
def test_predict_writes_the_same_files_and_scores(tmp_path, capsys, monkeypatch, c_dim, pad):
    monkeypatch.chdir(tmp_path)
    video_list = _write_videos(tmp_path, exact_spans=True)
    extra = ['--padding_size', str(pad)]
    text_a, host_a = _predict(tmp_path, capsys, 'p', c_dim, video_list, tmp_path / 'host_a', extra)
    text_b, host_b = _predict(tmp_path, capsys, 'p', c_dim, video_list, tmp_path / 'host_b', extra)
    text_d, dev = _predict(tmp_path, capsys, 'p', c_dim, video_list, tmp_path / 'dev', extra + ['--device_preprocess'])
    assert sorted(dev) == sorted(host_a) and len(dev) >= 5 * (K + T + F + T)
    assert any(f.endswith(os.path.join('', 'pred_middle_%04d.png' % K)) for f in dev)
    for f in sorted(host_a):
        if os.path.basename(f).startswith('gt_'):
            assert dev[f] == host_a[f], f
    self_identical = all(host_a[f] == host_b[f] for f in host_a)
    print('default path self-identical at this shape: %s' % self_identical)
    for f in sorted(host_a):
        if os.path.basename(f).startswith('gt_'):
            continue
        if self_identical:
            assert dev[f] == host_a[f], f
        else:       # the forward is not reproducible at this small shape: decoded pixels to within one grey level
            a = np.asarray(Image.open(os.path.join(str(tmp_path / 'host_a'), f))).astype(np.int64)
            d = np.asarray(Image.open(os.path.join(str(tmp_path / 'dev'), f))).astype(np.int64)
            assert a.shape == d.shape and np.abs(a - d).max() <= 1, f
    line = re.compile(r'^rank 0: PSNR (\S+) \+- (\S+) dB, SSIM (\S+) \+- (\S+) over 5 clips$', re.M)
    ma, md = line.search(text_a), line.search(text_d)
    assert ma and md, (text_a, text_d)
    if self_identical:
        assert ma.group(1) == md.group(1) and ma.group(2) == md.group(2)
    else:
        assert abs(float(ma.group(1)) - float(md.group(1))) <= 0.05
    assert '# testing videos = 5 (rank 0 of 1 owns 5)' in text_d


@pytest.mark.parametrize('c_dim', [1, 3])
def test_list_backed_validation_scores_the_same_table(tmp_path, monkeypatch, c_dim):
    monkeypatch.chdir(tmp_path)
    video_list = _write_videos(tmp_path, exact_spans=False)
    torch.manual_seed(0)
    env = create_eval_environment(vfi.create_model(SPEC[c_dim]), str(tmp_path / 'ckpt'), 'v', 'none.ckpt', [0, 0],
                                  device=torch.device('cuda:0'), load_snapshot=False)
    leg = validation.Leg('T', K, T, F, video_list)

    def run(on_device):
        opt = argparse.Namespace(c_dim=c_dim, image_size=[SIZE, SIZE], padding_size=[0, 0], batch_size=3, num_threads=0, seed=1002,
                                 device_preprocess=on_device)
        return validation.run_leg(env, leg, opt, rank=0, world=1)

    (psnr_h, ssim_h, l2_h), (psnr_d, ssim_d, l2_d) = run(False), run(True)
    assert psnr_h.shape == (4, T)
    assert np.array_equal(psnr_h, psnr_d)
    assert np.abs(ssim_h - ssim_d).max() <= 1e-12
    assert np.isfinite(psnr_h).all()
