"""train.py's validation: the legs run every --validate_freq updates, model_best.ckpt holds the sums of the best first-leg
validation (recomputed here from the snapshot with the host metric), predict.py loads it by default, the graphed training step
survives validation passes, a resumed run keeps the stored best values, and a run without a validation source writes no
model_best.ckpt."""
import os
import re

import numpy as np
import pytest
import torch

import video_frame_inpainting_amd as vfi
from video_frame_inpainting_amd import metrics, validation
from video_frame_inpainting_amd.environments import create_eval_environment

pytestmark = pytest.mark.gpu

SPEC = '{"class": "TAIFillInModel", "args": [4, 1, 3, 51], "kwargs": {"num_block": 5, "kf_dim": 2}}'
K, T, F, SIZE, SEED = 3, 2, 3, 32, 1002


def _common(tmp_path, name):
    return ['--name', name, '--K', str(K), '--T', str(T), '--F', str(F), '--c_dim', '1', '--image_size', str(SIZE),
            '--model_key', SPEC, '--checkpoints_dir', str(tmp_path / 'ckpt')]


def _train(tmp_path, capsys, name, max_iter, extra=()):
    import train
    capsys.readouterr()
    train.main(_common(tmp_path, name) + ['--batch_size', '2', '--max_iter', str(max_iter), '--synthetic', '4',
                                          '--print_freq', '1', '--df_dim', '8'] + list(extra))
    return capsys.readouterr().out


def _ckpt(tmp_path, name, file):
    return torch.load(str(tmp_path / 'ckpt' / name / file), map_location='cpu', weights_only=False)


def _printed_sums(out, leg='T'):
    """(sum_avg_psnr, sum_avg_ssim) of every validation of ``leg``, in order."""
    return [(float(p), float(s)) for p, s in
            re.findall(r'^val %s \(K,T,F\).* sum_avg_psnr=(\S+) sum_avg_ssim=(\S+)$' % leg, out, re.M)]


def _expected_best(sums, start=(0, 0)):
    best, at = start, None
    for i, (p, s) in enumerate(sums):
        if s > best[1]:
            best, at = (p, s), i
    return best, at


def _recompute(tmp_path, name):
    """Load model_best.ckpt into an evaluation environment, run the validation clips in the training run's batches, score
    them with the host metric."""
    env = create_eval_environment(vfi.create_model(SPEC), str(tmp_path / 'ckpt'), name, 'model_best.ckpt', [0, 0],
                                  device=torch.device('cuda:0'))
    clips = validation.synthetic_clips(3, K, T, F, 1, SIZE, SIZE, SEED)
    rows = []
    for i in range(0, 3, 2):
        batch = clips[i:i + 2]
        env.set_test_inputs(batch[:, :K], batch[:, K + T:])
        env.T = T
        env.eval()
        env.forward_test()
        rows.append(metrics.compute_errors(env.gen_output['pred'].cpu().numpy(), batch[:, K:K + T].numpy()))
    psnr = np.concatenate([r[0] for r in rows])
    ssim = np.concatenate([r[1] for r in rows])
    return validation.sum_avg(psnr), validation.sum_avg(ssim)


def _check_run(tmp_path, out, name, max_iter):
    assert out.count('Validation (T=%d) done.' % T) == 2 * max_iter       # the T leg and the alt-K/F leg (same T)
    assert out.count('Validation (T=1) done.') == max_iter                   # the alt-T leg
    sums = _printed_sums(out)
    assert len(sums) == max_iter and len(_printed_sums(out, 'altT')) == max_iter and len(_printed_sums(out, 'altKF')) == max_iter
    best, at = _expected_best(sums)
    assert at is not None, sums
    snap = _ckpt(tmp_path, name, 'model_best.ckpt')
    assert snap['updates'] == at + 1
    assert (snap['sum_avg_psnr_err'], snap['sum_avg_ssim_err']) == best
    p, s = _recompute(tmp_path, name)
    assert abs(p - snap['sum_avg_psnr_err']) <= 1e-12 * max(1.0, abs(p))
    assert abs(s - snap['sum_avg_ssim_err']) <= 1e-12
    latest = _ckpt(tmp_path, name, 'model_latest.ckpt')
    assert latest['updates'] == max_iter and (latest['sum_avg_psnr_err'], latest['sum_avg_ssim_err']) == best
    return best


VAL = ['--val_synthetic', '3', '--validate_freq', '1', '--alt_T', '1', '--alt_K', '2', '--alt_F', '2']


def test_validation_keeps_best_snapshot_predict_loads_it_and_resume_carries_it(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    out = _train(tmp_path, capsys, 'val', 3, VAL)
    _check_run(tmp_path, out, 'val', 3)

    import predict
    predict.main(_common(tmp_path, 'val') + ['--batch_size', '2', '--synthetic', '3', '--qual_result_root', str(tmp_path / 'res')])
    assert 'model_best.ckpt' in capsys.readouterr().out
    assert os.path.isfile(tmp_path / 'res' / 'synthetic_000002' / 'pred_middle_0003.png')

    # resume: the stored best (made unbeatable here) carries over, so no later validation replaces model_best.ckpt
    path = tmp_path / 'ckpt' / 'val' / 'model_latest.ckpt'
    latest = _ckpt(tmp_path, 'val', 'model_latest.ckpt')
    latest['sum_avg_psnr_err'], latest['sum_avg_ssim_err'] = 123.0, 1e9
    torch.save(latest, str(path))
    before = open(tmp_path / 'ckpt' / 'val' / 'model_best.ckpt', 'rb').read()
    out = _train(tmp_path, capsys, 'val', 5, VAL)
    assert len(_printed_sums(out)) == 2 and 'Current model has best SSIM' not in out
    assert open(tmp_path / 'ckpt' / 'val' / 'model_best.ckpt', 'rb').read() == before
    latest = _ckpt(tmp_path, 'val', 'model_latest.ckpt')
    assert latest['updates'] == 5 and (latest['sum_avg_psnr_err'], latest['sum_avg_ssim_err']) == (123.0, 1e9)


def test_validation_with_graph_step(tmp_path, capsys, monkeypatch):
    # updates 1-2 eager, 3 captured and replayed, 4 replayed after a validation pass
    monkeypatch.chdir(tmp_path)
    out = _train(tmp_path, capsys, 'valg', 4, VAL + ['--graph_step'])
    _check_run(tmp_path, out, 'valg', 4)


def test_no_validation_source_writes_no_best_snapshot(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    out = _train(tmp_path, capsys, 'noval', 2, ['--validate_freq', '1'])
    assert 'Validation' not in out
    assert not (tmp_path / 'ckpt' / 'noval' / 'model_best.ckpt').exists()
    latest = _ckpt(tmp_path, 'noval', 'model_latest.ckpt')
    assert (latest['updates'], latest['sum_avg_psnr_err'], latest['sum_avg_ssim_err']) == (2, 0, 0)
