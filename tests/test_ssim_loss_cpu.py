"""The SSIM training loss without a GPU (train.py --ssim_weight; losses.SSIMLoss; include/tai_sepconv.h tai_ssim_loss): the numpy
restatement of the definition (ssim_loss_ref.py) against float64 autograd of the module's torch path, the flag's refusal, the term inside
a CPU MCNet environment, and the unchanged keys with the flag absent."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssim_loss_ref as ref  # noqa: E402

import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import synthetic  # noqa: E402
from video_frame_inpainting_amd.environments import create_training_environment  # noqa: E402
from video_frame_inpainting_amd.losses import SSIMLoss  # noqa: E402

SHAPES = [(1, 1, 7, 7), (2, 1, 8, 13), (5, 3, 17, 33), (2, 1, 2, 41, 37), (1, 1, 128, 128)]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', ref.KINDS)
def test_restatement_matches_float64_autograd_of_the_torch_path(kind, shape):
    """Both sides are float64 evaluations of one definition that differ in the order of the window sums (avg_pool2d against
    vertical-then-horizontal) and of the means: loss within 1e-12, gradient within 1e-10 of its maximum (worst seen: 1.4e-12).  With
    pred == gt the exact gradient is zero (SSIM is at its maximum) and what either side returns is the rounding of three cancelling terms:
    there the 1e-10 is taken of the terms' size, the only scale such a difference has."""
    pred32, gt32 = ref.make_pair(kind, shape, 17 + shape[-1])
    pred, gt = pred32.astype(np.float64), gt32.astype(np.float64)
    want = ref.ssim_loss_ref(pred, gt)
    p = torch.from_numpy(pred).requires_grad_()
    module = SSIMLoss()
    loss = module(p, torch.from_numpy(gt))
    assert loss.dtype == torch.float64 and loss.dim() == 0
    loss.backward()
    d_loss = abs(float(loss.detach()) - want['loss'])
    scale = np.abs(want['grad64']).max() if kind != 'equal' else want['term_scale']
    d_grad = np.abs(p.grad.numpy() - want['grad64']).max()
    print('%s %s: loss %.15f diff %.2e; grad max %.3e diff %.2e' % (kind, shape, float(loss.detach()), d_loss, scale, d_grad))
    assert d_loss <= 1e-12
    assert d_grad <= 1e-10 * scale
    # a single plane has no other plane to average the order noise with: a 49-term sum's order moves E[x^2] (at most 1.6 here) by a few
    # float64 ulps (16 x 2.2e-16 at the outside), and a flat plane divides that by C2 = 9e-4 in every window alike: 6e-12
    d_plane = np.abs(module.plane_ssim.numpy() - want['plane_ssim']).max()
    print('plane_ssim diff %.2e' % d_plane)
    assert d_plane <= 1e-11
    if kind == 'equal':
        assert abs(want['loss']) <= 1e-12 and np.abs(want['plane_ssim'] - 1.0).max() <= 1e-12


def test_float32_inputs_take_the_fp32_range_map_and_stay_unclipped():
    """x = (pred + 1) / 2 in fp32, then float64: the torch path on float32 tensors against the restatement on the same arrays; values
    outside [-1, 1] keep a gradient."""
    pred, gt = ref.make_pair('wide', (2, 1, 19, 23), 5)
    want = ref.ssim_loss_ref(pred, gt)
    p = torch.from_numpy(pred).requires_grad_()
    module = SSIMLoss()
    loss = module(p, torch.from_numpy(gt))
    assert loss.dtype == torch.float32
    loss.backward()
    np.testing.assert_allclose(module.plane_ssim.numpy(), want['plane_ssim'], rtol=0, atol=1e-12)
    g = want['grad64']
    assert np.all(np.abs(p.grad.numpy() - g) <= 2.0 ** -23 * np.abs(g) + 1e-9 * np.abs(g).max())       # one fp32 rounding
    outside = np.abs(pred) > 1
    assert outside.any() and np.all(p.grad.numpy()[outside] != 0)


def test_planes_below_the_window_are_refused():
    for shape in [(1, 1, 6, 32), (1, 1, 32, 6), (2, 3, 1, 1)]:
        x = torch.zeros(shape)
        with pytest.raises(ValueError):
            SSIMLoss()(x, x)
    with pytest.raises(ValueError):
        SSIMLoss()(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 9))


def test_the_module_carries_no_state():
    assert not SSIMLoss().state_dict() and not list(SSIMLoss().parameters())


def test_a_negative_weight_is_refused(monkeypatch):
    import train
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)         # the option parser's own check; nothing else is reached
    monkeypatch.setattr(train, '_run', lambda *a, **k: pytest.fail('the run was started'))
    for extra in ([], ['--resumable']):
        with pytest.raises(SystemExit) as e:
            train.main(['--name', 'x', '--K', '3', '--T', '2', '--F', '3', '--c_dim', '1', '--image_size', '32', '--batch_size', '2',
                        '--model_key', 'MCNet_gray', '--ssim_weight', '-1'] + extra)
        assert '--ssim_weight' in str(e.value) and e.value.code not in (0, None)
    with pytest.raises(ValueError, match='ssim_weight'):
        _env('unused', 'unused', ssim_weight=-1.0)


K, T, F = 3, 2, 3
_CLIPS = torch.from_numpy(synthetic.make_clips(2, K + T + F, 1, 32, 32, 77))


def _env(root, name, alpha=1.0, beta=0.02, **kw):
    torch.manual_seed(0)
    np.random.seed(0)
    return create_training_environment(vfi.MCNetFillInModel(4, 1, 3), 1, str(root), name, K, T, F, [32, 32], alpha, beta, 1e-3, 0.5, 4, 2,
                                       3, [0, 0], device='cpu', **kw)


def _forward(env):
    env.K, env.T, env.F = K, T, F
    env.train()
    env.set_train_inputs(_CLIPS[:, :K], _CLIPS[:, K + T:], _CLIPS[:, K:K + T])
    env.forward_train()


def test_the_term_alone_is_one_minus_the_mean_ssim_of_the_prediction(tmp_path):
    env = _env(tmp_path, 'ssim', alpha=0.0, beta=0.0, ssim_weight=1.0)
    _forward(env)
    env.optimize_parameters()
    pred = env.gen_output['pred'].detach().numpy()
    want = ref.ssim_loss_ref(pred, _CLIPS[:, K:K + T].numpy())
    assert 0.0 < want['loss'] < 2.0
    assert abs(float(env.loss_G.item()) - want['loss']) <= 1.2e-7          # the fp32 scalar: one rounding of a value below 2
    errs = env.get_current_errors()
    assert errs['G_ssim'] == float(env.ssim.item()) and abs(errs['G_ssim'] - want['loss']) <= 1.2e-7
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in env.generator.parameters() if p.requires_grad)
    assert any(float(p.grad.abs().max()) > 0 for p in env.generator.parameters())


def test_the_default_weight_changes_no_key_and_builds_no_module(tmp_path):
    env = _env(tmp_path, 'plain')
    _forward(env)
    env.optimize_parameters()
    assert sorted(env.get_current_errors()) == ['D_fake', 'D_real', 'G_GAN', 'G_Lp', 'G_gdl', 'G_loss']
    assert env.loss_ssim is None and not hasattr(env, 'ssim')
    state = env.get_current_state_dict(1, 0, 0)
    assert sorted(state) == ['discriminator', 'generator', 'optimizer_D', 'optimizer_G', 'sum_avg_psnr_err', 'sum_avg_ssim_err', 'updates']
    with_term = _env(tmp_path, 'with', ssim_weight=0.5)
    assert sorted(with_term.get_current_state_dict(1, 0, 0)) == sorted(state)
    assert list(with_term.generator.state_dict()) == list(env.generator.state_dict())
