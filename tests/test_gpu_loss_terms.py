"""The table of loss terms on the GPU, where the fused kernels supply the values and the separable convolution exists: one eager update
of the tiny real TAI model (three predictions) and of MC-Net (one), every term on, with both kinds of image loss -- loss_G's bits are the
written-out fold's, the tensors with history an update leaves behind are step outputs, and the printed keys are the listed ones
(loss_kit.check_fold; test_loss_terms_cpu.py runs every combination of terms on the torch paths)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_kit as kit  # noqa: E402

import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import losses, synthetic  # noqa: E402
from video_frame_inpainting_amd.environments import MCNetTrainingEnvironment, TAITrainingEnvironment, create_training_environment  # noqa: E402

pytestmark = pytest.mark.gpu
K, T, F = kit.K, kit.T, kit.F


@pytest.mark.parametrize('image_loss', ['l2', 'charbonnier'])
@pytest.mark.parametrize('model', ['SPEC', 'MCNET'])
def test_loss_G_is_the_written_out_fold_with_every_term_on(tmp_path, model, image_loss):
    torch.manual_seed(0)
    np.random.seed(0)
    settings = losses.LossSettings(image_loss=image_loss, lap_levels=4, **kit.TERM_WEIGHTS)
    env = create_training_environment(vfi.create_model(getattr(kit, model)), 1, str(tmp_path), 'terms', K, T, F, [kit.SIZE, kit.SIZE], 1.0,
                                      0.02, 1e-4, 0.5, 8, 3, 3, [0, 0], device=kit.DEV, losses=settings)
    three = model == 'SPEC'
    assert type(env) is (TAITrainingEnvironment if three else MCNetTrainingEnvironment)
    clips = torch.from_numpy(synthetic.make_clips(2, K + T + F, 1, kit.SIZE, kit.SIZE, 77))
    env.K, env.T, env.F = K, T, F
    env.train()
    env.train_step(clips[:, :K], clips[:, K + T:], clips[:, K:K + T])
    torch.cuda.synchronize()
    kit.check_fold(env, image_loss, tuple(kit.TERM_WEIGHTS), three)
