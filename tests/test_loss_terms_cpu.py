"""The table of loss terms the training environments build from a losses.LossSettings (environments.L2GDLDiscTrainingEnvironment), without
a GPU: for one and for three predictions, every on/off combination of the four weighted terms and both kinds of image loss, loss_G is the
fold loss_kit.check_fold writes out, every tensor with history an update leaves behind is a step output, the printed keys are the listed
ones, each module is called as often as its kind says, and a term that is off builds nothing."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_kit as kit  # noqa: E402

import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import losses, synthetic  # noqa: E402
from video_frame_inpainting_amd.ablations import BidirectionalSimpleAverageFillInModel  # noqa: E402
from video_frame_inpainting_amd.environments import MCNetTrainingEnvironment, TAITrainingEnvironment, create_training_environment  # noqa: E402

K, T, F = kit.K, kit.T, kit.F
_OPT_IN = (losses.SSIMLoss, losses.ImageLoss, losses.LapLoss, losses.TemporalLoss, losses.CensusLoss)
_COMBINATIONS = [on for n in range(len(kit.TERM_WEIGHTS) + 1) for on in itertools.combinations(kit.TERM_WEIGHTS, n)]


def _env(root, model, image_loss, on):
    torch.manual_seed(0)
    np.random.seed(0)
    net = vfi.MCNetFillInModel(4, 1, 3) if model == 'mcnet' else BidirectionalSimpleAverageFillInModel(4, 1, 3)
    settings = losses.LossSettings(image_loss=image_loss, lap_levels=4, **{k: kit.TERM_WEIGHTS[k] for k in on})
    return create_training_environment(net, 1, str(root), 'terms', K, T, F, [32, 32], 1.0, 0.02, 1e-3, 0.5, 4, 2, 3, [0, 0], device='cpu',
                                       losses=settings)


def _reachable(obj, seen):
    """Everything that hangs on ``obj``: attributes, the items of containers, what functions have closed over or are bound to."""
    if id(obj) in seen or isinstance(obj, (str, bytes, int, float, torch.Tensor, np.ndarray, type(None))):
        return
    seen[id(obj)] = obj
    if isinstance(obj, dict):
        children = list(obj.values())
    elif isinstance(obj, (list, tuple, set)):
        children = list(obj)
    else:
        children = [c.cell_contents for c in getattr(obj, '__closure__', None) or ()] + [getattr(obj, '__self__', None)]
        children += list(vars(obj).values()) if hasattr(obj, '__dict__') and not isinstance(obj, torch.nn.Module) else []
    for c in children:
        _reachable(c, seen)


@pytest.mark.parametrize('image_loss', ['l2', 'charbonnier'])
@pytest.mark.parametrize('model', ['mcnet', 'bidirectional'])
def test_loss_G_is_the_written_out_fold_for_every_combination_of_terms(tmp_path, model, image_loss):
    """The separable convolution exists on the GPU only, so the three-prediction environment is driven here by the bidirectional average
    model (the same TAITrainingEnvironment, the same three outputs) and the one-prediction environment by MC-Net."""
    three = model == 'bidirectional'
    for i, on in enumerate(_COMBINATIONS):
        env = _env(tmp_path, model, image_loss, on)
        assert type(env) is (TAITrainingEnvironment if three else MCNetTrainingEnvironment)
        modules = {'image_loss': env.loss_image, 'ssim_weight': env.loss_ssim, 'lap_weight': env.loss_lap,
                   'temporal_weight': env.loss_temporal, 'census_weight': env.loss_census}
        assert all((m is not None) == (k in on or (k == 'image_loss' and image_loss != 'l2')) for k, m in modules.items())
        seen = {}
        _reachable(env, seen)
        hanging = [m for m in seen.values() if isinstance(m, _OPT_IN)]
        assert sorted(map(id, hanging)) == sorted(id(m) for m in modules.values() if m is not None)          # off: nothing is built
        calls = {k: 0 for k in list(modules) + ['discriminator']}

        def count(key):
            def hook(*_):
                calls[key] += 1
            return hook
        for key, m in list(modules.items()) + [('discriminator', env.discriminator)]:
            if m is not None:
                m.register_forward_hook(count(key))
        env.K, env.T, env.F = K, T, F
        env.train()
        clips = torch.from_numpy(synthetic.make_clips(2, K + T + F, 1, 32, 32, 77 + i))          # other values in every fold
        env.set_train_inputs(clips[:, :K], clips[:, K + T:], clips[:, K:K + T])
        env.forward_train()
        env._zero_grad(env.optimizer_G, env._reducer_G)
        env.compute_loss_G()
        # one frozen discriminator evaluation; one call for all predictions of image, temporal and census; one per prediction of ssim, lap
        n = 3 if three else 1
        want = {'discriminator': 1, 'image_loss': 1, 'temporal_weight': 1, 'census_weight': 1, 'ssim_weight': n, 'lap_weight': n}
        assert calls == {k: (want[k] if k == 'discriminator' or modules[k] is not None else 0) for k in calls}
        env.optimize_parameters()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in env.generator.parameters() if p.requires_grad)
        kit.check_fold(env, image_loss, on, three)
