"""TAI_color at the shapes the reference publishes its colour numbers at (240 x 320, K = F = 4, T = 3: the UCF-101 / HMDB-51 test
argument files) and trains at (160 x 208, --sample_KTF): the kernel network's bottom planes are 15 x 20 and 10 x 13 there, the
weight gradients run on rows of 20-104 pixels and the discriminator's last layer sees a 10 x 13 space-to-depth plane.  Every
convolution of those shapes runs in-tree (csrc/wino_conv.hip.inc EPI 3, csrc/wino_wrw.hip.inc WRW_RAGGED)."""
import os

import numpy as np
import pytest
import torch

import video_frame_inpainting_amd as vfi
from video_frame_inpainting_amd import metrics, synthetic
from video_frame_inpainting_amd.graph import GraphedForward
from oracle import tai_oracle, train_oracle

import kink_sides  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KEYS = ('pred', 'pred_forward', 'pred_backward', 'interp_net_outputs_1', 'interp_net_outputs_2')
REL_TOL = 1e-4      # per output key: max |gpu - oracle| <= REL_TOL * max |oracle| (the bound of tests/test_gpu_model.py)
# the training step's settings and bounds of tests/test_gpu_training.py: options.py defaults, loss terms relative, generator gradients
# relative to each parameter's largest, discriminator gradients with the oracle differentiating on the product's side of every kink
ALPHA, BETA, IP, DISC_T = 1.0, 0.02, 3, 3
LOSS_RTOL, GRAD_RTOL, D_GRAD_RTOL = 2e-4, 5e-3, 2e-5
GRAD_KEYS = ('generator.motion_enc.dyn_conv1.0.weight', 'generator.motion_enc.dyn_conv3.1.weight',
             'generator.conv_lstm_cell.conv.weight', 'generator.conv_lstm_cell.conv.bias',
             'generator.content_enc.cont_conv1.0.weight',          # the 3 -> 64 layer at full resolution
             'generator.content_enc.cont_conv2.3.weight', 'generator.content_enc.cont_conv3.5.weight',
             'generator.dec_cnn.dec1.2.weight',                    # the 64 -> 3 (transposed) layer at full resolution
             'merge_residual2.res.0.weight', 'kernelnet.moduleConv.0.0.weight', 'kernelnet.moduleDeconv.0.0.weight',
             'kernelnet.moduleVertical1.7.weight', 'kernelnet.moduleHorizontal2.7.bias')


@pytest.fixture(autouse=True)
def _fp32_convs():
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False


def _assert_matches_oracle(out, ref, GT, name):
    """Each key within REL_TOL of the oracle relative to its own maximum; PSNR / SSIM against ground truth agree with the oracle's to
    0.01 dB / 1e-4."""
    for k in KEYS:
        scale = float(ref[k].abs().max())
        assert scale > 0.05, (name, k, scale)
        err = float((out[k].cpu() - ref[k]).abs().max())
        assert err <= REL_TOL * scale, (name, k, err, scale)
    pred_gpu, pred_cpu = out['pred'].cpu().numpy(), ref['pred'].numpy()
    assert len(np.unique(metrics.to_uint8(pred_gpu))) > 50, name
    p_gpu, s_gpu, _ = metrics.compute_errors(pred_gpu, GT.numpy())
    p_cpu, s_cpu, _ = metrics.compute_errors(pred_cpu, GT.numpy())
    assert np.max(np.abs(p_gpu - p_cpu)) <= 0.01, (name, p_gpu, p_cpu)
    assert np.max(np.abs(s_gpu - s_cpu)) <= 1e-4, (name, s_gpu, s_cpu)


class _OddPlaneRoutes(object):
    """Counts the convolutions on planes with an odd side that _wino_ok hands to the Winograd kernel (on top of DispatchAt)."""

    def __init__(self, monkeypatch):
        from video_frame_inpainting_amd import conv_ops
        self.taken = set()
        ok = conv_ops._wino_ok

        def wino_ok(N, Ci, Co, H, W, *a, **k):
            r = ok(N, Ci, Co, H, W, *a, **k)
            if r and (H % 2 or W % 2):
                self.taken.add((Ci, Co, H, W))
            return r
        monkeypatch.setattr(conv_ops, '_wino_ok', wino_ok)


def test_tai_color_at_240x320_matches_cpu_oracle(monkeypatch):
    """Full-width create_model('TAI_color') at 240 x 320, K = F = 4, T = 3 on one seeded clip: eager, hipGraph replay, and at the
    dispatch of a 16-clip batch (the published batch) with Winograd tile 4 and 2 -- there no ATen convolution is left and the
    15 x 20 layers run the odd-plane kernel."""
    from conftest import DispatchAt, miopen_convolutions
    from video_frame_inpainting_amd import conv_ops
    m = synthetic.seeded_init(vfi.create_model('TAI_color'), 0)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    clips = synthetic.make_clips(1, 11, 3, 240, 320, synthetic.SEEDS['cfg4'])
    P, GT, Fo = (torch.from_numpy(x) for x in synthetic.split_clip(clips, 4, 3, 4))
    with torch.no_grad():
        ref = tai_oracle.tai_forward(sd, 3, 4, 51, 3, P, Fo)
        m.to(DEV).eval()
        _assert_matches_oracle(m(3, P.to(DEV), Fo.to(DEV)), ref, GT, 'TAI_color 240x320, eager')
        g = GraphedForward(m, 3, P.to(DEV), Fo.to(DEV))
        _assert_matches_oracle(g(), ref, GT, 'TAI_color 240x320, hipGraph replay')
        del g
        with monkeypatch.context() as mp:
            DispatchAt(mp, 16)
            odd = _OddPlaneRoutes(mp)
            for tile in (4, 2):
                prev = conv_ops.set_winograd_tile(tile)
                try:
                    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU], record_shapes=True) as prof:
                        out = m(3, P.to(DEV), Fo.to(DEV))
                finally:
                    conv_ops.set_winograd_tile(prev)
                _assert_matches_oracle(out, ref, GT, 'TAI_color 240x320, dispatch of 16 clips, Winograd tile %d' % tile)
                assert not miopen_convolutions(prof), miopen_convolutions(prof)[:4]
            assert any(H == 15 and W == 20 for (_, _, H, W) in odd.taken), odd.taken


def _color_env(tmp_path, K, T, F, H, W):
    from video_frame_inpainting_amd.environments import TAITrainingEnvironment
    model = vfi.TAIFillInModel(64, 3, 3, 51, num_block=4)            # TAI_color's generator (create_model.py)
    env = TAITrainingEnvironment(model, str(tmp_path), 'pub', [H, W], 3, ALPHA, BETA, 1e-4, 0.5, 64, IP, DISC_T, K, T, F, [0, 0],
                                 device=DEV)
    synthetic.seeded_init(env.generator, 21)
    synthetic.seeded_init(env.discriminator, 22)
    g = torch.Generator().manual_seed(23)
    u = {}
    for name, mod in env.discriminator.named_modules():
        if hasattr(mod, 'Ip'):
            u[name] = torch.randn(1, mod.weight.size(0), generator=g)
            mod.u = u[name].to(DEV)
    return env, u


def _update(env, P, Fo, GT, K, T, F):
    """One G + D update's gradients (the reference's step order, environments.py:348-355, without the optimiser steps)."""
    env.set_train_inputs(P, Fo, GT)
    env.K, env.T, env.F = K, T, F
    env.train()
    env.forward_train()
    env.optimizer_G.zero_grad()
    env.compute_loss_G()
    env.loss_G.backward()
    gg = {k: p.grad.detach().clone() for k, p in env.generator.named_parameters() if p.grad is not None}
    env.optimizer_D.zero_grad()
    env.compute_loss_D()
    env.loss_D.backward()
    dg = {k: p.grad.detach().clone() for k, p in env.discriminator.named_parameters() if p.grad is not None}
    return gg, dg


def test_training_update_at_160x208_matches_the_oracle_runs_in_tree_and_reproduces(tmp_path, monkeypatch):
    """One full-width G + D step of TAI_color's generator (c_dim 3, num_block 4) at 160 x 208, K = F = 4, T = 3, B = 2, routed as a
    32-clip batch (DispatchAt(16): 16 x these 2 clips): every loss term and the gradients against the CPU oracle's training legs
    (train_oracle.generator_leg / discriminator_leg, the bounds of tests/test_gpu_training.py); no ATen convolution in the update -- the
    10 x 13 kernel-network bottom, the weight gradients on rows of 26-104 pixels, the discriminator's 10 x 13 space-to-depth layer and the
    two 3-channel layers at full resolution all run in-tree -- and a second identical step gives the same losses and the same bits in
    every discriminator gradient and every gradient of the kernel network and the merge layers (whose 15 x 20 / 10 x 13 planes are the
    odd-plane route).  Before the oracle's D half takes the product's LeakyReLU sides, all 4 layers of all 3 discriminator evaluations are
    held to the float64 layer on their own operands (kink_sides.check_layer) at the first, the middle and the last of the 9 windows -- the
    images at both ends of the batch-stacked planes and one inside; the other 6 windows' layer outputs are the only thing left out.  The MC-Net generator's gradients of two identical updates differ in the last bits (~2e-7 of their maximum) at the
    parent commit's 128 x 128 gray update as well, where no shape of this route occurs: they are held to 1e-5 here."""
    from conftest import DispatchAt, miopen_convolutions
    K, T, F, H, W, B = 4, 3, 4, 160, 208, 2
    env, u = _color_env(tmp_path, K, T, F, H, W)
    gen_sd = {k: v.detach().cpu().clone() for k, v in env.generator.state_dict().items()}
    disc_sd = {k: v.detach().cpu().clone() for k, v in env.discriminator.state_dict().items()}
    disc_state = {k: v.detach().clone() for k, v in env.discriminator.state_dict().items()}
    clips = torch.from_numpy(synthetic.make_clips(B, K + T + F, 3, H, W, synthetic.SEEDS['cfg3']))
    P, GT, Fo = synthetic.split_clip(clips, K, T, F)
    DispatchAt(monkeypatch, 16)
    odd = _OddPlaneRoutes(monkeypatch)
    sides = kink_sides.DiscriminatorSpy(monkeypatch, kink_sides.ends_and_middle)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU], record_shapes=True) as prof:
        g1, d1 = _update(env, P, Fo, GT, K, T, F)
    convs = miopen_convolutions(prof)
    assert not convs, sorted(set((c[0], tuple(c[1][0])) for c in convs))
    assert any(H2 == 10 and W2 == 13 for (_, _, H2, W2) in odd.taken), odd.taken
    errs = env.get_current_errors()
    assert len(sides.layers) == 12, len(sides.layers)           # D(fake) in the G loss, D(fake.detach()), D(real): 4 layers each
    # every layer call of the product against the float64 layer on its own operands, BEFORE its kink sides go anywhere
    layer_results = kink_sides.check_discriminator_calls(sides)

    # the CPU oracle
    keys = [k for k in GRAD_KEYS if k in gen_sd]
    assert len(keys) == len(GRAD_KEYS), sorted(set(GRAD_KEYS) - set(keys))
    disc = train_oracle.DiscriminatorState(disc_sd, u, IP, DISC_T)
    terms, g_ref, _, fake = train_oracle.generator_leg(gen_sd, disc, 3, 4, 51, P, GT, Fo, ALPHA, BETA, keys)
    disc_own = train_oracle.DiscriminatorState(disc.sd, disc.u, IP, DISC_T)
    d_terms, d_ref = train_oracle.discriminator_leg(disc, fake, P, GT, Fo, sides.masks_of_call(1, B), sides.masks_of_call(2, B))
    with kink_sides.OracleSides() as own:               # the sides the oracle's own rounding picks: counted against the imposed ones, not bounded
        train_oracle.discriminator_leg(disc_own, fake, P, GT, Fo)
    losses = {k: float(v) for k, v in list(terms.items()) + list(d_terms.items())}
    print('\n'.join(['== TAI_color gf_dim 64 B %d K %d T %d F %d %dx%d, 32-clip dispatch' % (B, K, T, F, H, W)] +
                    kink_sides.report_lines(sides, layer_results, own.differences(sides, B))))
    report, worst = [], {'G': 0.0, 'D': 0.0}
    for k in sorted(losses):
        rel = abs(errs[k] - losses[k]) / max(abs(losses[k]), 1e-12)
        report.append('%-16s gpu %.7g oracle %.7g rel %.2e' % (k, errs[k], losses[k], rel))
        assert rel <= LOSS_RTOL, report[-1]
        assert abs(losses[k]) > 1e-4, report[-1]
    for k in keys:
        scale = float(g_ref[k].abs().max())
        err = float((g1[k].cpu() - g_ref[k]).abs().max())
        report.append('%-44s max|g| %.3e  err/max %.2e' % (k, scale, err / max(scale, 1e-30)))
        assert scale > 1e-7, report[-1]
        worst['G'] = max(worst['G'], err / scale)
        assert err <= GRAD_RTOL * scale, report[-1]
    for k in sorted(d_ref):
        scale = float(d_ref[k].abs().max())
        err = float((d1[k].cpu() - d_ref[k]).abs().max())
        report.append('%-44s max|g| %.3e  err/max %.2e' % ('D.' + k, scale, err / max(scale, 1e-30)))
        assert scale > 1e-7, report[-1]
        worst['D'] = max(worst['D'], err / scale)
        assert err <= D_GRAD_RTOL * scale, report[-1]
    report.append('worst err/max: generator %.2e (bound %.0e)  discriminator %.2e (bound %.0e)' % (worst['G'], GRAD_RTOL, worst['D'], D_GRAD_RTOL))
    print('\n'.join(report))

    # the spectral-norm state moved during the step: put it back, then the same step once more -- the same bits
    env.discriminator.load_state_dict(disc_state)
    for name, mod in env.discriminator.named_modules():
        if name in u:
            mod.u = u[name].to(DEV)
    g2, d2 = _update(env, P, Fo, GT, K, T, F)
    assert sorted(g1) == sorted(g2) and sorted(d1) == sorted(d2)
    errs2 = env.get_current_errors()
    assert all(errs[k] == errs2[k] for k in errs), [(k, errs[k], errs2[k]) for k in errs if errs[k] != errs2[k]]
    assert all(torch.equal(d1[k], d2[k]) for k in d1), [k for k in d1 if not torch.equal(d1[k], d2[k])][:5]
    outside = [k for k in g1 if not k.startswith('generator.')]
    assert len(outside) > 30 and any(k.startswith('kernelnet.moduleDeconv') for k in outside)
    assert all(torch.equal(g1[k], g2[k]) for k in outside), [k for k in outside if not torch.equal(g1[k], g2[k])][:5]
    rel = {k: float((g1[k] - g2[k]).abs().max()) / max(float(g1[k].abs().max()), 1e-30) for k in g1 if k.startswith('generator.')}
    assert max(rel.values()) <= 1e-5, sorted(rel.items(), key=lambda kv: -kv[1])[:5]


def test_predict_cli_at_the_published_flags(tmp_path, monkeypatch):
    """predict.py with the reference's colour flags (TAI_color, --c_dim 3, --image_size 240 320, K = F = 4, T = 3) writes the
    reference's PNG set at 240 x 320."""
    import predict
    monkeypatch.chdir(tmp_path)
    predict.main(['--name', 'pub', '--model_key', 'TAI_color', '--c_dim', '3', '--image_size', '240', '320', '--K', '4', '--F', '4',
                  '--T', '3', '--batch_size', '2', '--synthetic', '2', '--random_init', '--checkpoints_dir', str(tmp_path / 'ckpt'),
                  '--qual_result_root', str(tmp_path / 'res'), '--intermediate_preds'])
    files = sorted(os.listdir(tmp_path / 'res' / 'synthetic_000001'))
    want = (['gt_preceding_%04d.png' % i for i in range(4)] + ['gt_middle_%04d.png' % i for i in (4, 5, 6)] +
            ['gt_following_%04d.png' % i for i in (7, 8, 9, 10)] +
            ['%s_%04d.png' % (p, i) for p in ('pred_middle', 'pred_middle_forward', 'pred_middle_backward',
                                                'interp_net_outputs_1', 'interp_net_outputs_2') for i in (4, 5, 6)])
    assert files == sorted(want)
    from PIL import Image
    im = np.asarray(Image.open(tmp_path / 'res' / 'synthetic_000001' / 'pred_middle_0004.png'))
    assert im.shape == (240, 320, 3) and im.dtype == np.uint8
