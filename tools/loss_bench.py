#!/usr/bin/env python3
"""The fused losses (tai_ssim_loss, tai_image_loss, tai_lap_loss, tai_temporal_loss, tai_census_loss behind losses.SSIMLoss, ImageLoss,
LapLoss, TemporalLoss, CensusLoss): the launch against the torch ops it replaces, and one eager TAI_gray update with and without the term.

  python tools/loss_bench.py --loss {ssim,image,lap,temporal,census} [--reps 30] [--updates 10] [--out profiles/<loss>_loss_bench.jsonl]
                             [--no-updates]

(a) launches   at the loss's two shapes (below), loss + gradient:
                 kernel   the entry through the C ABI, outputs and workspace made once (the launches only);
                 module   the module's forward + backward through autograd (what an update pays: allocations, fp32 scalars, grad * map);
                 torch    forward + backward of the torch ops named below on the same device;
               HIP events, median of --reps; the variants alternate in one process and the whole comparison is made three times:
               `ms` is the median of the three medians, `spread_ms` the largest distance between the three medians of any variant.
(b) updates    eager milliseconds per update of two TAI_gray training environments at 128 x 128, 32 clips, K = T = F = 5, one without
               and one with the term (below); legs alternate, three times, --updates each after a warm-up.
No threshold: the ratios and the milliseconds are reported as measured.  One JSON line per measurement, printed and appended to --out;
every loss keeps its metric names, record fields and file, so old and new lines compare.

ssim      train.py --ssim_weight.  (a) [160, 1, 128, 128] (TAI_gray, 32 clips x 5 frames) and [48, 3, 256, 256]; torch: the same
          definition composed from avg_pool2d in float64 (losses._ssim_planes, the module's host path).  (b) without the term and with
          --ssim_weight 0.2 (three SSIM terms per update).
image     train.py --image_loss.  (a) three predictions against one ground truth at [32, 5, 1, 128, 128] (TAI_gray, 32 clips) and
          [16, 3, 3, 256, 256], kind 0 (L2: the composition's own quantity); torch: today's composition for the same three predictions,
          _time_major_01 of each tensor, MSELoss, GDL (what L2GDLDiscTrainingEnvironment / TAITrainingEnvironment run).  The launch's
          bytes ((npred + 1) reads + npred writes of 4 bytes per element) over its time are given as a fraction of the HBM peak.
          (b) --image_loss l2 (the composition) and charbonnier (the launch).
lap       train.py --lap_weight.  (a) [160, 1, 128, 128] (the pyramid in LDS) and [48, 3, 256, 256] (the pyramid in the workspace),
          5 levels; torch: the same definition composed from torch ops in float64 (losses._lap_terms, the module's host path);
          `kernel_share_of_8TBps`: the algorithmic bytes (pred and gt read, grad written: 12 per pixel) over the kernel's time, as a
          share of the HBM peak.  (b) without the term and with --lap_weight 0.5 (three pyramid terms per update).
temporal  train.py --temporal_weight.  (a) three predictions against one ground truth at [32, 5, 1, 128, 128] (``pred`` stored
          time-major, as tai.py returns it, the other two and the ground truth [B, T, ...]) and [16, 3, 3, 256, 256], kind 2
          (Charbonnier, the default of the flag); torch: the same definition in torch ops (losses._temporal_terms, the module's own
          path for tensors the kernel does not take), once per prediction; bytes as for image.  (b) without the term and with
          --temporal_weight 0.5; the difference is given next to the leg-to-leg spread, and next to what the module alone takes at the
          update's shape.
census    train.py --census_weight.  (a) the temporal loss's two shapes and layouts; torch: the same definition in torch ops in float64
          (losses._census_terms, the module's own path for tensors the kernel does not take), once per prediction.  The kernel is bound
          by the vector ALU (48 offsets x (2 square roots + 5 divisions) per pixel and prediction), so next to the bytes its rate is given
          in (pixel, offset, prediction) terms per second.  (b) without the term and with --census_weight 0.5, as for temporal."""
import argparse
import ctypes
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import _native, losses, synthetic  # noqa: E402
from video_frame_inpainting_amd.environments import L2GDLDiscTrainingEnvironment, create_training_environment  # noqa: E402
from grad_guard_bench import event_ms  # noqa: E402

NPRED = 3
LEVELS = 5
KIND, EPS = 2, 1e-3                                              # the temporal loss's
HBM_PEAK_GBPS = 8000.0
K = T = F = 5
BATCH, SIZE = 32, 128
DEV = torch.device('cuda:0')
PLANE_SHAPES = (('TAI_gray 32 clips x 5', (160, 1, 128, 128)), ('color 256x256', (48, 3, 256, 256)))
CLIP_SHAPES = (('TAI_gray 32 clips x 5', (32, 5, 1, 128, 128)), ('color 256x256', (16, 3, 3, 256, 256)))


def one_pair(name, shape):
    """([pred], gt) [N, C, H, W] on the device."""
    N, C, H, W = shape
    clips = synthetic.make_clips(N, 2, C, H, W, 31)
    return [torch.from_numpy(np.ascontiguousarray(clips[:, 0])).to(DEV)], torch.from_numpy(np.ascontiguousarray(clips[:, 1])).to(DEV)


def three_against_one(name, shape):
    """(three preds, gt) [B, T, C, H, W] on the device; the first stored time-major (a transposed view, as tai.py returns ``pred``)
    where the shape's name says so."""
    B, Tn, C, H, W = shape
    clips = synthetic.make_clips(B, Tn * (NPRED + 1), C, H, W, 31).reshape(B, NPRED + 1, Tn, C, H, W)
    preds = [torch.from_numpy(np.ascontiguousarray(clips[:, 1 + i])).to(DEV) for i in range(NPRED)]
    if 'time-major' in name:
        preds[0] = preds[0].transpose(0, 1).contiguous().transpose(0, 1)
    return preds, torch.from_numpy(np.ascontiguousarray(clips[:, 0])).to(DEV)


def raw_launcher(entry, query, n_detail, n_totals, preds, args):
    """The entry through the C ABI with everything made once -> (callable, totals float64, gradient maps, workspace bytes).
    ``args(preds, detail, totals, maps, workspace)`` -> the entry's arguments before the stream, pointers as integers."""
    L = _native.lib()
    nbytes = getattr(L, entry + '_workspace_bytes')(*query)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    out = torch.empty(n_detail + n_totals, dtype=torch.float64, device=DEV)
    grads = [torch.empty_strided(p.shape, p.stride(), dtype=torch.float32, device=DEV) for p in preds]
    totals = out[n_detail:]
    fixed = args([p.data_ptr() for p in preds], out.data_ptr(), totals.data_ptr(), [x.data_ptr() for x in grads], ws.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    call = getattr(L, entry)
    return (lambda: _native.check(call(*fixed, stream), entry)), totals, grads, nbytes


def table(pointers):
    return (ctypes.c_void_p * len(pointers))(*pointers)


def pixel_rates(pixels, kernel_ms, share):
    rates = {'kernel_Gpixel_per_s': round(pixels / kernel_ms / 1e6, 2),
             'kernel_min_traffic_GBps': round(12 * pixels / kernel_ms / 1e6, 1)}          # reads pred and gt, writes grad: 12 bytes per pixel
    if share:
        rates['kernel_share_of_8TBps'] = round(12 * pixels / kernel_ms / 1e6 / 8000.0, 4)
    return rates


def byte_rates(g, kernel_ms):
    elements = g.numel()
    nbytes = (2 * NPRED + 1) * 4 * elements
    return {'launch_bytes': nbytes, 'kernel_GBps': round(nbytes / kernel_ms / 1e6, 1),
            'kernel_fraction_of_hbm_peak': round(nbytes / kernel_ms / 1e6 / HBM_PEAK_GBPS, 4), 'hbm_peak_GBps': HBM_PEAK_GBPS}


def census_rates(g, kernel_ms):
    terms = g.numel() // g.shape[2] * 48 * NPRED                  # every pixel of the plane looks at (up to) 48 neighbours, per prediction
    return {**byte_rates(g, kernel_ms), 'kernel_Gterms_per_s': round(terms / kernel_ms / 1e6, 2)}


def planes_head(name, shape, reps, **first):
    N, C, H, W = shape
    return dict(first, shape=name, N=N, C=C, H=H, W=W, reps=reps)


def ssim_kernel(preds, g):
    N, C, H, W = g.shape
    return raw_launcher('tai_ssim_loss', (N, C, H, W), N * C, 2, preds,
                        lambda p, detail, totals, m, ws: (p[0], g.data_ptr(), detail, totals, m[0], ws, N, C, H, W))


def image_kernel(preds, g):
    H, W = g.shape[-2:]
    P, n = g.numel() // (H * W), len(preds)
    return raw_launcher('tai_image_loss', (n, P, H, W), n * P * 2, n * 3, preds,
                        lambda p, detail, totals, m, ws: (table(p), n, g.data_ptr(), 0, 1e-3, detail, totals, table(m), ws, P, H, W))


def lap_kernel(preds, g):
    N, C, H, W = g.shape
    return raw_launcher('tai_lap_loss', (N * C, H, W, LEVELS), N * C * LEVELS, LEVELS + 1, preds,
                        lambda p, detail, totals, m, ws: (p[0], g.data_ptr(), LEVELS, detail, totals, m[0], ws, N * C, H, W))


def temporal_kernel(preds, g):
    B, Tn, C, H, W = g.shape
    n, S = len(preds), B * C
    strides = (ctypes.c_longlong * (2 * n + 2))(*[v for t in list(preds) + [g] for v in losses._block_strides(t)])
    return raw_launcher('tai_temporal_loss', (n, B, Tn, C, H, W), n * S * (Tn + 1), n * (Tn + 2), preds,
                        lambda p, detail, totals, m, ws: (table(p), n, g.data_ptr(), strides, KIND, EPS, detail, totals, table(m), ws,
                                                          B, Tn, C, H, W))


def census_kernel(preds, g):
    B, Tn, C, H, W = g.shape
    n = len(preds)
    strides = (ctypes.c_longlong * (2 * n + 2))(*[v for t in list(preds) + [g] for v in losses._block_strides(t)])
    return raw_launcher('tai_census_loss', (n, B, Tn, C, H, W), n * B * Tn, n, preds,
                        lambda p, detail, totals, m, ws: (table(p), n, g.data_ptr(), strides, detail, totals, table(m), ws, B, Tn, C, H, W))


def composition(pt, g):
    """MSELoss + GDL of three predictions as the environments run them."""
    mse, gdl = torch.nn.MSELoss(), losses.GDL()
    time_major = L2GDLDiscTrainingEnvironment._time_major_01
    gt = time_major(g)                                   # as the environments do: gt's copy is made once per pass of compute_loss_G,
    x = time_major(pt[0])                                # for pred ...
    total = mse(x, gt) + gdl(x, gt)
    gt = time_major(g)                                   # ... and for pred_forward and pred_backward
    xf, xb = time_major(pt[1]), time_major(pt[2])
    return total + (mse(xf, gt) + mse(xb, gt) + gdl(xf, gt) + gdl(xb, gt))


def sum_of_three(module, pm, g):
    a, b, c = module(tuple(pm), g)
    return a + b + c


# Per loss: the shapes; inputs(name, shape) -> (preds, gt); the raw-ABI launcher; the module, how it is called and the torch ops, each ->
# the tensor to call backward on; head(name, shape, reps, preds, gt) -> the record's fields up to `reps`; rates
# (gt, kernel ms); which variant the record's verdict compares with torch; value(totals) -> the loss field(s); more(grads, torch grads) -> further fields.
# For the update legs: the two environments {leg: (name, keyword arguments)}, the record's settings, the names of its difference and
# verdict fields (``two_sided``: the verdict takes the difference's size) and the errors it lists.
LOSSES = {
    'ssim': SimpleNamespace(
        shapes=PLANE_SHAPES, inputs=one_pair, kernel=ssim_kernel, module=losses.SSIMLoss, call=lambda m, pm, g: m(pm[0], g),
        torch=lambda pt, g: (1.0 - losses._ssim_planes(pt[0], g).mean(dim=(1, 2, 3)).mean()).to(torch.float32),
        head=lambda name, shape, reps, preds, g: planes_head(name, shape, reps),
        rates=lambda g, ms: pixel_rates(g.numel(), ms, False), verdict='kernel', value=lambda totals: {'loss': float(totals[-1])},
        more=lambda grads, ref: {},
        envs={'plain': ('slb_plain', {}), 'ssim': ('slb_ssim', {'ssim_weight': 0.2})}, settings={'ssim_weight': 0.2},
        difference='added_ms_per_update', update_verdict='added_is_more_than_the_spread', two_sided=False,
        errors=('G_ssim', ('G_ssim', 'G_ssim_forward', 'G_ssim_backward'))),
    'image': SimpleNamespace(
        shapes=CLIP_SHAPES, inputs=three_against_one, kernel=image_kernel, module=lambda: losses.ImageLoss('l2'), call=sum_of_three,
        torch=composition,
        head=lambda name, shape, reps, preds, g: {'shape': name, 'dims': list(shape), 'npred': NPRED, 'kind': 'l2', 'reps': reps},
        rates=byte_rates, verdict='module', value=lambda totals: {'losses': [float(x) for x in totals.view(NPRED, 3)[:, 2]]},
        more=lambda grads, ref: {},
        envs={'l2': ('ilb_l2', {'image_loss': 'l2'}), 'charbonnier': ('ilb_charbonnier', {'image_loss': 'charbonnier'})}, settings={},
        difference='charbonnier_minus_l2_ms', update_verdict='difference_is_more_than_the_spread', two_sided=True,
        errors=('G_Lp_G_gdl', ('G_Lp', 'G_gdl', 'G_Lp_forward', 'G_gdl_forward', 'G_Lp_backward', 'G_gdl_backward'))),
    'lap': SimpleNamespace(
        shapes=PLANE_SHAPES, inputs=one_pair, kernel=lap_kernel, module=lambda: losses.LapLoss(LEVELS), call=lambda m, pm, g: m(pm[0], g),
        torch=lambda pt, g: losses._lap_terms(pt[0], g, LEVELS)[0].to(torch.float32),
        head=lambda name, shape, reps, preds, g: planes_head(name, shape, reps, levels=LEVELS),
        rates=lambda g, ms: pixel_rates(g.numel(), ms, True), verdict='kernel', value=lambda totals: {'loss': float(totals[-1])},
        # (both exact: no word should differ)
        more=lambda grads, ref: {'grad_words_differing_from_torch_autograd': int((grads[0].view(torch.int32) != ref[0].view(torch.int32)).sum())},
        envs={'plain': ('llb_plain', {}), 'lap': ('llb_lap', {'lap_weight': 0.5, 'lap_levels': LEVELS})},
        settings={'lap_weight': 0.5, 'levels': LEVELS},
        difference='added_ms_per_update', update_verdict='added_is_more_than_the_spread', two_sided=False,
        errors=('G_lap', ('G_lap', 'G_lap_forward', 'G_lap_backward'))),
    'temporal': SimpleNamespace(
        shapes=(('TAI_gray 32 clips x 5, pred time-major', CLIP_SHAPES[0][1]), CLIP_SHAPES[1]), inputs=three_against_one,
        kernel=temporal_kernel, module=lambda: losses.TemporalLoss(losses.IMAGE_LOSS_KINDS[KIND], EPS), call=sum_of_three,
        torch=lambda pt, g: sum(losses._temporal_terms(p, g, KIND, EPS)[0] for p in pt),
        head=lambda name, shape, reps, preds, g: {'shape': name, 'dims': list(shape), 'npred': NPRED, 'kind': 'charbonnier', 'reps': reps,
                                                  'strides': [list(losses._block_strides(t)) for t in preds + [g]]},
        rates=byte_rates, verdict='module', value=lambda totals: {'losses': [float(x) for x in totals.view(NPRED, -1)[:, -1]]},
        more=lambda grads, ref: {},
        envs={'plain': ('tlb_plain', {}), 'temporal': ('tlb_temporal', {'temporal_weight': 0.5})},
        settings={'temporal_weight': 0.5, 'kind': 'charbonnier'},
        difference='temporal_minus_plain_ms', update_verdict='difference_is_more_than_the_spread', two_sided=True,
        errors=('G_temporal', ('G_temporal', 'G_temporal_forward', 'G_temporal_backward'))),
    'census': SimpleNamespace(
        shapes=(('TAI_gray 32 clips x 5, pred time-major', CLIP_SHAPES[0][1]), CLIP_SHAPES[1]), inputs=three_against_one,
        kernel=census_kernel, module=losses.CensusLoss, call=sum_of_three,
        torch=lambda pt, g: sum(losses._census_terms(p, g)[0] for p in pt),
        head=lambda name, shape, reps, preds, g: {'shape': name, 'dims': list(shape), 'npred': NPRED, 'reps': reps,
                                                  'strides': [list(losses._block_strides(t)) for t in preds + [g]]},
        rates=census_rates, verdict='module', value=lambda totals: {'losses': [float(x) for x in totals]},
        more=lambda grads, ref: {},
        envs={'plain': ('clb_plain', {}), 'census': ('clb_census', {'census_weight': 0.5})},
        settings={'census_weight': 0.5},
        difference='census_minus_plain_ms', update_verdict='difference_is_more_than_the_spread', two_sided=True,
        errors=('G_census', ('G_census', 'G_census_forward', 'G_census_backward'))),
}


def alternate(runs, measure):
    """Every variant in turn, the whole round three times -> ({variant: its three results}, {variant: their median}, the largest distance
    between the three results of any variant)."""
    results = {k: [] for k in runs}
    for _ in range(3):
        for k, run in runs.items():
            results[k].append(measure(run))
    return results, {k: float(np.median(v)) for k, v in results.items()}, max(max(v) - min(v) for v in results.values())


def launch_lines(which, reps, out_path):
    loss = LOSSES[which]
    module_ms = {}
    for name, shape in loss.shapes:
        preds, g = loss.inputs(name, shape)
        kernel, totals, grads, ws_bytes = loss.kernel(preds, g)
        module = loss.module()
        pm = [p.detach().clone(memory_format=torch.preserve_format).requires_grad_() for p in preds]
        pt = [p.detach().clone(memory_format=torch.preserve_format).requires_grad_() for p in preds]
        assert [p.stride() for p in pm] == [p.stride() for p in preds]

        def run_module():
            for p in pm:
                p.grad = None
            loss.call(module, pm, g).backward()

        def run_torch():
            for p in pt:
                p.grad = None
            loss.torch(pt, g).backward()
        runs = {'kernel': kernel, 'module': run_module, 'torch': run_torch}
        meds, ms, spread = alternate(runs, lambda run: event_ms(run, reps))
        torch.cuda.synchronize()
        # the three compute one thing: the kernel's maps against autograd of the torch ops
        scale = max(float(p.grad.abs().max()) for p in pt)
        diff = max(float((x - p.grad).abs().max()) for x, p in zip(grads, pt))
        module_ms[tuple(shape)] = ms['module']
        emit({'metric': which + '_loss_launch', **loss.head(name, shape, reps, preds, g),
              'library_version': _native.lib().tai_sepconv_version(), 'workspace_bytes': ws_bytes,
              'ms_medians': {k: [round(x, 4) for x in v] for k, v in meds.items()}, 'ms': {k: round(v, 4) for k, v in ms.items()},
              'spread_ms': round(spread, 4), **loss.rates(g, ms['kernel']),
              'torch_over_kernel': round(ms['torch'] / ms['kernel'], 2), 'torch_over_module': round(ms['torch'] / ms['module'], 2),
              loss.verdict + '_faster_than_torch_by_more_than_the_spread': bool(ms['torch'] - ms[loss.verdict] > spread),
              **loss.value(totals), 'grad_max': scale, 'grad_max_diff_to_torch_autograd': diff, **loss.more(grads, [p.grad for p in pt])},
             out_path)
        del pm, pt, runs, kernel, grads, totals
        torch.cuda.empty_cache()
    return module_ms


def make_env(name, **kw):
    torch.manual_seed(0)
    env = create_training_environment(vfi.create_model('TAI_gray'), 1, os.path.join(ROOT, 'build', 'no_checkpoints'), name,
                                      K, T, F, [SIZE, SIZE], 1.0, 0.02, 1e-4, 0.5, 64, 3, 3, [0, 0], device=DEV, losses=losses.LossSettings(**kw))
    env.K, env.T, env.F = K, T, F
    env.train()
    return env


def update_ms(env, clips, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        c = clips[(i % 2) * BATCH:(i % 2 + 1) * BATCH]
        env.train_step(c[:, :K], c[:, K + T:], c[:, K:K + T])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def update_lines(which, updates, out_path, module_ms):
    loss = LOSSES[which]
    clips = torch.from_numpy(synthetic.make_clips(2 * BATCH, K + T + F, 1, SIZE, SIZE, 1002))
    envs = {leg: make_env(name, **kw) for leg, (name, kw) in loss.envs.items()}
    for env in envs.values():
        update_ms(env, clips, 3)                                 # MIOpen's searches, lazy allocations, Adam's state
    legs, ms, spread = alternate(envs, lambda env: update_ms(env, clips, updates))
    base, term = envs                                            # the leg without the term (or with the composition), the leg with it
    errs = envs[term].get_current_errors()
    added = ms[term] - ms[base]
    alone = module_ms.get((BATCH, T, 1, SIZE, SIZE))
    field, keys = loss.errors
    emit({'metric': which + '_loss_update', 'model': 'TAI_gray 128x128', 'batch': BATCH, 'KTF': [K, T, F], **loss.settings,
          'updates_per_leg': updates, 'ms_legs': {k: [round(x, 3) for x in v] for k, v in legs.items()},
          'ms': {k: round(v, 3) for k, v in ms.items()}, 'spread_ms': round(spread, 3),
          loss.difference: round(added, 3), 'ratio': round(ms[term] / ms[base], 4),
          loss.update_verdict: bool((abs(added) if loss.two_sided else added) > spread),
          **({'module_alone_ms_at_this_shape': None if alone is None else round(alone, 4)} if which in ('temporal', 'census') else {}),
          field: [round(errs[k], 5) for k in keys]}, out_path)


def emit(rec, out_path):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'a') as f:
            f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0], epilog=__doc__.split('\n\n', 2)[2],
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--loss', required=True, choices=sorted(LOSSES))
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--updates', type=int, default=10)
    ap.add_argument('--out', type=str, default=None, help='default: profiles/<loss>_loss_bench.jsonl')
    ap.add_argument('--no-updates', action='store_true', help='skip the training updates')
    args = ap.parse_args()
    out = args.out if args.out is not None else os.path.join(ROOT, 'profiles', args.loss + '_loss_bench.jsonl')
    assert torch.cuda.is_available(), 'loss_bench needs a GPU: there is nothing to time without one'
    torch.cuda.set_device(0)
    vfi.configure_miopen()
    module_ms = launch_lines(args.loss, args.reps, out)
    if not args.no_updates:
        update_lines(args.loss, args.updates, out, module_ms)


if __name__ == '__main__':
    main()
