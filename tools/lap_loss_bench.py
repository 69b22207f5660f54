#!/usr/bin/env python3
"""The Laplacian-pyramid loss (tai_lap_loss, losses.LapLoss, train.py --lap_weight): the launch against the torch composition of the
same definition, and one eager TAI_gray update with and without the term.

  python tools/lap_loss_bench.py [--reps 30] [--updates 10] [--out profiles/lap_loss_bench.jsonl]

(a) launches   at [160, 1, 128, 128] (TAI_gray, 32 clips x 5 frames; the pyramid in LDS) and [48, 3, 256, 256] (the pyramid in the
               workspace), 5 levels, loss + gradient:
                 kernel   tai_lap_loss through the C ABI, outputs and workspace made once (the two launches only);
                 module   LapLoss forward + backward through autograd (what an update pays: allocations, the fp32 scalar, grad * map);
                 torch    forward + backward of the same definition composed from torch ops in float64 on the same device
                          (losses._lap_terms, the module's host path);
               HIP events, median of --reps; the variants alternate in one process and the whole comparison is made three times:
               `ms` is the median of the three medians, `spread_ms` the largest distance between the three medians of any variant.
               `kernel_share_of_8TBps`: the algorithmic bytes (pred and gt read, grad written: 12 per pixel) over the kernel's time, as a
               share of the HBM peak.
(b) updates    eager milliseconds per update of two TAI_gray training environments at 128 x 128, 32 clips, K = T = F = 5, without the
               term and with --lap_weight 0.5 (three pyramid terms per update); legs alternate, three times, --updates each after a
               warm-up.
No threshold: the ratio and the added milliseconds are reported as measured.  One JSON line per measurement, printed and appended to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import _native, losses, synthetic  # noqa: E402
from video_frame_inpainting_amd.environments import create_training_environment  # noqa: E402
from grad_guard_bench import event_ms  # noqa: E402

SHAPES = (('TAI_gray 32 clips x 5', 160, 1, 128, 128), ('color 256x256', 48, 3, 256, 256))
LEVELS = 5
K = T = F = 5
BATCH, SIZE = 32, 128
DEV = torch.device('cuda:0')


def kernel_launcher(p, g):
    L = _native.lib()
    N, C, H, W = p.shape
    nbytes = L.tai_lap_loss_workspace_bytes(N * C, H, W, LEVELS)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    out = torch.empty(N * C * LEVELS + LEVELS + 1, dtype=torch.float64, device=DEV)
    grad = torch.empty_like(p)
    stream = torch.cuda.current_stream().cuda_stream

    def run():
        _native.check(L.tai_lap_loss(p.data_ptr(), g.data_ptr(), LEVELS, out.data_ptr(), out[N * C * LEVELS:].data_ptr(), grad.data_ptr(),
                                     ws.data_ptr(), N * C, H, W, stream), 'tai_lap_loss')
    return run, out, grad, nbytes


def launch_lines(reps, out_path):
    for name, N, C, H, W in SHAPES:
        clips = synthetic.make_clips(N, 2, C, H, W, 31)
        p = torch.from_numpy(np.ascontiguousarray(clips[:, 0])).to(DEV)
        g = torch.from_numpy(np.ascontiguousarray(clips[:, 1])).to(DEV)
        kernel, out, grad, ws_bytes = kernel_launcher(p, g)
        module = losses.LapLoss(LEVELS)
        pm, pt = p.clone().requires_grad_(), p.clone().requires_grad_()

        def run_module():
            pm.grad = None
            module(pm, g).backward()

        def run_torch():
            pt.grad = None
            losses._lap_terms(pt, g, LEVELS)[0].to(torch.float32).backward()
        runs = {'kernel': kernel, 'module': run_module, 'torch': run_torch}
        meds = {k: [] for k in runs}
        for _ in range(3):
            for k, run in runs.items():
                meds[k].append(event_ms(run, reps))
        torch.cuda.synchronize()
        # the three compute one thing: the kernel's map against autograd of the composition (both exact: no word should differ)
        scale = float(pt.grad.abs().max())
        diff = float((grad - pt.grad).abs().max())
        words = int((grad.view(torch.int32) != pt.grad.view(torch.int32)).sum())
        ms = {k: float(np.median(v)) for k, v in meds.items()}
        spread = max(max(v) - min(v) for v in meds.values())
        pixels = N * C * H * W
        emit({'metric': 'lap_loss_launch', 'levels': LEVELS, 'shape': name, 'N': N, 'C': C, 'H': H, 'W': W, 'reps': reps,
              'library_version': _native.lib().tai_sepconv_version(), 'workspace_bytes': ws_bytes,
              'ms_medians': {k: [round(x, 4) for x in v] for k, v in meds.items()}, 'ms': {k: round(v, 4) for k, v in ms.items()},
              'spread_ms': round(spread, 4), 'kernel_Gpixel_per_s': round(pixels / ms['kernel'] / 1e6, 2),
              'kernel_min_traffic_GBps': round(12 * pixels / ms['kernel'] / 1e6, 1),         # reads pred and gt, writes grad: 12 bytes per pixel
              'kernel_share_of_8TBps': round(12 * pixels / ms['kernel'] / 1e6 / 8000.0, 4),
              'torch_over_kernel': round(ms['torch'] / ms['kernel'], 2), 'torch_over_module': round(ms['torch'] / ms['module'], 2),
              'kernel_faster_than_torch_by_more_than_the_spread': bool(ms['torch'] - ms['kernel'] > spread),
              'loss': float(out[-1]), 'grad_max': scale, 'grad_max_diff_to_torch_autograd': diff,
              'grad_words_differing_from_torch_autograd': words}, out_path)
        del pm, pt, runs, kernel, grad, out
        torch.cuda.empty_cache()


def make_env(name, **kw):
    torch.manual_seed(0)
    env = create_training_environment(vfi.create_model('TAI_gray'), 1, os.path.join(ROOT, 'build', 'no_checkpoints'), name,
                                      K, T, F, [SIZE, SIZE], 1.0, 0.02, 1e-4, 0.5, 64, 3, 3, [0, 0], device=DEV, **kw)
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


def update_lines(updates, out_path):
    clips = torch.from_numpy(synthetic.make_clips(2 * BATCH, K + T + F, 1, SIZE, SIZE, 1002))
    envs = {'plain': make_env('llb_plain'), 'lap': make_env('llb_lap', lap_weight=0.5, lap_levels=LEVELS)}
    for env in envs.values():
        update_ms(env, clips, 3)                                 # MIOpen's searches, lazy allocations, Adam's state
    legs = {k: [] for k in envs}
    for _ in range(3):
        for k, env in envs.items():
            legs[k].append(update_ms(env, clips, updates))
    ms = {k: float(np.median(v)) for k, v in legs.items()}
    spread = max(max(v) - min(v) for v in legs.values())
    errs = envs['lap'].get_current_errors()
    emit({'metric': 'lap_loss_update', 'model': 'TAI_gray 128x128', 'batch': BATCH, 'KTF': [K, T, F], 'lap_weight': 0.5, 'levels': LEVELS,
          'updates_per_leg': updates, 'ms_legs': {k: [round(x, 3) for x in v] for k, v in legs.items()},
          'ms': {k: round(v, 3) for k, v in ms.items()}, 'spread_ms': round(spread, 3),
          'added_ms_per_update': round(ms['lap'] - ms['plain'], 3), 'ratio': round(ms['lap'] / ms['plain'], 4),
          'added_is_more_than_the_spread': bool(ms['lap'] - ms['plain'] > spread),
          'G_lap': [round(errs[k], 5) for k in ('G_lap', 'G_lap_forward', 'G_lap_backward')]}, out_path)


def emit(rec, out_path):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'a') as f:
            f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--updates', type=int, default=10)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'lap_loss_bench.jsonl'))
    ap.add_argument('--no-updates', action='store_true', help='skip the training updates')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'lap_loss_bench needs a GPU: there is nothing to time without one'
    torch.cuda.set_device(0)
    vfi.configure_miopen()
    launch_lines(args.reps, args.out)
    if not args.no_updates:
        update_lines(args.updates, args.out)


if __name__ == '__main__':
    main()
