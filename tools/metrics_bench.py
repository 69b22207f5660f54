#!/usr/bin/env python3
"""Frame metrics (PSNR / SSIM / L2) on the GPU against the host restatement, and one validation leg end to end.

  python tools/metrics_bench.py [--reps 50] [--host-reps 2]

Kernel: metrics.frame_metrics_device with its output and workspace preallocated (the two launches only), HIP events around each
call, median of --reps.  Host: metrics.compute_errors on the same frames (numpy float64, per frame), median of --host-reps.
Shapes: configs[1] [32, 5, 1, 128, 128], configs[3] [16, 5, 3, 256, 256], TAI_color at 240x320 [16, 5, 3, 240, 320].  Device
inputs come from HBM as the validation loop hands them over; the kernel reads both tensors once.

Validation leg: TAI_gray at configs[1]'s shape (K = F = 5, T = 5), 64 seeded synthetic clips in batches of 32, seeded weights:
validation.run_leg (eager forward + compute_errors_device per batch) against the same forwards scored by the host metric.
One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import _native, metrics, synthetic, validation  # noqa: E402
from video_frame_inpainting_amd.environments import create_eval_environment  # noqa: E402

SHAPES = (('configs[1]', 32, 5, 1, 128, 128), ('configs[3]', 16, 5, 3, 256, 256), ('TAI_color 240x320', 16, 5, 3, 240, 320))


def kernel_ms(p, g, reps):
    N = p.shape[0] * p.shape[1]
    C, H, W = p.shape[2:]
    nbytes = _native.lib().tai_frame_metrics_workspace_bytes(N, C, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    out = torch.empty(3, N, dtype=torch.float64, device=p.device)
    pf, gf = p.reshape(N, C, H, W), g.reshape(N, C, H, W)
    for _ in range(5):
        metrics.frame_metrics_device(pf, gf, out, ws)
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        metrics.frame_metrics_device(pf, gf, out, ws)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), nbytes


def host_ms(pred, gt, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        metrics.compute_errors(pred, gt)
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def metric_lines(reps, host_reps):
    dev = torch.device('cuda:0')
    for name, B, T, C, H, W in SHAPES:
        clips = synthetic.make_clips(B, 2 * T, C, H, W, 31)
        pred, gt = clips[:, :T], clips[:, T:]
        p, g = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
        k_ms, ws_bytes = kernel_ms(p, g, reps)
        # end to end as compute_errors_device runs: launches, one copy of the [3, B T] results, PSNR on the host
        t0 = time.perf_counter()
        for _ in range(10):
            metrics.compute_errors_device(p, g)
        e2e_ms = (time.perf_counter() - t0) * 1e2
        h_ms = host_ms(pred, gt, host_reps)
        read = 2 * pred.nbytes
        print(json.dumps({'metric': 'frame_metrics', 'shape': name, 'frames': B * T, 'C': C, 'H': H, 'W': W,
                          'kernel_ms': round(k_ms, 4), 'kernel_read_GBps': round(read / k_ms / 1e6, 1), 'workspace_bytes': ws_bytes,
                          'device_call_ms': round(e2e_ms, 3), 'host_ms': round(h_ms, 2), 'host_over_kernel': round(h_ms / k_ms, 1)}),
              flush=True)


class _Opt(object):
    pass


def leg_lines(n_clips=64, batch=32):
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    env = create_eval_environment(vfi.create_model('TAI_gray'), 'checkpoints', 'bench', None, [0, 0], device=dev, load_snapshot=False)
    synthetic.seeded_init(env.generator, 5)          # after the environment's own init
    opt = _Opt()
    opt.K = opt.F = opt.T = 5
    opt.image_size, opt.padding_size, opt.c_dim, opt.batch_size, opt.seed = [128, 128], [0, 0], 1, batch, 1002
    leg = validation.Leg('T', 5, 5, 5, ('synthetic', n_clips))
    cache = {}
    validation.run_leg(env, leg, opt, 0, 1, cache)            # warm-up: MIOpen, lazy allocations, the clips themselves
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    psnr, ssim, _ = validation.run_leg(env, leg, opt, 0, 1, cache)
    dev_s = time.perf_counter() - t0
    # the same forwards scored by the host metric
    clips = cache[leg]
    t0 = time.perf_counter()
    fwd = 0.0
    for i in range(0, n_clips, batch):
        b = clips[i:i + batch].to(dev)
        f0 = time.perf_counter()
        env.set_test_inputs(b[:, :5], b[:, 10:])
        env.T = 5
        env.eval()
        env.forward_test()
        pred = env.gen_output['pred'].cpu().numpy()
        fwd += time.perf_counter() - f0
        metrics.compute_errors(pred, b[:, 5:10].cpu().numpy())
    host_s = time.perf_counter() - t0
    print(json.dumps({'metric': 'validation_leg', 'model': 'TAI_gray', 'clips': n_clips, 'batch': batch, 'K,T,F': [5, 5, 5],
                      'device_metric_s': round(dev_s, 4), 'host_metric_s': round(host_s, 4), 'forward_and_copy_s': round(fwd, 4),
                      'mean_psnr': round(float(np.mean(psnr)), 4), 'mean_ssim': round(float(np.mean(ssim)), 5)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--host-reps', type=int, default=2)
    ap.add_argument('--no-leg', action='store_true', help='skip the validation leg')
    args = ap.parse_args()
    vfi.configure_miopen()
    metric_lines(args.reps, args.host_reps)
    if not args.no_leg:
        leg_lines()


if __name__ == '__main__':
    main()
