#!/usr/bin/env python3
"""The temporal-difference loss (tai_temporal_loss, losses.TemporalLoss, train.py --temporal_weight): one launch for three predictions
against the same definition in torch ops, and one eager TAI_gray update with and without the term.

  python tools/temporal_loss_bench.py [--reps 30] [--updates 10] [--out profiles/temporal_loss_bench.jsonl]

(a) launches   three predictions against one ground truth at [32, 5, 1, 128, 128] (TAI_gray, 32 clips; ``pred`` stored time-major, as
               tai.py returns it, the other two and the ground truth [B, T, ...]) and [16, 3, 3, 256, 256], loss + gradient of all
               three, kind 2 (Charbonnier, the default of the flag):
                 kernel   tai_temporal_loss through the C ABI, outputs and workspace made once (the three launches only);
                 module   TemporalLoss forward + backward through autograd (what an update pays: allocations, fp32 scalars, grad * map);
                 torch    forward + backward of the same definition in torch ops on the same device (losses._temporal_terms, the
                          module's own path for tensors the kernel does not take), once per prediction;
               HIP events, median of --reps; the variants alternate in one process and the whole comparison is made three times:
               `ms` is the median of the three medians, `spread_ms` the largest distance between the three medians of any variant.
               The launch's bytes ((npred + 1) reads + npred writes of 4 bytes per element) over its time are given as a fraction of the
               HBM peak.
(b) updates    eager milliseconds per update of two TAI_gray training environments at 128 x 128, 32 clips, K = T = F = 5, without the
               term and with --temporal_weight 0.5; legs alternate, three times, --updates each after a warm-up.  The difference is
               given next to the leg-to-leg spread, and next to what the module alone takes at the update's shape.
No threshold: the ratios and the milliseconds are reported as measured.  One JSON line per measurement, printed and appended to --out."""
import argparse
import ctypes
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

SHAPES = (('TAI_gray 32 clips x 5, pred time-major', (32, 5, 1, 128, 128), True), ('color 256x256', (16, 3, 3, 256, 256), False))
NPRED = 3
KIND, EPS = 2, 1e-3
HBM_PEAK_GBPS = 8000.0
K = T = F = 5
BATCH, SIZE = 32, 128
DEV = torch.device('cuda:0')


def time_major(x):
    """The values of ``x`` [B, T, ...] stored [T, B, ...]: a transposed view, as tai.py returns ``pred``."""
    return x.transpose(0, 1).contiguous().transpose(0, 1)


def kernel_launcher(preds, g):
    L = _native.lib()
    B, Tn, C, H, W = g.shape
    n = len(preds)
    S = B * C
    nbytes = L.tai_temporal_loss_workspace_bytes(n, B, Tn, C, H, W)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    out = torch.empty(n * S * (Tn + 1) + n * (Tn + 2), dtype=torch.float64, device=DEV)
    grads = [torch.empty_strided(p.shape, p.stride(), dtype=torch.float32, device=DEV) for p in preds]
    pred_ptrs = (ctypes.c_void_p * n)(*[p.data_ptr() for p in preds])
    grad_ptrs = (ctypes.c_void_p * n)(*[x.data_ptr() for x in grads])
    strides = (ctypes.c_longlong * (2 * n + 2))(*[v for t in list(preds) + [g] for v in losses._block_strides(t)])
    stream = torch.cuda.current_stream().cuda_stream
    totals = out[n * S * (Tn + 1):]

    def run():
        _native.check(L.tai_temporal_loss(pred_ptrs, n, g.data_ptr(), strides, KIND, EPS, out.data_ptr(), totals.data_ptr(), grad_ptrs,
                                          ws.data_ptr(), B, Tn, C, H, W, stream), 'tai_temporal_loss')
    return run, totals.view(n, Tn + 2), grads, nbytes


def launch_lines(reps, out_path):
    module_ms = {}
    for name, shape, pred_time_major in SHAPES:
        B, Tn, C, H, W = shape
        clips = synthetic.make_clips(B, Tn * (NPRED + 1), C, H, W, 31).reshape(B, NPRED + 1, Tn, C, H, W)
        g = torch.from_numpy(np.ascontiguousarray(clips[:, 0])).to(DEV)
        preds = [torch.from_numpy(np.ascontiguousarray(clips[:, 1 + i])).to(DEV) for i in range(NPRED)]
        if pred_time_major:
            preds[0] = time_major(preds[0])
        kernel, totals, grads, ws_bytes = kernel_launcher(preds, g)
        module = losses.TemporalLoss(losses.IMAGE_LOSS_KINDS[KIND], EPS)
        pm = [p.detach().clone(memory_format=torch.preserve_format).requires_grad_() for p in preds]
        pt = [p.detach().clone(memory_format=torch.preserve_format).requires_grad_() for p in preds]
        assert [p.stride() for p in pm] == [p.stride() for p in preds]

        def run_module():
            for p in pm:
                p.grad = None
            a, b, c = module(tuple(pm), g)
            (a + b + c).backward()

        def run_torch():
            for p in pt:
                p.grad = None
            total = sum(losses._temporal_terms(p, g, KIND, EPS)[0] for p in pt)
            total.backward()
        runs = {'kernel': kernel, 'module': run_module, 'torch': run_torch}
        meds = {k: [] for k in runs}
        for _ in range(3):
            for k, run in runs.items():
                meds[k].append(event_ms(run, reps))
        torch.cuda.synchronize()
        # the three compute one thing: the kernel's maps against autograd of the torch ops
        scale = max(float(p.grad.abs().max()) for p in pt)
        diff = max(float((x - p.grad).abs().max()) for x, p in zip(grads, pt))
        ms = {k: float(np.median(v)) for k, v in meds.items()}
        spread = max(max(v) - min(v) for v in meds.values())
        module_ms[tuple(shape)] = ms['module']
        nbytes = (2 * NPRED + 1) * 4 * g.numel()
        emit({'metric': 'temporal_loss_launch', 'shape': name, 'dims': list(shape), 'npred': NPRED, 'kind': 'charbonnier', 'reps': reps,
              'strides': [list(losses._block_strides(t)) for t in preds + [g]],
              'library_version': _native.lib().tai_sepconv_version(), 'workspace_bytes': ws_bytes,
              'ms_medians': {k: [round(x, 4) for x in v] for k, v in meds.items()}, 'ms': {k: round(v, 4) for k, v in ms.items()},
              'spread_ms': round(spread, 4), 'launch_bytes': nbytes, 'kernel_GBps': round(nbytes / ms['kernel'] / 1e6, 1),
              'kernel_fraction_of_hbm_peak': round(nbytes / ms['kernel'] / 1e6 / HBM_PEAK_GBPS, 4), 'hbm_peak_GBps': HBM_PEAK_GBPS,
              'torch_over_kernel': round(ms['torch'] / ms['kernel'], 2), 'torch_over_module': round(ms['torch'] / ms['module'], 2),
              'module_faster_than_torch_by_more_than_the_spread': bool(ms['torch'] - ms['module'] > spread),
              'losses': [float(x) for x in totals[:, -1]], 'grad_max': scale, 'grad_max_diff_to_torch_autograd': diff}, out_path)
        del pm, pt, runs, kernel, grads, totals
        torch.cuda.empty_cache()
    return module_ms


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


def update_lines(updates, out_path, module_ms):
    clips = torch.from_numpy(synthetic.make_clips(2 * BATCH, K + T + F, 1, SIZE, SIZE, 1002))
    envs = {'plain': make_env('tlb_plain'), 'temporal': make_env('tlb_temporal', temporal_weight=0.5)}
    for env in envs.values():
        update_ms(env, clips, 3)                                 # MIOpen's searches, lazy allocations, Adam's state
    legs = {k: [] for k in envs}
    for _ in range(3):
        for k, env in envs.items():
            legs[k].append(update_ms(env, clips, updates))
    ms = {k: float(np.median(v)) for k, v in legs.items()}
    spread = max(max(v) - min(v) for v in legs.values())
    errs = envs['temporal'].get_current_errors()
    alone = module_ms.get((BATCH, T, 1, SIZE, SIZE))
    emit({'metric': 'temporal_loss_update', 'model': 'TAI_gray 128x128', 'batch': BATCH, 'KTF': [K, T, F], 'temporal_weight': 0.5,
          'kind': 'charbonnier', 'updates_per_leg': updates,
          'ms_legs': {k: [round(x, 3) for x in v] for k, v in legs.items()}, 'ms': {k: round(v, 3) for k, v in ms.items()},
          'spread_ms': round(spread, 3), 'temporal_minus_plain_ms': round(ms['temporal'] - ms['plain'], 3),
          'ratio': round(ms['temporal'] / ms['plain'], 4), 'difference_is_more_than_the_spread': bool(abs(ms['temporal'] - ms['plain']) > spread),
          'module_alone_ms_at_this_shape': None if alone is None else round(alone, 4),
          'G_temporal': [round(errs[k], 5) for k in ('G_temporal', 'G_temporal_forward', 'G_temporal_backward')]}, out_path)


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
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'temporal_loss_bench.jsonl'))
    ap.add_argument('--no-updates', action='store_true', help='skip the training updates')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'temporal_loss_bench needs a GPU: there is nothing to time without one'
    torch.cuda.set_device(0)
    vfi.configure_miopen()
    module_ms = launch_lines(args.reps, args.out)
    if not args.no_updates:
        update_lines(args.updates, args.out, module_ms)


if __name__ == '__main__':
    main()
