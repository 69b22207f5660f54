#!/usr/bin/env python3
"""The gradient guard (tai_grad_stats, train.py --guard) on the full-width TAI_gray training environment.

  python tools/grad_guard_bench.py [--reps 50] [--updates 20] [--out profiles/grad_guard_bench.jsonl]

Builds the TAI_gray training environment at 128 x 128, 32 clips, K = T = F = 5, makes one real update so that the gradients are real, then
  kernel_ms     HIP events around tai_grad_stats alone (the table already on the device) over the generator's and over the
                discriminator's gradients, median of --reps, and its share of the box's once-read streaming rate (tai_hbm_read_probe in
                the same process), the bytes computed from the table;
  torch_ms      the same job spelled in PyTorch on the same gradients: torch.nn.utils.clip_grad_norm_ with a max_norm that does not clip
                plus one torch.isfinite(...).all() per tensor reduced to one flag, timed the same way; the two alternate in one process
                and the whole comparison is made three times: `spread_ms` is the largest distance between the three medians of either;
  update_ms     eager milliseconds per update without and with the guard (order A B A B, --updates each after a warm-up): the
                difference includes the two small device-to-host reads per update that the host needs before it may decide about a step.
One JSON line, printed and appended to --out."""
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
from video_frame_inpainting_amd import _native, grad_guard, run_state, synthetic  # noqa: E402
from video_frame_inpainting_amd.environments import create_training_environment  # noqa: E402
from state_digest_bench import streaming_read_GBps  # noqa: E402

K = T = F = 5
BATCH, SIZE = 32, 128


def event_ms(run, reps):
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def kernel_launcher(grads):
    """tai_grad_stats over `grads`, the table and the buffers made once -> (callable, bytes read, segments)."""
    rows, device, n_segments = run_state.build_table(grads, grad_guard.SEG)
    L = _native.lib()
    n = rows.shape[0]
    table = torch.from_numpy(rows).to(device)
    workspace = torch.empty(L.tai_grad_stats_workspace_bytes(n, n_segments) // 8 + 2, dtype=torch.int64, device=device)
    result = torch.zeros(5 * (n + 1), dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    base = result.data_ptr()
    run = lambda: _native.check(L.tai_grad_stats(table.data_ptr(), rows.ctypes.data, n, n_segments, 0, workspace.data_ptr(), base,
                                                 base + 16 * (n + 1), base + 8 * (n + 1), stream), 'tai_grad_stats')
    run.keep = (table, workspace, result, rows)
    return run, 4 * int(rows[:, 1].sum()), int(n_segments)


def torch_spelling(params):
    def run():
        torch.nn.utils.clip_grad_norm_(params, 1e30)
        return torch.stack([torch.isfinite(p.grad).all() for p in params]).all()
    return run


def update_ms(env, clips, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        c = clips[(i % 2) * BATCH:(i % 2 + 1) * BATCH]
        env.train_step(c[:, :K], c[:, K + T:], c[:, K:K + T])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--updates', type=int, default=20)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'grad_guard_bench.jsonl'))
    args = ap.parse_args()
    device = torch.device('cuda:0')
    torch.cuda.set_device(device)
    torch.manual_seed(0)
    env = create_training_environment(vfi.create_model('TAI_gray'), 1, os.path.join(ROOT, 'build', 'no_checkpoints'), 'grad_guard_bench',
                                      K, T, F, [SIZE, SIZE], 1.0, 0.02, 1e-4, 0.5, 64, 3, 3, [0, 0], device=device)
    clips = torch.from_numpy(synthetic.make_clips(2 * BATCH, K + T + F, 1, SIZE, SIZE, 1002))
    env.K, env.T, env.F = K, T, F
    env.train()
    update_ms(env, clips, 3)                                     # real gradients in place; MIOpen's searches done

    rec = {'metric': 'grad_guard', 'model': 'TAI_gray 128x128', 'batch': BATCH, 'KTF': [K, T, F], 'reps': args.reps,
           'library_version': _native.lib().tai_sepconv_version()}
    rates = {'default': streaming_read_GBps(device, 0), 'nt': streaming_read_GBps(device, 1)}
    rec.update(streaming_read_GBps_default=round(rates['default'], 1), streaming_read_GBps_nt=round(rates['nt'], 1))
    for which, module in (('G', env.generator), ('D', env.discriminator)):
        params = [p for p in module.parameters() if p.grad is not None]
        grads = [p.grad for p in params]
        kernel, nbytes, n_segments = kernel_launcher(grads)
        spelled = torch_spelling(params)
        kernel_meds, torch_meds = [], []
        for _ in range(3):                                       # the whole comparison three times, the two alternating
            kernel_meds.append(event_ms(kernel, args.reps))
            torch_meds.append(event_ms(spelled, args.reps))
        (sumsq, maxabs, bad), totals = grad_guard.grad_stats(grads)
        want = float(torch.nn.utils.clip_grad_norm_(params, 1e30))
        k_ms, t_ms = float(np.median(kernel_meds)), float(np.median(torch_meds))
        spread = max(max(kernel_meds) - min(kernel_meds), max(torch_meds) - min(torch_meds))
        rec[which] = {'tensors': len(grads), 'bytes': nbytes, 'segments': n_segments,
                      'kernel_ms_medians': [round(v, 4) for v in kernel_meds], 'torch_ms_medians': [round(v, 4) for v in torch_meds],
                      'kernel_ms': round(k_ms, 4), 'torch_ms': round(t_ms, 4), 'spread_ms': round(spread, 4),
                      'kernel_faster_by_more_than_the_spread': bool(t_ms - k_ms > spread),
                      'kernel_GBps': round(nbytes / k_ms / 1e6, 1),
                      'fraction_of_streaming_read': round(nbytes / k_ms / 1e6 / max(rates.values()), 4),
                      'norm': float(np.sqrt(totals[0])), 'norm_torch_fp32': want, 'nonfinite': totals[2]}
    # eager updates without (A) and with (B) the guard, A B A B
    legs = {'A': [], 'B': []}
    for leg in 'ABAB':
        env.guard = grad_guard.GradGuard() if leg == 'B' else None
        update_ms(env, clips, 2)
        legs[leg].append(update_ms(env, clips, args.updates))
    env.guard = None
    a, b = float(np.mean(legs['A'])), float(np.mean(legs['B']))
    rec.update(updates_per_leg=args.updates, update_ms_plain_legs=[round(v, 3) for v in legs['A']],
               update_ms_guard_legs=[round(v, 3) for v in legs['B']], update_ms_plain=round(a, 3), update_ms_guard=round(b, 3),
               guard_ms_per_update=round(b - a, 3), guard_fraction_of_update=round((b - a) / a, 5))
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
