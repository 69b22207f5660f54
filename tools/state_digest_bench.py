#!/usr/bin/env python3
"""The state digest (tai_state_digest, run_state.digest) on the full-width TAI_gray training state.

  python tools/state_digest_bench.py [--reps 50] [--out profiles/state_digest_bench.jsonl]

Builds the TAI_gray training environment at 128 x 128 (generator, spectral-norm discriminator, both Adam optimizers with their moments
in place, the u vectors drawn), then times
  launch_ms      HIP events around tai_state_digest alone (the table already on the device), median of --reps;
  digest_wall_ms run_state.digest(env) end to end: the host entries summed with numpy, the table built and uploaded, the launch, the
                 read-back of the result;
and the box's once-read streaming rate (tai_hbm_read_probe, default cache policy and non-temporal loads, 1.2 GB) in the same process:
`fraction_of_streaming_read` = device bytes / launch time over the better of the two.  One JSON line, printed and written to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import _native, parallel, run_state  # noqa: E402
from video_frame_inpainting_amd.environments import create_training_environment  # noqa: E402

UPDATE_MS = 203.0        # one training update of the flagship configuration (README)


def streaming_read_GBps(device, nt, reps=10):
    nbytes = 1200 << 20
    a = torch.empty(nbytes // 4, dtype=torch.float32, device=device).fill_(1.0)
    sink = torch.zeros(4096, dtype=torch.float32, device=device)
    L = _native.lib()
    stream = torch.cuda.current_stream(device).cuda_stream
    run = lambda: _native.check(L.tai_hbm_read_probe(a.data_ptr(), nbytes, int(nt), sink.data_ptr(), stream), 'hbm_read_probe')
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    e1.synchronize()
    return nbytes / (e0.elapsed_time(e1) * 1e3 / reps) / 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--graph_step', action='store_true', help="Adam's step counters on the device (capturable), as with train.py --graph_step")
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'state_digest_bench.jsonl'))
    args = ap.parse_args()
    device = torch.device('cuda:0')
    torch.cuda.set_device(device)
    torch.manual_seed(0)
    env = create_training_environment(vfi.create_model('TAI_gray'), 1, os.path.join(ROOT, 'build', 'no_checkpoints'), 'state_digest_bench',
                                      5, 5, 5, [128, 128], 1.0, 0.02, 1e-4, 0.5, 64, 3, 3, [0, 0], device=device,
                                      graph_step=args.graph_step)
    parallel.materialise_sn_vectors(env.discriminator)
    for module, optimizer in ((env.generator, env.optimizer_G), (env.discriminator, env.optimizer_D)):
        for p in module.parameters():                          # one Adam step on small gradients: the moments and counters exist
            p.grad = torch.full_like(p, 1e-3)
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)
    torch.cuda.synchronize()

    entries = run_state.state_entries(env)
    host, dev, n_segments = run_state.build_table(entries)
    device_words = int(sum(r[1] for r in host if r[0] != 0))
    host_words = int(sum(r[1] for r in host if r[0] == 0))
    L = _native.lib()
    table = torch.from_numpy(host).to(device)
    workspace = torch.empty(L.tai_state_digest_workspace_bytes(host.shape[0], n_segments) // 8 + 1, dtype=torch.int64, device=device)
    result = torch.zeros(1, dtype=torch.int64, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    run = lambda: _native.check(L.tai_state_digest(table.data_ptr(), host.ctypes.data, host.shape[0], n_segments, run_state.SEG_WORDS,
                                                   workspace.data_ptr(), result.data_ptr(), stream), 'tai_state_digest')
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    value = int(result.item()) & ((1 << 64) - 1)
    wall = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        again = run_state.digest(env)
        wall.append((time.perf_counter() - t0) * 1e3)
    assert again == value, (again, value)
    rates = {'default': streaming_read_GBps(device, 0), 'nt': streaming_read_GBps(device, 1)}
    launch_ms = float(np.median(times))
    rec = {'metric': 'state_digest', 'model': 'TAI_gray 128x128', 'graph_step': bool(args.graph_step), 'entries': int(host.shape[0]),
           'segments': int(n_segments), 'seg_words': run_state.SEG_WORDS, 'device_bytes': 4 * device_words, 'host_bytes': 4 * host_words,
           'reps': args.reps, 'launch_ms_median': round(launch_ms, 4), 'launch_ms_min': round(float(np.min(times)), 4),
           'launch_ms_max': round(float(np.max(times)), 4), 'launch_GBps': round(4 * device_words / launch_ms / 1e6, 1),
           'streaming_read_GBps_default': round(rates['default'], 1), 'streaming_read_GBps_nt': round(rates['nt'], 1),
           'fraction_of_streaming_read': round(4 * device_words / launch_ms / 1e6 / max(rates.values()), 4),
           'digest_wall_ms_median': round(float(np.median(wall)), 3), 'update_ms': UPDATE_MS,
           'launch_fraction_of_update': round(launch_ms / UPDATE_MS, 5), 'wall_fraction_of_update': round(float(np.median(wall)) / UPDATE_MS, 5),
           'digest': '%016x' % value}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
