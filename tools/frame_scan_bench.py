#!/usr/bin/env python3
"""The frame scan (tai_frame_scan, restore.scan_frames) on videos resident on the device.

  python tools/frame_scan_bench.py [--launches 20] [--out profiles/frame_scan_bench.jsonl]

Per shape -- 512 frames of 128 x 128 gray, 256 frames of 240 x 320 colour, and 2048 frames of 240 x 320 colour (472 MB: the only one of the
three that does not fit the 256 MiB Infinity Cache, so the only one whose rate is a rate of HBM) -- one JSON line with
  launch_ms        HIP events around --launches back-to-back launches (both kernels of the entry), divided by their number; three rounds of
                   --reps such windows each, the median of every round and the spread of the three medians;
  GBps             the video's bytes (each counted once) over the median launch time, and its share of the 8 TB/s peak and of the box's
                   own once-read streaming rate (tai_hbm_read_probe, 1.2 GB, default cache policy and non-temporal loads, the better of
                   the two) measured in the same process;
  torch_ms         the same four sums written in torch ops on the device (int16 differences, int64 sums), timed the same way;
  numpy_ms         the numpy restatement on the host (wall clock, the frames already in host memory), once;
and the three results are required to be equal before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from frame_scan_ref import frame_scan_ref  # noqa: E402
from video_frame_inpainting_amd import _native  # noqa: E402

PEAK_GBPS = 8000.0
SHAPES = (('128x128 gray', 512, 128, 128, 1), ('240x320 colour', 256, 240, 320, 3), ('240x320 colour, past the cache', 2048, 240, 320, 3))


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


def torch_scan(video, tol):
    """The four sums in torch ops, frame by frame pairs in one expression each (int16 differences: no wrap)."""
    n = video.shape[0]
    v = video.reshape(n, -1)
    w = v.to(torch.int32)
    out = torch.zeros(n, 4, dtype=torch.int64, device=video.device)
    out[:, 0] = w.sum(dim=1, dtype=torch.int64)
    out[:, 1] = (w * w).sum(dim=1, dtype=torch.int64)
    d = (v[1:].to(torch.int16) - v[:-1].to(torch.int16)).abs()
    out[1:, 2] = d.sum(dim=1, dtype=torch.int64)
    out[1:, 3] = (d > tol).sum(dim=1, dtype=torch.int64)
    return out


def windows(run, launches, reps):
    """Three rounds of ``reps`` windows of ``launches`` back-to-back calls -> the rounds' medians of the time per call, ms."""
    medians = []
    for _ in range(3):
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                run()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) / launches)
        medians.append(float(np.median(times)))
    return medians


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--launches', type=int, default=20, help='back-to-back launches per timed window')
    ap.add_argument('--reps', type=int, default=9, help='windows per round')
    ap.add_argument('--tol', type=int, default=0)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'frame_scan_bench.jsonl'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU: there is no fallback'
    device = torch.device('cuda:0')
    torch.cuda.set_device(device)
    L = _native.lib()
    stream = torch.cuda.current_stream(device).cuda_stream
    probe = {'default': streaming_read_GBps(device, 0), 'nt': streaming_read_GBps(device, 1)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name, n, h, w, c in SHAPES:
        rng = np.random.RandomState(n + h)
        host = rng.randint(0, 256, (n, h, w, c)).astype(np.uint8)
        host[n // 2] = host[n // 2 - 1]
        video = torch.from_numpy(host).to(device)
        frame_bytes = h * w * c
        need = L.tai_frame_scan_workspace_bytes(n, frame_bytes)
        stats = torch.empty(n, 4, dtype=torch.int64, device=device)
        workspace = torch.empty(need // 8, dtype=torch.int64, device=device)
        run = lambda: _native.check(L.tai_frame_scan(video.data_ptr(), n, frame_bytes, args.tol, stats.data_ptr(), workspace.data_ptr(), stream),
                                    'tai_frame_scan')
        run()
        t0 = time.perf_counter()
        # (in blocks of 256 frames behind the previous block's last frame: the int64 temporaries of the whole video would not fit the host)
        want = np.concatenate([frame_scan_ref(host[max(a - 1, 0):a + 256], args.tol)[1 if a else 0:] for a in range(0, n, 256)])
        numpy_ms = (time.perf_counter() - t0) * 1e3
        assert torch.equal(stats.cpu(), torch.from_numpy(want)) and torch.equal(torch_scan(video, args.tol).cpu(), torch.from_numpy(want))
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        ours = windows(run, args.launches, args.reps)
        theirs = windows(lambda: torch_scan(video, args.tol), max(1, args.launches // 4), max(3, args.reps // 3))
        ms = float(np.median(ours))
        gbps = n * frame_bytes / ms / 1e6
        rec = {'metric': 'frame_scan', 'shape': name, 'frames': n, 'H': h, 'W': w, 'C': c, 'frame_bytes': frame_bytes, 'video_bytes': n * frame_bytes,
               'fits_infinity_cache': n * frame_bytes <= 256 << 20, 'tol': args.tol, 'launches_per_window': args.launches, 'windows_per_round': args.reps,
               'launch_ms_round_medians': [round(t, 5) for t in ours], 'launch_ms': round(ms, 5),
               'launch_ms_spread': round((max(ours) - min(ours)) / ms, 4), 'GBps': round(gbps, 1), 'fraction_of_8TBps_peak': round(gbps / PEAK_GBPS, 4),
               'streaming_read_GBps_default': round(probe['default'], 1), 'streaming_read_GBps_nt': round(probe['nt'], 1),
               'fraction_of_streaming_read': round(gbps / max(probe.values()), 4), 'workspace_bytes': int(need),
               'torch_ms_round_medians': [round(t, 4) for t in theirs], 'torch_ms': round(float(np.median(theirs)), 4),
               'torch_over_kernel': round(float(np.median(theirs)) / ms, 1), 'numpy_ms': round(numpy_ms, 1), 'numpy_over_kernel': round(numpy_ms / ms, 1)}
        print(json.dumps(rec), flush=True)
        with open(args.out, 'a') as f:
            f.write(json.dumps(rec) + '\n')
        del video, stats, workspace


if __name__ == '__main__':
    main()
