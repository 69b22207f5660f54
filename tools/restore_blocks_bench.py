#!/usr/bin/env python3
"""Partly damaged frames: the block scan, the composite and restore.py's two passes with and without --detect_blocks.

  python tools/restore_blocks_bench.py [--launches 20] [--skip_end_to_end] [--out profiles/restore_blocks_bench.jsonl]

HIP events around --launches back-to-back launches, the variants alternating window by window in one process, three rounds of --reps
windows each, the median of every round and the spread of the three medians.  One JSON line per row:
  block_scan        on resident RGB videos of 512 x 120 x 160, 256 x 240 x 320 and 2048 x 240 x 320 (the last is past the Infinity Cache),
                    bs 16, tol 0 and 3: tai_block_scan against tai_frame_scan on the same buffer (the yardstick: same bytes, same read
                    pattern), tai_hbm_read_probe in the same process, and the torch-op restatement on the device;
  damage_composite  64 items of 128 x 128 gray and 16 of 240 x 320 colour, feather 4, one block in eight damaged: tai_damage_composite
                    against the same definition in torch ops (two frames_to_uint8_device, a max_pool2d ramp, an integer blend);
  end_to_end        a 256-frame 240 x 320 restore (randomly initialised TAI_color, a painted block in every 16th frame) with and without
                    --detect_blocks blank: wall time of pass 1 and of the fill, legs alternating, with the leg-to-leg spread.
Results are required to be equal (to the numpy restatements / to each other) before anything is timed."""
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from block_scan_ref import block_scan_ref  # noqa: E402
from damage_composite_ref import damage_composite_ref  # noqa: E402
from frame_scan_bench import streaming_read_GBps  # noqa: E402
from video_frame_inpainting_amd import _native, restore  # noqa: E402
from video_frame_inpainting_amd.clip_pipeline import frames_to_uint8_device  # noqa: E402

SCAN_SHAPES = (('120x160 colour', 512, 120, 160, 3), ('240x320 colour', 256, 240, 320, 3), ('240x320 colour, past the cache', 2048, 240, 320, 3))
COMP_SHAPES = (('128x128 gray', 64, 128, 128, 1), ('240x320 colour', 16, 240, 320, 3))
MODEL = 'TAI_color'                     # the end-to-end row's model: the colour configuration, which takes 240 x 320 planes


def alternating(runs, launches, reps):
    """{name: call} -> {name: the three rounds' medians of the time per call, ms}; within a round the variants take turns, window by window."""
    medians = {k: [] for k in runs}
    for _ in range(3):
        times = {k: [] for k in runs}
        for _ in range(reps):
            for k, (run, share) in runs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                m = max(1, launches // share)
                a.record()
                for _ in range(m):
                    run()
                b.record()
                b.synchronize()
                times[k].append(a.elapsed_time(b) / m)
        for k in runs:
            medians[k].append(float(np.median(times[k])))
    return medians


def summary(prefix, rounds):
    ms = float(np.median(rounds))
    return {prefix + '_ms_round_medians': [round(t, 5) for t in rounds], prefix + '_ms': round(ms, 5),
            prefix + '_ms_spread': round((max(rounds) - min(rounds)) / ms, 4)}


def torch_block_scan(video, bs, tol):
    """The block statistics in torch ops (zero padding up to whole blocks, int16 differences, int64 sums)."""
    n, h, w, c = video.shape
    Bh, Bw = -(-h // bs), -(-w // bs)
    cells = lambda a: torch.nn.functional.pad(a, (0, 0, 0, Bw * bs - w, 0, Bh * bs - h)).reshape(a.shape[0], Bh, bs, Bw, bs, c).sum(
        dim=(2, 4, 5), dtype=torch.int64)
    out = torch.zeros(n, Bh, Bw, 4, dtype=torch.int64, device=video.device)
    v = video.to(torch.int32)
    out[..., 0] = cells(v)
    out[..., 1] = cells(v * v)
    d = (video[1:].to(torch.int16) - video[:-1].to(torch.int16)).abs()
    out[1:, ..., 2] = cells(d)
    out[1:, ..., 3] = cells((d > tol).to(torch.int16))
    return out


def torch_composite(pred, src, core, h, w, feather, rgb):
    """The definition in torch ops: pred, src fp32 [n, C, Hs, Ws]; core bool [n, h, w] -> uint8 [n, h, w, C]."""
    R = feather + 1
    P, S = frames_to_uint8_device(pred, h, w, rgb).to(torch.int32), frames_to_uint8_device(src, h, w, rgb).to(torch.int32)
    A, grown = core.to(torch.int32) * R, core[:, None].float()
    for d in range(1, R):
        grown = torch.nn.functional.max_pool2d(grown, 3, 1, 1)
        A = torch.maximum(A, grown[:, 0].to(torch.int32) * (R - d))
    A = A[..., None]
    return ((2 * (A * P + (R - A) * S) + R) // (2 * R)).to(torch.uint8)


def bench_scan(args, device, probe, emit):
    L, stream = _native.lib(), torch.cuda.current_stream(device).cuda_stream
    for name, n, h, w, c in SCAN_SHAPES:
        rng = np.random.RandomState(n + h)
        host = rng.randint(0, 256, (n, h, w, c)).astype(np.uint8)
        host[n // 2, 16:32, 32:48] = host[n // 2 - 1, 16:32, 32:48]
        video = torch.from_numpy(host).to(device)
        bs, Bh, Bw = 16, -(-h // 16), -(-w // 16)
        stats = torch.empty(n, Bh, Bw, 4, dtype=torch.int64, device=device)
        fstats = torch.empty(n, 4, dtype=torch.int64, device=device)
        fwork = torch.empty(L.tai_frame_scan_workspace_bytes(n, h * w * c) // 8, dtype=torch.int64, device=device)
        assert L.tai_block_scan_workspace_bytes(n, h, w, c, bs) == 0
        for tol in (0, 3):
            ours = lambda: _native.check(L.tai_block_scan(video.data_ptr(), n, h, w, c, bs, tol, stats.data_ptr(), None, stream), 'tai_block_scan')
            frame = lambda: _native.check(L.tai_frame_scan(video.data_ptr(), n, h * w * c, tol, fstats.data_ptr(), fwork.data_ptr(), stream),
                                          'tai_frame_scan')
            ours(), frame()
            want = torch.from_numpy(block_scan_ref(host[:17], bs, tol))
            assert torch.equal(stats[:17].cpu(), want) and torch.equal(stats.sum(dim=(1, 2)), fstats)
            assert torch.equal(torch_block_scan(video[:64], bs, tol), stats[:64])
            small = video[:max(64, n // 8)]                       # the torch form's temporaries of the whole video would not fit
            t = alternating({'block_scan': (ours, 1), 'frame_scan': (frame, 1), 'torch': (lambda: torch_block_scan(small, bs, tol), 8)},
                            args.launches, args.reps)
            ms, fms = float(np.median(t['block_scan'])), float(np.median(t['frame_scan']))
            nbytes = n * h * w * c
            gbps = nbytes / ms / 1e6
            rec = {'metric': 'block_scan', 'shape': name, 'frames': n, 'H': h, 'W': w, 'C': c, 'bs': bs, 'tol': tol, 'video_bytes': nbytes,
                   'fits_infinity_cache': nbytes <= 256 << 20, 'launches_per_window': args.launches, 'windows_per_round': args.reps}
            rec.update(summary('block_scan', t['block_scan']))
            rec.update(summary('frame_scan', t['frame_scan']))
            rec.update({'GBps': round(gbps, 1), 'frame_scan_GBps': round(nbytes / fms / 1e6, 1), 'share_of_frame_scan_rate': round(fms / ms, 4),
                        'streaming_read_GBps': round(probe, 1), 'share_of_streaming_read': round(gbps / probe, 4),
                        'torch_frames': int(small.shape[0]), 'torch_ms_scaled_to_the_video': round(float(np.median(t['torch'])) * n / small.shape[0], 4),
                        'torch_over_kernel': round(float(np.median(t['torch'])) * n / small.shape[0] / ms, 1)})
            emit(rec)
        del video, stats


def bench_composite(args, device, emit):
    for name, n, h, w, C in COMP_SHAPES:
        rng = np.random.RandomState(h)
        bs, feather, rgb = 16, 4, C == 3
        pred = torch.from_numpy(rng.uniform(-1.2, 1.2, (n, C, h, w)).astype(np.float32)).to(device)
        src = torch.from_numpy(rng.uniform(-1.2, 1.2, (n, C, h, w)).astype(np.float32)).to(device)
        maps = (rng.rand(n, -(-h // bs), -(-w // bs)) < 0.125).astype(np.uint8)
        taps_host = restore.tap_tables(h, h) + restore.tap_tables(w, w)
        taps = [torch.from_numpy(t).to(device) for t in taps_host]
        items = [[k * C * h * w, k * C * h * w, k, k] for k in range(n)]
        table_host = torch.tensor(items, dtype=torch.int64)
        table, blocks = table_host.to(device), torch.from_numpy(maps).to(device)
        out = torch.empty(n, h, w, C, dtype=torch.uint8, device=device)
        L, stream = _native.lib(), torch.cuda.current_stream(device).cuda_stream
        ours = lambda: _native.check(L.tai_damage_composite(
            pred.data_ptr(), pred.numel(), src.data_ptr(), src.numel(), table.data_ptr(), table_host.data_ptr(), n, blocks.data_ptr(), n,
            maps.shape[1], maps.shape[2], bs, taps[0].data_ptr(), taps[1].data_ptr(), taps[2].data_ptr(), taps[3].data_ptr(), out.data_ptr(), n, C,
            h, w, h, w, feather, int(rgb), stream), 'tai_damage_composite')
        core = blocks.bool().repeat_interleave(bs, 1).repeat_interleave(bs, 2)[:, :h, :w].contiguous()        # identity taps
        theirs = lambda: torch_composite(pred, src, core, h, w, feather, rgb)
        ours()
        assert torch.equal(out, theirs())
        for k in (0, n - 1):
            assert np.array_equal(out[k].cpu().numpy(), damage_composite_ref(pred[k].cpu().numpy(), src[k].cpu().numpy(), maps[k], taps_host, bs, h, w,
                                                                             feather, rgb))
        t = alternating({'kernel': (ours, 1), 'torch': (theirs, 4)}, args.launches, args.reps)
        rec = {'metric': 'damage_composite', 'shape': name, 'items': n, 'h': h, 'w': w, 'C': C, 'bs': bs, 'feather': feather,
               'damaged_share': round(float(maps.mean()), 4), 'out_bytes': n * h * w * C}
        rec.update(summary('kernel', t['kernel']))
        rec.update(summary('torch', t['torch']))
        rec['torch_over_kernel'] = round(rec['torch_ms'] / rec['kernel_ms'], 1)
        emit(rec)


def bench_end_to_end(args, device, emit, tmp):
    import video_frame_inpainting_amd as vfi
    from video_frame_inpainting_amd.environments import create_eval_environment
    from video_frame_inpainting_amd.options import RestoreOptions
    n, h, w = 256, 240, 320
    rng = np.random.RandomState(3)
    video = rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    for i in range(8, n - 8, 16):
        video[i, 64:80, 96:112] = 77
    path = os.path.join(tmp, 'video.npy')
    np.save(path, video)
    base = ['--name', 'b', '--K', '3', '--T', '1', '--F', '3', '--c_dim', '3', '--image_size', str(h), str(w), '--model_key', MODEL, '--random_init',
            '--checkpoints_dir', os.path.join(tmp, 'ckpt'), '--input', path, '--output_dir', os.path.join(tmp, 'out'), '--batch_size', '4']
    legs = {'off': base + ['--gaps', ','.join(str(i) for i in range(8, n - 8, 16))], 'detect_blocks blank': base + ['--detect_blocks', 'blank']}
    vfi.configure_miopen()
    torch.manual_seed(0)
    times = {k: {'pass1_s': [], 'fill_s': []} for k in legs}
    env = None
    for leg in range(4):                                   # the first leg of each warms up and is dropped
        for k, argv in legs.items():
            opt = RestoreOptions().parse(argv, require_gpu=True)
            if env is None:
                env = create_eval_environment(vfi.create_model(opt.model_key), opt.checkpoints_dir, opt.name, opt.snapshot_file_name, opt.padding_size,
                                              device=device, load_snapshot=False)
            r = restore.Restorer(env, opt)
            reader, present = restore.open_source(path)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats, flags, gaps = r.plan(reader, present, device)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            frames = r.model_frames(reader)
            out_u8 = np.zeros((n, h, w, 3), dtype=np.uint8)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            r.fill(frames, gaps, out_u8)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            assert sum(g['status'] == 'fill' for g in gaps) == 15 and (k == 'off' or int((flags == restore.PARTIAL).sum()) == 15)
            if leg:
                times[k]['pass1_s'].append(t1 - t0)
                times[k]['fill_s'].append(t3 - t2)
            del frames
    rec = {'metric': 'end_to_end', 'frames': n, 'H': h, 'W': w, 'gaps': 15, 'legs_timed': 3}
    for k, t in times.items():
        for part, v in t.items():
            rec['%s %s' % (k, part)] = round(float(np.median(v)), 4)
            rec['%s %s spread' % (k, part)] = round((max(v) - min(v)) / float(np.median(v)), 4)
    emit(rec)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--launches', type=int, default=20, help='back-to-back launches per timed window')
    ap.add_argument('--reps', type=int, default=9, help='windows per round')
    ap.add_argument('--skip_end_to_end', action='store_true')
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'restore_blocks_bench.jsonl'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU: there is no fallback'
    device = torch.device('cuda:0')
    torch.cuda.set_device(device)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(rec):
        print(json.dumps(rec), flush=True)
        with open(args.out, 'a') as f:
            f.write(json.dumps(rec) + '\n')
    probe = max(streaming_read_GBps(device, 0), streaming_read_GBps(device, 1))
    bench_scan(args, device, probe, emit)
    bench_composite(args, device, emit)
    if not args.skip_end_to_end:
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            bench_end_to_end(args, device, emit, tmp)


if __name__ == '__main__':
    main()
