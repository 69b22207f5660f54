#!/usr/bin/env python3
"""Clip preparation, host path against the device clip pipeline (--device_preprocess), and the way out to uint8 pixels.

  python tools/clip_pipeline_bench.py [--reps 10] [--workers 16] [--out profiles/clip_pipeline_bench.jsonl]

For each source -> clip row below and a batch of 32 clips x 15 frames (random uint8 frames held in memory: DECODE IS EXCLUDED
everywhere; mirror and time reversal on):
  (a) host path, one process: data._ClipReader.clip per clip, torch.stack of the batch;
  (b) host path through a DataLoader with --workers persistent workers, every worker busy (a first pass starts the workers and is
      not timed);
  (c) device path: DeviceClipBuilder.build on the raw items (pack into pinned staging, one upload, one kernel): wall clock around
      build + synchronize, the pack alone (into a pinned buffer), HIP events around build (the GPU's view: it waits for the pack,
      then upload + kernel), and HIP events around the kernel alone (tai_clip_from_frames on frames already resident), with the kernel's bytes (uint8 read once + fp32
      written) over 8 TB/s beside it;
  (d) the way out for 32 x 5 frames of the row's output shape: util.frames_to_uint8 after a float copy to the host against
      clip_pipeline.to_uint8_host.
Frames/s throughout; one JSON line per row, printed and written to --out.  `device_over_host_workers` > 1 is the feature's point;
`device_over_forward_appetite` compares (c) with 3 x the headline frames/s of profiles/r05_bench_line.json (K + T + F = 15 frames
read per 5 produced)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from video_frame_inpainting_amd import _native, clip_pipeline  # noqa: E402
from video_frame_inpainting_amd.data import _ArrayVideo, _ClipReader  # noqa: E402
from video_frame_inpainting_amd.util import frames_to_uint8  # noqa: E402

# name, source (h, w), output (H, W), padding, c_dim
ROWS = (('120x160 -> 128x128 gray (KTH)', (120, 160), (128, 128), (0, 0), 1),
        ('240x320 -> 240x320 + pad (16, 0) colour (UCF)', (240, 320), (240, 320), (16, 0), 3),
        ('240x320 -> 128x128 colour', (240, 320), (128, 128), (0, 0), 3),
        ('480x640 -> 128x128 gray', (480, 640), (128, 128), (0, 0), 1))
B, T, T_OUT = 32, 15, 5
HBM_BYTES_PER_S = 8e12


class MemoryClips(torch.utils.data.Dataset):
    """B in-memory clips served over and over; host mode returns the clip tensor, raw mode the frames."""

    def __init__(self, clips, reader, raw, length):
        self.clips, self.reader, self.raw, self.length = clips, reader, raw, length

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        frames = self.clips[i % len(self.clips)]
        source = _ArrayVideo(frames, 'memory')
        if self.raw:
            return {'frames': self.reader.raw_clip(source, range(T), True), 'mirror': True, 'clip_label': str(i)}
        return self.reader.clip(source, range(T), True, True)


def host_one_process(dataset):
    t0 = time.perf_counter()
    torch.stack([dataset[i] for i in range(B)])
    return time.perf_counter() - t0


def host_workers(dataset, workers):
    """Loader batches of B / workers clips, so that one 32-clip batch keeps every worker busy (their concatenation is not timed: the
    figure favours the host).  Persistent workers; the first pass over the dataset starts them and is not timed, the second is
    timed from iter() to its last batch."""
    loader = torch.utils.data.DataLoader(dataset, batch_size=max(B // workers, 1), shuffle=False, num_workers=workers, drop_last=True,
                                         persistent_workers=True)
    for _ in loader:
        pass
    t0 = time.perf_counter()
    n = 0
    for clips in loader:
        n += clips.shape[0]
    seconds = time.perf_counter() - t0
    del loader
    return seconds * B / n, n // B


def device_path(items, builder, reps):
    dev = builder.device
    wall, stream, pack = [], [], []
    scratch = torch.empty(clip_pipeline.packed_bytes([it['frames'] for it in items]), dtype=torch.uint8, pin_memory=True)
    for rep in range(reps + 2):
        t0 = time.perf_counter()
        clip_pipeline.pack_clips([it['frames'] for it in items], [it['mirror'] for it in items], out=scratch)
        if rep >= 2:
            pack.append(time.perf_counter() - t0)
    for rep in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        builder.build(clip_pipeline.collate_items(items))          # packs straight into the pinned staging buffer
        b.record()
        torch.cuda.synchronize()
        if rep >= 2:
            wall.append(time.perf_counter() - t0), stream.append(a.elapsed_time(b) * 1e-3)
    batch = clip_pipeline.collate_raw(items)
    # the kernel alone, on a resident batch
    n, head = B * T, clip_pipeline.header_bytes(B * T)
    staged = batch['packed'].to(dev)
    levels = clip_pipeline.level_tables().to(dev)
    (H, W), (ph, pw) = builder.image_size, builder.padding_size
    out = torch.empty(n, builder.c_dim, H + ph, W + pw, device=dev)
    L = _native.lib()
    kernel = []
    for rep in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _native.check(L.tai_clip_from_frames(staged.data_ptr() + head, staged.numel() - head, staged.data_ptr(), batch['packed'].data_ptr(),
                                             levels.data_ptr(), out.data_ptr(), n, builder.c_dim, H, W, ph, pw,
                                             torch.cuda.current_stream(dev).cuda_stream), 'tai_clip_from_frames')
        b.record()
        b.synchronize()
        if rep >= 2:
            kernel.append(a.elapsed_time(b) * 1e-3)
    moved = (staged.numel() - head) + out.numel() * 4
    med = lambda v: float(np.median(v))
    return med(pack), med(wall), med(stream), med(kernel), moved


def way_out(c_dim, Hs, Ws, h, w, reps):
    x = (torch.rand(B, T_OUT, c_dim, Hs, Ws) * 2.4 - 1.2).to('cuda:0')
    host, dev = [], []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        u = frames_to_uint8(x.float().cpu().reshape(-1, c_dim, Hs, Ws)[:, :, :h, :w])
        if c_dim == 3:
            u = np.ascontiguousarray(u[..., ::-1])
        t1 = time.perf_counter()
        v = clip_pipeline.to_uint8_host(x, h, w, c_dim == 3)
        t2 = time.perf_counter()
        if rep >= 1:
            host.append(t1 - t0), dev.append(t2 - t1)
    assert np.array_equal(u.reshape(v.shape), v)
    return float(np.median(host)), float(np.median(dev))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--worker-batches', type=int, default=8, help='32-clip batches per pass of leg (b)')
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'clip_pipeline_bench.jsonl'))
    args = ap.parse_args()
    headline = json.load(open(os.path.join(ROOT, 'profiles', 'r05_bench_line.json')))['value']
    appetite = 3.0 * headline
    frames = B * T
    lines = []

    def make(h, w, c_dim, size, pad):
        rng = np.random.RandomState(h + c_dim)
        clips = [rng.randint(0, 256, (T, h, w, 3), dtype=np.uint8) for _ in range(B)]
        reader = _ClipReader(c_dim, list(size), list(pad))
        return clips, reader, MemoryClips(clips, reader, False, B * args.worker_batches)

    # every host leg first, before this process opens the GPU: the forked workers must not inherit an open device
    host_times = {}
    for name, (h, w), size, pad, c_dim in ROWS:
        clips, reader, host = make(h, w, c_dim, size, pad)
        host_times[name] = (host_one_process(host),) + host_workers(host, args.workers)
        del clips, host
    for name, (h, w), size, pad, c_dim in ROWS:
        clips, reader, host = make(h, w, c_dim, size, pad)
        a_s, b_s, b_n = host_times[name]
        raw = MemoryClips(clips, reader, True, B)
        items = [raw[i] for i in range(B)]
        builder = clip_pipeline.DeviceClipBuilder(c_dim, size, pad, 'cuda:0')
        want = torch.stack([host[i] for i in range(2)])
        assert torch.equal(builder.build(clip_pipeline.collate_raw(items[:2])).cpu(), want)        # the same bits, before any timing
        pack_s, wall_s, stream_s, kernel_s, moved = device_path(items, builder, args.reps)
        out_host_s, out_dev_s = way_out(c_dim, size[0] + pad[0], size[1] + pad[1], size[0], size[1], max(args.reps // 2, 2))
        rec = {'metric': 'clip_pipeline', 'row': name, 'clips': B, 'frames_per_clip': T, 'c_dim': c_dim, 'decode': 'excluded',
               'host_1proc_fps': round(frames / a_s, 1), 'host_workers': args.workers, 'host_workers_fps': round(frames / b_s, 1),
               'host_workers_batches_timed': b_n,
               'device_wall_fps': round(frames / wall_s, 1), 'device_wall_ms': round(wall_s * 1e3, 3), 'pack_ms': round(pack_s * 1e3, 3),
               'events_ms_pack_upload_kernel': round(stream_s * 1e3, 3), 'kernel_ms': round(kernel_s * 1e3, 4),
               'kernel_bytes': moved, 'kernel_fraction_of_8TBps': round(moved / kernel_s / HBM_BYTES_PER_S, 4),
               'device_over_host_workers': round(b_s / wall_s, 2), 'device_over_host_1proc': round(a_s / wall_s, 2),
               'forward_appetite_fps': round(appetite, 1), 'device_over_forward_appetite': round(frames / wall_s / appetite, 2),
               'way_out_frames': B * T_OUT, 'way_out_host_fps': round(B * T_OUT / out_host_s, 1),
               'way_out_device_fps': round(B * T_OUT / out_dev_s, 1)}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        del clips, host, raw, items, builder
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
