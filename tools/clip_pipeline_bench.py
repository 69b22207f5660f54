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
read per 5 produced).

  python tools/clip_pipeline_bench.py --augment [--reps 10] [--launches 200] [--updates 10] [--out profiles/clip_augment_bench.jsonl]

The augmented way in (train.py --aug_*; tai_clip_from_frames_aug), on the same rows and batches.  Per row, three variants in turn, the
round three times, each result HIP events around --launches back-to-back launches on a resident batch (`ms_medians` the three results,
`ms` their median, `spread_ms` the largest distance between the three results of any variant):
  existing           tai_clip_from_frames;
  aug_neutral        tai_clip_from_frames_aug with a full-frame window and neutral tables, one per clip: the same work and the same bits
                     (asserted), the yardstick for the staged form;
  aug_crop_flicker   --aug_crop 0.5 with the other flags on and --aug_flicker: a window per clip, a table per frame;
then the augmented host path through --workers DataLoader workers against the device path's wall clock (pack into pinned staging with
the tables, one upload, one kernel).  A last line: eager TAI_gray updates (128 x 128, 32 clips, K = T = F = 5, the KTH row's frames)
that build their clip on the device first, with and without the flags; legs alternate, three times, --updates each after a warm-up."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from video_frame_inpainting_amd import _native, clip_pipeline  # noqa: E402
from video_frame_inpainting_amd.data import ClipAugment, _ArrayVideo, _ClipReader, with_window  # noqa: E402
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

    def __init__(self, clips, reader, raw, length, augment=None):
        self.clips, self.reader, self.raw, self.length, self.augment = clips, reader, raw, length, augment

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        frames = self.clips[i % len(self.clips)]
        source = _ArrayVideo(frames, 'memory')
        aug = None if self.augment is None else with_window(self.augment.draw(random.Random(i), T), frames.shape[1], frames.shape[2])
        if self.raw:
            item = {'frames': self.reader.raw_clip(source, range(T), True), 'mirror': True, 'clip_label': str(i)}
            return item if aug is None else dict(item, aug=aug)
        return self.reader.clip(source, range(T), True, True, aug)


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


AUGMENT = dict(crop=0.5, vflip=True, brightness=0.2, contrast=0.3, gamma=0.5, flicker=0.1)


def events_ms(run, launches):
    """Milliseconds per call of ``run`` from HIP events around ``launches`` back-to-back calls, after a warm-up."""
    for _ in range(3):
        run()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        run()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def alternate(runs, measure):
    """Every variant in turn, the whole round three times -> ({variant: its three results}, {variant: their median}, the largest distance
    between the three results of any variant)."""
    results = {k: [] for k in runs}
    for _ in range(3):
        for k, run in runs.items():
            results[k].append(measure(run))
    return results, {k: float(np.median(v)) for k, v in results.items()}, max(max(v) - min(v) for v in results.values())


def augment_kernels(items_by_variant, builder, launches):
    """The three launches on resident batches -> (alternate()'s results, the outputs of 'existing' and 'aug_neutral' for the equality)."""
    dev, L = builder.device, _native.lib()
    n = B * T
    (H, W), (ph, pw) = builder.image_size, builder.padding_size
    levels = clip_pipeline.level_tables().to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    runs, outs, keep = {}, {}, []
    for name, items in items_by_variant.items():
        batch = clip_pipeline.collate_raw(items)
        staged, out = batch['packed'].to(dev), torch.empty(n, builder.c_dim, H + ph, W + pw, device=dev)
        keep.append((batch, staged))
        outs[name] = out
        if 'n_tables' in batch:
            head = clip_pipeline.aug_header_bytes(n)
            first = head + batch['n_tables'] * clip_pipeline.TABLE_BYTES
            call = (L.tai_clip_from_frames_aug, (staged.data_ptr() + first, staged.numel() - first, staged.data_ptr(), batch['packed'].data_ptr(),
                                                 staged.data_ptr() + head, batch['n_tables'], levels.data_ptr(), out.data_ptr(), n, builder.c_dim,
                                                 H, W, ph, pw, stream))
        else:
            head = clip_pipeline.header_bytes(n)
            call = (L.tai_clip_from_frames, (staged.data_ptr() + head, staged.numel() - head, staged.data_ptr(), batch['packed'].data_ptr(),
                                             levels.data_ptr(), out.data_ptr(), n, builder.c_dim, H, W, ph, pw, stream))
        runs[name] = lambda call=call: _native.check(call[0](*call[1]), 'launch')
    result = alternate(runs, lambda run: events_ms(run, launches))
    torch.cuda.synchronize()
    return result, outs


def build_wall_ms(items, builder, reps):
    wall = []
    for rep in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        builder.build(clip_pipeline.collate_items(items))
        torch.cuda.synchronize()
        if rep >= 2:
            wall.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(wall))


def augment_updates(items_plain, items_aug, builder, updates):
    """Eager TAI_gray updates that build their clip on the device first, with and without augmentation records."""
    import video_frame_inpainting_amd as vfi
    from video_frame_inpainting_amd.environments import create_training_environment
    K = F = T_OUT
    torch.manual_seed(0)
    env = create_training_environment(vfi.create_model('TAI_gray'), 1, os.path.join(ROOT, 'build', 'no_checkpoints'), 'clip_augment_bench',
                                      K, T_OUT, F, list(builder.image_size), 1.0, 0.02, 1e-4, 0.5, 64, 3, 3, [0, 0], device=builder.device)
    env.K, env.T, env.F = K, T_OUT, F
    env.train()

    def update_ms(items, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            c = builder.build(clip_pipeline.collate_items(items))
            env.train_step(c[:, :K], c[:, K + T_OUT:], c[:, K:K + T_OUT])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n
    legs = {'plain': items_plain, 'augmented': items_aug}
    for items in legs.values():
        update_ms(items, 3)                                  # MIOpen's searches, lazy allocations, Adam's state
    return alternate(legs, lambda items: update_ms(items, updates))


def augment_main(args):
    frames = B * T
    augment = ClipAugment(**AUGMENT)
    out_path = args.out or os.path.join(ROOT, 'profiles', 'clip_augment_bench.jsonl')
    lines = []

    def make(h, w, c_dim, size, pad):
        rng = np.random.RandomState(h + c_dim)
        clips = [rng.randint(0, 256, (T, h, w, 3), dtype=np.uint8) for _ in range(B)]
        return clips, _ClipReader(c_dim, list(size), list(pad))

    # the host legs first, before this process opens the GPU: the forked workers must not inherit an open device
    host_times = {}
    for name, (h, w), size, pad, c_dim in ROWS:
        clips, reader = make(h, w, c_dim, size, pad)
        host_times[name] = host_workers(MemoryClips(clips, reader, False, B * args.worker_batches, augment), args.workers)
    update_items = None
    for name, (h, w), size, pad, c_dim in ROWS:
        clips, reader = make(h, w, c_dim, size, pad)
        plain = [MemoryClips(clips, reader, True, B)[i] for i in range(B)]
        cropped = [MemoryClips(clips, reader, True, B, augment)[i] for i in range(B)]
        neutral = [dict(it, aug=dict(c['aug'], window=(0, 0, h, w), vflip=False, gamma=1.0, gain=1.0, offset=0.0, flicker=None))
                   for it, c in zip(plain, cropped)]
        builder = clip_pipeline.DeviceClipBuilder(c_dim, size, pad, 'cuda:0')
        host = MemoryClips(clips, reader, False, B, augment)
        assert torch.equal(builder.build(clip_pipeline.collate_raw(cropped[:2])).cpu(), torch.stack([host[i] for i in range(2)]))
        (meds, ms, spread), outs = augment_kernels({'existing': plain, 'aug_neutral': neutral, 'aug_crop_flicker': cropped}, builder,
                                                   args.launches)
        assert torch.equal(outs['existing'], outs['aug_neutral'])                              # the same work, the same bits
        wall_plain, wall_aug = build_wall_ms(plain, builder, args.reps), build_wall_ms(cropped, builder, args.reps)
        b_s, b_n = host_times[name]
        moved = sum(int(np.prod(c.shape)) for c in clips) + outs['existing'].numel() * 4
        rec = {'metric': 'clip_augment', 'row': name, 'clips': B, 'frames_per_clip': T, 'c_dim': c_dim, 'decode': 'excluded',
               'library_version': _native.lib().tai_sepconv_version(), 'settings': augment.state(), 'launches_per_result': args.launches,
               'ms_medians': {k: [round(x, 5) for x in v] for k, v in meds.items()}, 'ms': {k: round(v, 5) for k, v in ms.items()},
               'spread_ms': round(spread, 5), 'aug_neutral_over_existing': round(ms['aug_neutral'] / ms['existing'], 3),
               'aug_neutral_slower_than_existing_by_more_than_the_spread': bool(ms['aug_neutral'] - ms['existing'] > spread),
               'full_frame_bytes': moved, 'existing_fraction_of_8TBps': round(moved / (ms['existing'] * 1e-3) / HBM_BYTES_PER_S, 4),
               'aug_neutral_fraction_of_8TBps': round(moved / (ms['aug_neutral'] * 1e-3) / HBM_BYTES_PER_S, 4),
               'host_workers': args.workers, 'host_workers_augmented_fps': round(frames / b_s, 1), 'host_workers_batches_timed': b_n,
               'device_wall_ms': {'plain': round(wall_plain, 3), 'augmented': round(wall_aug, 3)},
               'device_augmented_wall_fps': round(frames / (wall_aug * 1e-3), 1),
               'device_over_host_workers': round(b_s / (wall_aug * 1e-3), 2)}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        if update_items is None:                             # the KTH row: 120x160 -> 128x128 gray, TAI_gray's own shape
            update_items = (plain, cropped, builder)
    if not args.no_updates:
        legs, ms, spread = augment_updates(*update_items, args.updates)
        added = ms['augmented'] - ms['plain']
        rec = {'metric': 'clip_augment_update', 'model': 'TAI_gray 128x128', 'row': ROWS[0][0], 'batch': B, 'KTF': [T_OUT] * 3,
               'settings': augment.state(), 'updates_per_leg': args.updates, 'ms_legs': {k: [round(x, 3) for x in v] for k, v in legs.items()},
               'ms': {k: round(v, 3) for k, v in ms.items()}, 'spread_ms': round(spread, 3), 'augmented_minus_plain_ms': round(added, 3),
               'difference_is_more_than_the_spread': bool(abs(added) > spread)}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--augment', action='store_true', help='the augmented way in (tai_clip_from_frames_aug) instead of the rows above')
    ap.add_argument('--launches', type=int, default=200, help='(--augment) back-to-back launches per kernel result')
    ap.add_argument('--updates', type=int, default=10, help='(--augment) updates per leg of the update line')
    ap.add_argument('--no-updates', action='store_true', help='(--augment) skip the training updates')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--worker-batches', type=int, default=8, help='32-clip batches per pass of leg (b)')
    ap.add_argument('--out', type=str, default=None, help='default: profiles/clip_pipeline_bench.jsonl (clip_augment_bench.jsonl with --augment)')
    args = ap.parse_args()
    if args.augment:
        return augment_main(args)
    args.out = args.out or os.path.join(ROOT, 'profiles', 'clip_pipeline_bench.jsonl')
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
