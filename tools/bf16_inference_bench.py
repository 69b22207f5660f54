#!/usr/bin/env python3
"""fp32 against the opt-in bf16 convolution mode (conv_ops.set_conv_precision) in ONE process on the same box: the forward of
configs[1] (TAI_gray 128x128, 32 clips, T = 5), configs[3] (TAI_color 256x256, 16 clips, T = 5) and configs[4] (TAI_gray, 32 clips,
T = 10), bench.py's seeded weights and clips, hipGraph replay.  Each mode's graph is captured with the mode set; the two are then
replayed alternately for several rounds.  Prints one JSON line per config and round-set (frames/s per mode and the ratio).
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bf16_inference_bench.py --configs 1`.

Usage (repository root):  python tools/bf16_inference_bench.py [--configs 1,3,4] [--rounds 5] [--reps 5]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import conv_ops, synthetic  # noqa: E402
from video_frame_inpainting_amd.graph import GraphedForward  # noqa: E402

# index: (model key, clips, C, H, W, K, T, F, clip seed)
CONFIGS = {1: ('TAI_gray', 32, 1, 128, 128, 5, 5, 5, 'cfg2'),
           3: ('TAI_color', 16, 3, 256, 256, 3, 5, 3, 'cfg4'),
           4: ('TAI_gray', 32, 1, 128, 128, 5, 10, 5, 'cfg5')}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--configs', default='1,3,4')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5, help='replays per mode per round')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.backends.cudnn.allow_tf32 = False
    vfi.configure_miopen()
    for idx in [int(c) for c in args.configs.split(',')]:
        key, B, C, H, W, K, T, F, seed = CONFIGS[idx]
        m = synthetic.seeded_init(vfi.create_model(key), 0).to(dev).eval()
        clips = synthetic.make_clips(B, K + T + F, C, H, W, synthetic.SEEDS[seed])
        P, _, Fo = (torch.from_numpy(x).to(dev) for x in synthetic.split_clip(clips, K, T, F))
        graphs = {}
        for mode in ('fp32', 'bf16'):
            prev = conv_ops.set_conv_precision(mode)
            try:
                graphs[mode] = GraphedForward(m, T, P, Fo, warmup=1)
            finally:
                conv_ops.set_conv_precision(prev)
        ms = {'fp32': [], 'bf16': []}
        for _ in range(args.rounds):
            for mode in ('fp32', 'bf16'):
                g = graphs[mode]
                g()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    g()
                torch.cuda.synchronize()
                ms[mode].append((time.perf_counter() - t0) * 1e3 / args.reps)
        best = {k: min(v) for k, v in ms.items()}
        print(json.dumps({'config': idx, 'model': key, 'clips': B, 'T': T,
                          'ms_per_forward': {k: [round(x, 2) for x in v] for k, v in ms.items()},
                          'frames_per_s_best': {k: round(B * T / (v / 1e3), 1) for k, v in best.items()},
                          'bf16_speedup_best': round(best['fp32'] / best['bf16'], 3)}), flush=True)
        del graphs, m
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
