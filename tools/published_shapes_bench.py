"""TAI_color at the reference's published shapes on one GPU, with and without the odd-plane routes (conv_ops.set_ragged_routes):

  * inference: 240 x 320 BGR, K = F = 4, T = 3, 16 clips per step (the UCF-101 / HMDB-51 test argument files), hipGraph replay,
    2 warm-up + `--steps` timed replays -> frames/s;
  * training: one G + D update (train_step: GAN + reconstruction losses, Adam, fp32) at 160 x 208, K = F = 4, T = 3, 16 clips,
    eager as train.py issues it, 2 warm-up + `--steps` timed updates -> ms per update;
  * for both, the ATen convolutions (MIOpen on ROCm) one step launches, one count per convolution or convolution backward
    (torch.profiler, CPU side: the eager forward for inference).

  python tools/published_shapes_bench.py [--steps 3] [--out profiles/published_shapes.json]

One JSON document on stdout (and in --out).  The odd planes of these shapes: the kernel network's bottom (15 x 20 at 240 x 320,
10 x 13 at 160 x 208), the weight gradients on rows of 20-104 pixels, the discriminator's last layer (10 x 13 space-to-depth plane)."""
import argparse
import contextlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import conv_ops, synthetic  # noqa: E402
from video_frame_inpainting_amd.graph import GraphedForward  # noqa: E402

# one profiler event per ATen convolution: the MIOpen leaf of a forward (F.conv2d -> aten::conv2d -> aten::convolution ->
# aten::_convolution -> aten::miopen_convolution: only the last is counted) and the backward entry (aten::convolution_backward, the
# op autograd and conv_ops call; its MIOpen leaves are not counted again)
ATEN_CONVS = ('aten::miopen_convolution', 'aten::miopen_convolution_transpose', 'aten::miopen_depthwise_convolution',
              'aten::convolution_backward')


def _aten_convs(fn):
    """(convolutions counted, {op name: events} of every convolution-related ATen op seen, for the record)"""
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    names = {}
    for e in prof.events():
        if 'conv' in e.name and e.name.startswith('aten::'):
            names[e.name] = names.get(e.name, 0) + 1
    return sum(v for k, v in names.items() if k in ATEN_CONVS), names


def inference(device, steps, B=16, H=240, W=320, K=4, T=3, F=4):
    torch.backends.cudnn.allow_tf32 = False
    m = synthetic.seeded_init(vfi.create_model('TAI_color'), 0).to(device).eval()
    clips = synthetic.make_clips(B, K + T + F, 3, H, W, synthetic.SEEDS['cfg4'])
    P, _, Fo = (torch.from_numpy(x).to(device) for x in synthetic.split_clip(clips, K, T, F))
    with torch.no_grad():
        convs, ops = _aten_convs(lambda: m(T, P, Fo))
        g = GraphedForward(m, T, P, Fo, warmup=1)
        for _ in range(2):
            g()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            g()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        pred = g()['pred'].float().cpu().numpy()
    del g, m
    torch.cuda.empty_cache()
    return {'clips': B, 'frame': [3, H, W], 'K_T_F': [K, T, F], 'ms_per_step': round(dt * 1e3, 2), 'frames_per_s': round(B * T / dt, 1),
            'steps_timed': steps, 'aten_convolutions_per_step': convs, 'aten_conv_op_events': ops, 'pred_finite': bool(np.isfinite(pred).all())}


def training(device, steps, B=16, H=160, W=208, K=4, T=3, F=4):
    from video_frame_inpainting_amd.environments import create_training_environment
    torch.backends.cudnn.allow_tf32 = False
    with contextlib.redirect_stdout(sys.stderr):
        env = create_training_environment(vfi.create_model('TAI_color'), 3, tempfile.mkdtemp(prefix='tai_pub_'), 'pub', K, T, F, [H, W],
                                          1.0, 0.02, 1e-4, 0.5, 64, 3, 3, [0, 0], device=device)
    env.sync_replicas()
    clips = torch.from_numpy(synthetic.make_clips(B, K + T + F, 3, H, W, synthetic.SEEDS['cfg3']))
    P, GT, Fo = synthetic.split_clip(clips, K, T, F)

    def step():
        env.K, env.T, env.F = K, T, F
        env.train()
        env.train_step(P, Fo, GT)
    t0 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    convs, ops = _aten_convs(step)
    errs = env.get_current_errors()
    del env
    torch.cuda.empty_cache()
    return {'clips': B, 'frame': [3, H, W], 'K_T_F': [K, T, F], 'ms_per_update': round(dt * 1e3, 1), 'updates_timed': steps,
            'first_update_s': round(first, 2), 'aten_convolutions_per_update': convs, 'aten_conv_op_events': ops,
            'losses_finite': bool(all(np.isfinite(v) for v in errs.values()))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--legs', default='inference,training')
    args = ap.parse_args()
    device = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(device), 'miopen_find_mode': os.environ.get('MIOPEN_FIND_MODE')}
    for leg in args.legs.split(','):
        fn = {'inference': inference, 'training': training}[leg]
        for routes in ('new', 'old'):
            prev = conv_ops.set_ragged_routes(routes == 'new')
            try:
                res['%s_%s_routes' % (leg, routes)] = r = fn(device, args.steps)
            finally:
                conv_ops.set_ragged_routes(prev)
            print('%s, %s routes: %s' % (leg, routes, r), file=sys.stderr)
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
