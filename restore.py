#!/usr/bin/env python3
"""Repair a damaged video: find the damaged frames, plan the gaps, fill them with the model, write the whole sequence.

``predict.py`` is told where the gap is and is handed a clip of exactly K + T + F frames around it.  This driver takes the video as it
is: it scans every frame once on the GPU (``tai_frame_scan``), flags what the source lacks (``--detect missing``), what repeats the frame
before it (``dup``), what is constant (``blank``) and what the caller names (``--gaps``), chooses K and F per gap from the intact frames
around it, and writes ``frame_%06d.png`` for every frame plus ``report.json`` (video_frame_inpainting_amd/restore.py has the rules).
Gaps that cannot be filled (no two intact frames on a side, longer than ``--max_T``) are left as the source delivered them and are
listed in the report; the exit status is 0 all the same.

  python restore.py --name demo --K 5 --T 5 --F 5 --c_dim 1 --image_size 128 --model_key TAI_gray \
      --input damaged_frames/ --output_dir restored/ --detect missing,dup
"""
import sys

import torch


def main(args=None):
    from video_frame_inpainting_amd.options import RestoreOptions
    from video_frame_inpainting_amd.restore import Restorer
    argv = list(sys.argv[1:] if args is None else args)
    dry = '--dry_run' in argv
    opt = RestoreOptions().parse(argv, require_gpu=not dry)
    env = None
    if not dry:
        import video_frame_inpainting_amd as vfi
        from video_frame_inpainting_amd import conv_ops
        from video_frame_inpainting_amd.environments import create_eval_environment
        vfi.configure_miopen()
        device = torch.device('cuda', 0)
        torch.cuda.set_device(device)
        if opt.winograd_arithmetic != 'fp32':
            conv_ops.set_winograd_arithmetic(opt.winograd_arithmetic)
        if opt.conv_precision != 'fp32':
            conv_ops.set_conv_precision(opt.conv_precision)
        if opt.winograd_tile in (2, 4):
            conv_ops.set_winograd_tile(opt.winograd_tile)
        torch.manual_seed(0)
        env = create_eval_environment(vfi.create_model(opt.model_key), opt.checkpoints_dir, opt.name, opt.snapshot_file_name,
                                      opt.padding_size, device=device, load_snapshot=not opt.random_init, weights=opt.weights)
    try:
        report = Restorer(env, opt).run(opt.input, opt.output_dir)
    except (ValueError, IOError) as e:
        raise SystemExit('restore: %s' % e)
    for g in report['gaps']:
        print('gap at frame %d: T=%d K=%d F=%d %s' % (g['start'], g['T'], g['K'], g['F'], g['status']))
    filled = sum(g['status'] == 'fill' for g in report['gaps'])
    print('%d frames, %d flagged, %d gaps: %d filled, %d left as they were%s -> %s' % (
        report['n_frames'], sum(f['flags'] != 0 for f in report['frames']), len(report['gaps']), 0 if dry else filled,
        len(report['gaps']) - (0 if dry else filled), ' (dry run: nothing filled)' if dry else '', opt.output_dir))
    return report


if __name__ == '__main__':
    main()
