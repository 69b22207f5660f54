#!/usr/bin/env python3
"""Training driver for the bi-TAI path: the step sequence of the reference's ``train.py:102-119`` (sample K,T,F ->
slice the clip -> set_train_inputs -> train() -> forward_train() -> optimize_parameters()), one process per GPU (data
parallel over RCCL when launched with torch.distributed.run), with the reference's snapshot files ``model_latest.ckpt``
/ ``model_%08d.ckpt`` (train.py:137-140).  Clips come from ``--train_video_list_path`` (the reference's list format and
augmentation flags, train.py:37-43; video_frame_inpainting_amd/data.py; each rank shuffles with its own seed) or, with
``--synthetic N``, from N seeded synthetic clips.  Every ``--validate_freq`` updates the reference's validation legs run
(train.py:142-196; video_frame_inpainting_amd/validation.py) on ``--val_video_list*_path`` or, with ``--val_synthetic N``, on N
seeded synthetic clips, scored on the GPU (metrics.compute_errors_device); the snapshot with the best summed per-frame SSIM of
the first leg is kept as ``model_best.ckpt``.  TensorBoard logging is outside the hot path.

``--resumable``: a run cut into several processes is the same run, bit for bit.  Snapshots carry ``run_state`` (run_state.py: the
spectral-norm vectors, every generator state, the clip order's position, a state digest computed on the GPU), the clip order is one
that can be entered at any position (data.ResumableBatchSampler), SIGTERM / SIGINT / ``--max_wall_minutes`` end the run after the
update in flight with ``model_latest.ckpt`` written, and every printed line ends with the state digest (``state=%016x``).

``--guard [--clip_grad_norm X] [--guard_patience N]``: the gradients are looked at before each optimizer step (grad_guard.py): an
optimizer whose gradients hold a NaN or an Inf does not step in that update, gradients are scaled to a norm of at most X, printed lines
carry ``gnorm_G= gnorm_D= skipped=``, a state with non-finite values is never written over a snapshot, and after N consecutive updates
with a skipped step the run ends with a non-zero exit, ``model_latest.ckpt`` being the last one written while healthy.

``--fused_step [--ema_decay d]``: each optimizer's step is one HIP launch (fused_step.py) that scales, updates and averages on a verdict
made on the device from the gradient statistics, so the host no longer waits between a backward pass and the step; the guard's counters
are read where the run waits anyway (a printed line, validation, a save).  With ``--ema_decay`` an average of the generator's weights is
kept, validated, and saved as ``generator_ema`` (``predict.py --weights ema``).

``--ssim_weight G``: the generator's loss gains G (1 - mean SSIM) of each prediction against the ground truth (losses.SSIMLoss: one HIP
launch writes the loss and its gradient); printed lines gain ``G_ssim=`` (and ``G_ssim_forward= G_ssim_backward=`` for TAI).  0 = off.

``--lap_weight G`` (with ``--lap_levels L``, default 5): the generator's loss gains G times the L1 distance between the Laplacian
pyramids of each prediction and the ground truth (losses.LapLoss: one HIP launch writes the loss and its gradient); printed lines gain
``G_lap=`` (and ``G_lap_forward= G_lap_backward=`` for TAI).  0 = off.

``--temporal_weight G`` (with ``--temporal_kind {l2,l1,charbonnier}``, default charbonnier, and ``--temporal_eps E``, default 1e-3): the
generator's loss gains G times the temporal-difference term of each prediction (losses.TemporalLoss: the distance between the
frame-to-frame differences of prediction and ground truth over the gap and its two known neighbours; one HIP launch per update writes the
losses and gradients of all predictions, each read in its own layout); printed lines gain ``G_temporal=`` (and ``G_temporal_forward=
G_temporal_backward=`` for TAI).  0 = off.

``--census_weight G``: the generator's loss gains G times the census (soft ternary) term of each prediction (losses.CensusLoss: per
pixel, how it relates to its 7x7 neighbours, compared between prediction and ground truth, so a brightness offset costs nothing; one HIP
launch per update writes the losses and gradients of all predictions, each read in its own layout); printed lines gain ``G_census=`` (and
``G_census_forward= G_census_backward=`` for TAI).  0 = off.

``--image_loss {l2,l1,charbonnier}`` (default ``l2`` = the reference's MSELoss + GDL, untouched): with ``l1`` or ``charbonnier``
(``--charbonnier_eps E``, default 1e-3) the pointwise term of alpha (Lp + GDL) becomes mean |d| or mean sqrt(d^2 + E^2) for every
prediction; Lp and GDL then come from losses.ImageLoss, one HIP launch per update for the losses and gradients of all predictions.  The
printed keys ``G_Lp= G_gdl=`` (``_forward``, ``_backward``) stay and carry the chosen terms.

``--aug_crop SMIN --aug_vflip --aug_brightness B --aug_contrast C --aug_gamma G --aug_flicker F`` (all off by default): training clips
are cropped to a random window, flipped top-bottom and changed photometrically per clip (and, with ``--aug_flicker``, per frame), by
draws that follow a clip's window, mirror and reversal draws (data.ClipAugment; include/tai_sepconv.h at tai_clip_from_frames_aug).  The
host path and ``--device_preprocess`` (one HIP launch, tai_clip_from_frames_aug) give the same bits; validation never augments; a
``--resumable`` run records the settings and refuses a continuation with others.  Printed lines do not change.

``--lr_D X`` gives the discriminator a base rate of its own (with or without ``--fused_step``).  ``--lr_schedule {constant,step,cosine}
--warmup_updates W --lr_decay_every E --lr_gamma g --lr_min_ratio r --weight_decay wd`` (all off by default, each needs ``--fused_step``):
the rate follows the schedule over the steps taken -- it is the fused step's scalar table (fused_step.scheduled_table), so a skipped step
does not advance it and it is saved with the optimizer state -- and the generator's weights (not its biases, not the discriminator) take
decoupled weight decay in the same launch (tai_fused_step_decay).  Printed lines gain ``lr_G= lr_D=`` with a schedule or a warm-up; a
``--resumable`` run records the settings and refuses a continuation with others (another ``--max_iter`` is another cosine).

  python train.py --name demo --K 5 --T 5 --F 5 --c_dim 1 --image_size 128 --batch_size 4 --model_key TAI_gray \
      --max_iter 10 --synthetic 64
"""
import os
import time

import numpy as np
import torch

import video_frame_inpainting_amd as vfi
from video_frame_inpainting_amd import clip_pipeline, fused_step, grad_guard, parallel, run_state, synthetic, tai
from video_frame_inpainting_amd.data import ClipAugment, ContiguousVideoClipDataset, ResumableBatchSampler
from video_frame_inpainting_amd.environments import create_training_environment
from video_frame_inpainting_amd.losses import LossSettings
from video_frame_inpainting_amd.options import TrainOptions
from video_frame_inpainting_amd.validation import Validator


def main(args=None):
    opt = TrainOptions().parse(args, allow_unknown=True)
    if opt.guard and opt.graph_step:
        raise SystemExit('--guard refuses --graph_step: a replayed update cannot leave out an optimizer step')
    if not opt.guard and opt.clip_grad_norm is not None:
        raise SystemExit('--clip_grad_norm needs --guard')
    if opt.fused_step and opt.graph_step:
        raise SystemExit('--fused_step refuses --graph_step: its tables and their copies do not belong inside a captured update')
    if opt.ema_decay is not None and not opt.fused_step:
        raise SystemExit('--ema_decay needs --fused_step: the average is kept by the fused optimizer step')
    if opt.ema_decay is not None and not 0.0 < opt.ema_decay < 1.0:
        raise SystemExit('--ema_decay must lie strictly between 0 and 1, found %r' % opt.ema_decay)
    schedule = fused_step.Schedule(opt.lr_schedule, opt.warmup_updates, opt.lr_decay_every, opt.lr_gamma, opt.lr_min_ratio)
    try:
        schedule.check()
        fused_step.check_weight_decay(opt.weight_decay)
    except ValueError as e:
        raise SystemExit(str(e))
    if not opt.fused_step and fused_step.needs_fused_step(schedule, opt.weight_decay):
        raise SystemExit(fused_step.needs_fused_step(schedule, opt.weight_decay))
    opt.schedule = schedule
    opt.losses = LossSettings.from_options(opt)
    try:
        opt.losses.check()
    except ValueError as e:
        raise SystemExit(str(e))
    if not opt.resumable:
        return _run(opt, None)
    if opt.graph_step and GRAPH_STEP_REFUSAL:
        raise SystemExit('--resumable refuses --graph_step: ' + GRAPH_STEP_REFUSAL)
    # the handlers only set a flag; the loop looks at it between updates.  Whatever was installed before is back when main returns.
    stop = run_state.StopRequest(opt.max_wall_minutes)
    stop.install()
    # a resumed run can only repeat the uninterrupted one if an update is a function of the state: no float atomics in any backward
    # (the replication padding's in ATen, MIOpen's weight gradients on the shapes the in-tree kernels leave to it)
    previous = (tai.set_reproducible_backward(True), torch.backends.cudnn.deterministic)
    torch.backends.cudnn.deterministic = True
    try:
        return _run(opt, stop)
    finally:
        tai.set_reproducible_backward(previous[0])
        torch.backends.cudnn.deterministic = previous[1]
        stop.uninstall()


GRAPH_STEP_REFUSAL = None       # a reason, if a replayed update were found to differ from an eager one


def _run(opt, stop):
    resumable = stop is not None
    if getattr(opt, 'miopen_find_mode', None):          # before the first convolution reaches MIOpen
        os.environ['MIOPEN_FIND_MODE'] = opt.miopen_find_mode
    vfi.configure_miopen()                              # FAST find mode unless set; one find-db / kernel cache per rank
    rank, world, local_rank = parallel.init_from_env()
    if getattr(opt, 'winograd_arithmetic', 'fp32') != 'fp32':
        from video_frame_inpainting_amd import conv_ops
        conv_ops.set_winograd_arithmetic(opt.winograd_arithmetic)
    device = torch.device('cuda', local_rank)
    torch.cuda.set_device(device)
    H, W = opt.image_size[0] + opt.padding_size[0], opt.image_size[1] + opt.padding_size[1]
    loader, augment = None, None
    if getattr(opt, 'train_video_list_path', None) and not opt.synthetic:
        # --device_preprocess: the workers hand over raw uint8 frames and the GPU builds the (bit-identical) clip tensor
        on_device = bool(getattr(opt, 'device_preprocess', False))
        augment = ClipAugment.from_options(opt)                      # the training dataset's alone; off = nothing is drawn
        dataset = ContiguousVideoClipDataset(opt.c_dim, opt.train_video_list_path, opt.K + opt.T + opt.F, not opt.no_backwards,
                                             not opt.no_flip, opt.image_size, True, opt.padding_size, seed=opt.seed + 7 * rank,
                                             raw=on_device, rank=rank, augment=augment)
        collate = clip_pipeline.collate_for(opt.num_threads) if on_device else None
        sampler = None
        if resumable:
            # a counter-based order: the draws of position j of epoch e come from (seed, rank, e, j), whichever worker serves it
            sampler = ResumableBatchSampler(len(dataset), opt.batch_size, opt.seed, rank, serial=opt.serial_batches)
            # (a generator of its own: every new iterator draws a base seed for its workers, which must not come out of the global
            # generator -- a run entered in the middle of an epoch makes one iterator more than the uninterrupted one)
            loader = torch.utils.data.DataLoader(dataset, batch_sampler=sampler, num_workers=opt.num_threads,
                                                 worker_init_fn=dataset.worker_init, collate_fn=collate,
                                                 generator=torch.Generator().manual_seed(opt.seed + 7 * rank))
        else:
            gen = torch.Generator().manual_seed(opt.seed + 7 * rank)
            loader = torch.utils.data.DataLoader(dataset, batch_size=opt.batch_size, shuffle=not opt.serial_batches,
                                                 num_workers=opt.num_threads, drop_last=True, generator=gen,
                                                 worker_init_fn=dataset.worker_init, collate_fn=collate)
        builder = clip_pipeline.DeviceClipBuilder(opt.c_dim, opt.image_size, opt.padding_size, device) if on_device else None
        print('# training videos = %d' % len(dataset))

        def batches():                                               # inf_data_loader (train.py:41)
            while True:
                for item in loader:
                    if sampler is not None:
                        sampler.took_batch()           # counts batches TAKEN (this generator runs on demand), not prefetched ones
                    yield builder.build(item) if on_device else item['targets']
        stream = batches()
    else:
        n_clips = opt.synthetic or 64
        clips = torch.from_numpy(synthetic.make_clips(n_clips, opt.K + opt.T + opt.F, opt.c_dim, H, W, opt.seed + rank))

    torch.manual_seed(0)
    np.random.seed(0)          # identical (K, T, F) draws on every rank
    model = vfi.create_model(opt.model_key)
    guard = grad_guard.GradGuard(opt.clip_grad_norm, opt.guard_patience) if opt.guard else None
    env = create_training_environment(model, opt.c_dim, opt.checkpoints_dir, opt.name, opt.K, opt.T, opt.F,
                                      opt.image_size, opt.alpha, opt.beta, opt.lr, opt.beta1, opt.df_dim, opt.Ip,
                                      opt.disc_window_size, opt.padding_size, device=device,
                                      graph_step=opt.graph_step, resumable=resumable, guard=guard, fused_step=opt.fused_step,
                                      ema_decay=opt.ema_decay, max_iter=opt.max_iter, losses=opt.losses,
                                      lr_D=opt.lr_D, lr_schedule=opt.schedule, weight_decay=opt.weight_decay)
    env.sync_replicas()
    total_updates = env.start_update
    # a resumed run starts from the best values its snapshot carries (train.py:96-97)
    validator = Validator(opt, (env.start_sum_avg_psnr_err, env.start_sum_avg_ssim_err))
    for leg in validator.legs:
        if rank == 0:
            print('# validation leg %s: (K,T,F)=(%d,%d,%d) on %s' % (leg.name, leg.K, leg.T, leg.F,
                                                                      '%d synthetic clips' % leg.source[1]
                                                                      if isinstance(leg.source, tuple) else leg.source))
    order = np.random.RandomState(opt.seed + 7 * rank)
    if resumable:
        if loader is not None:
            # (the augmentation settings are part of what a position yields; recorded only when augmentation is on)
            env.data_state_source = (lambda: dict(sampler.state(), augment=augment.state())) if augment.on else sampler.state
        else:
            env.data_state_source = lambda: {'kind': 'synthetic', 'n_clips': n_clips, 'batch_size': opt.batch_size, 'order': order.get_state()}
        if env.exact_resume:           # position the clip order where the snapshot left it (no draw from any other generator)
            saved, mine = env.restored_data_state, env.data_state_source()
            if saved is None or saved.get('kind') != mine['kind']:
                raise RuntimeError('the snapshot was written with another clip source (%r): it cannot be continued exactly'
                                   % (saved and saved.get('kind'),))
            if loader is not None:
                sampler.load_state(saved)
                augment.check_continues(saved.get('augment'))
            else:
                if (saved['n_clips'], saved['batch_size']) != (n_clips, opt.batch_size):
                    raise RuntimeError('the snapshot was written with --synthetic %d --batch_size %d: it cannot be continued exactly'
                                       % (saved['n_clips'], saved['batch_size']))
                order.set_state(run_state.numpy_state(saved['order']))
    try:
        while total_updates < opt.max_iter:
            t0 = time.time()
            total_updates += 1
            env.total_updates = total_updates
            K, T, F = env.sample_KTF(opt.sample_KTF)
            all_frames = next(stream) if loader is not None else clips[order.randint(0, n_clips, opt.batch_size)]
            env.K, env.T, env.F = K, T, F
            env.train()
            # set_train_inputs -> forward_train -> optimize_parameters; one hipGraph replay per update with --graph_step
            env.train_step(all_frames[:, :K], all_frames[:, K + T:K + T + F], all_frames[:, K:K + T])
            if total_updates % opt.print_freq == 0 or total_updates == 1:
                torch.cuda.synchronize()
                env.sync_guard(agree=True)         # (with --fused_step the verdicts were made on the device: read them for the line)
                errs = env.get_current_errors()
                state = ((env.fused.rates_suffix() if env.fused is not None else '') + (guard.log_suffix() if guard is not None else '')
                         + (' state=%016x' % run_state.digest(env) if resumable else ''))
                if rank == 0:
                    print('iter %d (K,T,F)=(%d,%d,%d) %.3fs  %s%s' % (total_updates, K, T, F, time.time() - t0,
                                                                      ' '.join('%s=%.5f' % kv for kv in sorted(errs.items())), state))
            if resumable and stop.agreed():
                # a save has to fit between SIGTERM and SIGKILL: no validation pass is started once the flag is up
                env.save('model_latest.ckpt', total_updates, *validator.best)
                if rank == 0:
                    print('Stop requested: model_latest.ckpt holds update %d' % total_updates)
                return
            if total_updates % opt.save_latest_freq == 0:
                env.save('model_latest.ckpt', total_updates, *validator.best)
                env.save('model_%08d.ckpt' % total_updates, total_updates, *validator.best)
            if validator and total_updates % opt.validate_freq == 0:
                validator.validate(env, total_updates)
        env.save('model_latest.ckpt', total_updates, *validator.best)
    except grad_guard.GuardGaveUp as e:
        # no snapshot on the way out: model_latest.ckpt is the last one written while the run was healthy.  (With --fused_step the
        # device gave up in an update that may lie a few behind the one whose read found it; the state has stood still since.)
        raise SystemExit('iter %d: the guard gives up: %s' % (total_updates - getattr(e, 'updates_ago', 0), e))
    print('Done.')


if __name__ == '__main__':
    main()
