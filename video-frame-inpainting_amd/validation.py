"""Periodic validation of the training driver (reference train.py:142-196, compute_errors at :237-287), without TensorBoard and the
visualisation grids.

Every ``--validate_freq`` updates up to three legs run, each on its own clip source:
  'T'    (K, T, F)          on --val_video_list_path
  'altT' (K, alt_T, F)      on --val_video_list_alt_T_path
  'altKF'(alt_K, T, alt_F)  on --val_video_list_alt_K_F_path
A leg runs when its source and the alt values it uses are given; ``--val_synthetic N`` replaces the lists by N seeded synthetic
clips (seed ``--seed`` + VAL_SEED_OFFSET: never the training clips).  Each leg runs the current weights (with ``--ema_decay``: the
averaged weights, exchanged into the parameters for the leg and out again; the line then ends with ``weights=ema``) without gradients
(``env.eval()`` + ``env.forward_test()``) and scores the frames with ``metrics.compute_errors_device``.  Only the first leg decides the
best snapshot: ``sum(mean(ssim, axis=0))`` strictly above the best so far saves ``model_best.ckpt``.

Data parallel: each rank scores its ``parallel.shard_slice`` of the clips and ``parallel.gather_rows`` puts the per-clip rows back in
clip order on every rank."""
import collections
import time

import numpy as np
import torch

from . import clip_pipeline, fused_step, metrics, parallel, synthetic

VAL_SEED_OFFSET = 104729          # validation clips: --seed + this (training clips use --seed + rank)

Leg = collections.namedtuple('Leg', 'name K T F source')     # source: a list path, or ('synthetic', n_clips)


def validation_legs(opt):
    """-> the legs that run, in the reference's order; [] when no validation source is given."""
    n_syn = getattr(opt, 'val_synthetic', 0) or 0
    src = lambda path: ('synthetic', n_syn) if n_syn > 0 else path
    legs = []
    if src(opt.val_video_list_path):
        legs.append(Leg('T', opt.K, opt.T, opt.F, src(opt.val_video_list_path)))
    if opt.alt_T is not None and src(opt.val_video_list_alt_T_path):
        legs.append(Leg('altT', opt.K, opt.alt_T, opt.F, src(opt.val_video_list_alt_T_path)))
    if opt.alt_K is not None and opt.alt_F is not None and src(opt.val_video_list_alt_K_F_path):
        legs.append(Leg('altKF', opt.alt_K, opt.T, opt.alt_F, src(opt.val_video_list_alt_K_F_path)))
    return legs


def sum_avg(table):
    """Sum over frame positions of the mean over clips (train.py:160-161)."""
    return float(np.sum(np.mean(table, axis=0)))


def update_best(best, sum_avg_psnr, sum_avg_ssim):
    """best = (psnr, ssim) sums of the best snapshot so far -> (new best, improved).  A snapshot is better only when its SSIM sum is
    strictly greater (train.py:162-166)."""
    if sum_avg_ssim > best[1]:
        return (sum_avg_psnr, sum_avg_ssim), True
    return best, False


def synthetic_clips(n_clips, K, T, F, c_dim, H, W, seed):
    return torch.from_numpy(synthetic.make_clips(n_clips, K + T + F, c_dim, H, W, seed + VAL_SEED_OFFSET))


def leg_batches(leg, opt, rank, world, cache=None):
    """-> (number of clips in the leg, iterator over this rank's [b, K+T+F, C, H, W] batches, clips in order, last batch ragged).
    ``cache`` (a dict) keeps a leg's synthetic clips from one pass to the next."""
    H, W = opt.image_size[0] + opt.padding_size[0], opt.image_size[1] + opt.padding_size[1]
    length = leg.K + leg.T + leg.F
    if isinstance(leg.source, tuple):
        n = leg.source[1]
        clips = cache.get(leg) if cache is not None else None
        if clips is None:
            clips = synthetic_clips(n, leg.K, leg.T, leg.F, opt.c_dim, H, W, opt.seed)[parallel.shard_slice(n, rank, world)]
            if cache is not None:
                cache[leg] = clips
        return n, (clips[i:i + opt.batch_size] for i in range(0, clips.shape[0], opt.batch_size))
    from .data import ContiguousVideoClipDataset
    on_device = bool(getattr(opt, 'device_preprocess', False))       # raw frames in, the clip tensor built on the GPU (same bits)
    # built afresh for every pass with a fixed seed: each validation scores the same windows
    dataset = ContiguousVideoClipDataset(opt.c_dim, leg.source, length, False, False, opt.image_size, False, opt.padding_size,
                                         seed=opt.seed + VAL_SEED_OFFSET, raw=on_device)
    n = len(dataset)
    mine = range(n)[parallel.shard_slice(n, rank, world)]
    loader = torch.utils.data.DataLoader(torch.utils.data.Subset(dataset, list(mine)), batch_size=opt.batch_size, shuffle=False,
                                         num_workers=opt.num_threads, drop_last=False,
                                         generator=torch.Generator().manual_seed(opt.seed + VAL_SEED_OFFSET),
                                         worker_init_fn=dataset.worker_init,
                                         collate_fn=clip_pipeline.collate_for(opt.num_threads) if on_device else None)
    if on_device:
        builder = clip_pipeline.DeviceClipBuilder(opt.c_dim, opt.image_size, opt.padding_size,
                                                  torch.device('cuda', torch.cuda.current_device()))
        return n, (builder.build(item) for item in loader)
    return n, (item['targets'] for item in loader)


def score(env, batches, K, T, F):
    """Run the environment's generator on every batch (no gradients) and score its middle frames -> (psnr, ssim, l2) rows
    [clips, T] in batch order."""
    rows = []
    for all_frames in batches:
        all_frames = all_frames.to(env.device, non_blocking=True)
        env.set_test_inputs(all_frames[:, :K], all_frames[:, K + T:K + T + F])
        env.K, env.T, env.F = K, T, F
        env.eval()
        env.forward_test()
        rows.append(np.stack(metrics.compute_errors_device(env.gen_output['pred'], all_frames[:, K:K + T]), axis=1))
    return np.concatenate(rows, axis=0) if rows else np.zeros((0, 3, T))


def run_leg(env, leg, opt, rank=None, world=None, cache=None):
    """One validation leg -> (psnr, ssim, l2) tables [n_clips, leg.T], identical on every rank."""
    rank = parallel.rank() if rank is None else rank
    world = parallel.world_size() if world is None else world
    n, batches = leg_batches(leg, opt, rank, world, cache)
    table = parallel.gather_rows(score(env, batches, leg.K, leg.T, leg.F), n)
    return table[:, 0], table[:, 1], table[:, 2]


class Validator(object):
    """Runs the legs of ``opt`` and keeps the best-snapshot bookkeeping of train.py:142-196."""

    def __init__(self, opt, start_best=(0, 0)):
        self.opt = opt
        self.legs = validation_legs(opt)
        self.best = tuple(start_best)
        self._clips = {}

    def __bool__(self):
        return bool(self.legs)

    def validate(self, env, total_updates, log=print):
        """All legs; saves model_best.ckpt when the first leg improves.  -> {leg name: (psnr, ssim, l2)}."""
        results = {}
        if getattr(env, 'sync_guard', None) is not None:
            env.sync_guard(agree=True)         # a fused step's verdicts: read before anything is scored or saved
        for i, leg in enumerate(self.legs):
            t0 = time.time()
            # with a weight average (train.py --ema_decay) the averaged weights are the ones scored, and model_best.ckpt is chosen by them
            with fused_step.averaged_weights(env) as scored:
                psnr, ssim, l2 = run_leg(env, leg, self.opt, cache=self._clips)
            results[leg.name] = (psnr, ssim, l2)
            if parallel.rank() == 0:
                log('Validation (T=%d) done. Took %.03f minutes' % (leg.T, (time.time() - t0) / 60))
                log('val %s (K,T,F)=(%d,%d,%d) clips=%d psnr=%.5f ssim=%.5f l2=%.6f sum_avg_psnr=%r sum_avg_ssim=%r%s'
                    % (leg.name, leg.K, leg.T, leg.F, psnr.shape[0], float(np.mean(psnr)), float(np.mean(ssim)),
                       float(np.mean(l2)), sum_avg(psnr), sum_avg(ssim), ' weights=ema' if scored.active else ''))
            if i == 0:
                self.best, improved = update_best(self.best, sum_avg(psnr), sum_avg(ssim))
                if improved:
                    if parallel.rank() == 0:
                        log('Current model has best SSIM, saving...')
                    env.save('model_best.ckpt', total_updates, self.best[0], self.best[1])
        return results
