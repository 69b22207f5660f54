"""argparse flag system of the path (reference src/options/options.py:6-209): same flag names, defaults and
post-processing (image_size / padding_size widened to two-element lists, :54-58; ``assert torch.cuda.is_available()``,
:61).  Flags that only configure the reference's other model families (transformer teacher forcing, SloMo weights) and
the video-list paths of the real datasets are accepted where the reference requires them but are optional here: the
configs of this build run on synthetic clips (``--synthetic`` is the one added flag)."""
import argparse

import torch


class BaseOptions(object):
    def __init__(self):
        self.parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
        g = self.parser.add_argument_group('Experiment parameters')
        g.add_argument('--name', type=str, default='experiment_name', help='Name of the experiment')
        g = self.parser.add_argument_group('Model input/output parameters')
        g.add_argument('--K', type=int, required=True, help='Length of the preceding sequence (in frames)')
        g.add_argument('--T', type=int, required=True, help='Length of the middle sequence (in frames)')
        g.add_argument('--F', type=int, required=True, help='Length of the following sequence (in frames)')
        g.add_argument('--batch_size', type=int, default=4, help='Mini-batch size')
        g.add_argument('--image_size', type=int, nargs='+', default=[128], help='Image size (H x W); one number means H = W')
        g.add_argument('--padding_size', type=int, nargs='+', default=[0],
                       help='Padding added to the bottom and right sides of the image; one number means both')
        g.add_argument('--c_dim', type=int, default=3, help='Number of channels in the image input')
        g = self.parser.add_argument_group('Model specification parameters')
        g.add_argument('--model_key', type=str, required=True, help='Key identifying the generator to create')
        g = self.parser.add_argument_group('Directory parameters')
        g.add_argument('--checkpoints_dir', type=str, default='checkpoints', help='Path to store/load checkpoint files')
        g = self.parser.add_argument_group('Common data loading parameters')
        g.add_argument('--num_threads', type=int, default=2, help='Number of threads used to load data')
        g.add_argument('--synthetic', type=int, default=0, metavar='N_CLIPS',
                       help='(this build) run on N seeded synthetic clips instead of a video list')
        g.add_argument('--seed', type=int, default=1002, help='(this build) seed of the synthetic clips')
        g.add_argument('--device_preprocess', action='store_true',
                       help='(this build) build clips on the GPU from raw decoded frames (clip_pipeline.py: resize, BGR, flip, padding, '
                            'range map and gray in one HIP launch per batch; PNG pixels and PSNR / SSIM on the GPU in predict.py), '
                            'bit-equal to the host path; off = the host path, unchanged.  Ignored with --synthetic.  A clip window '
                            'inside a span longer than K + T + F is a seeded draw: with --num_threads 0 the flag reproduces the '
                            "default path's windows, with workers each worker draws from its own copy of the generator")
        g.add_argument('--winograd_arithmetic', type=str, default='fp32', choices=['fp32', 'bf16x3'],
                       help='(this build) arithmetic of the 3x3 Winograd GEMMs: fp32 = the fp32 MFMA (default, the arithmetic every '
                            'parity statement is made on); bf16x3 = opt-in split bf16 (three bf16 terms per operand, six products, '
                            'fp32 accumulation: error at or below the fp32 form, 3-25 %% faster per layer)')

        g.add_argument('--winograd_tile', type=int, default=4, choices=[2, 4],
                       help='(this build) output tile of the 3x3 Winograd convolutions at inference: 4 = F(4x4,3x3) on the layers with at least '
                            "128 input and output channels (default: 1.78x fewer MFMAs there, the forward's end-to-end error unchanged, ~3 %% "
                            'faster at 32 clips) and F(2x2,3x3) elsewhere; 2 = F(2x2,3x3) on every layer')

    def parse(self, args=None, allow_unknown=False, require_gpu=True):
        if allow_unknown:
            opt, unknown_opt = self.parser.parse_known_args(args)
            print('Ignored arguments: %s' % str(unknown_opt))
        else:
            opt = self.parser.parse_args(args)
        if len(opt.image_size) == 1:
            opt.image_size.append(opt.image_size[0])
        if len(opt.padding_size) == 1:
            opt.padding_size.append(opt.padding_size[0])
        if require_gpu:
            assert torch.cuda.is_available()      # options.py:61: the path has no CPU implementation
        return opt


class TrainOptions(BaseOptions):
    def __init__(self):
        super().__init__()
        g = self.parser.add_argument_group('Optimization parameters')
        g.add_argument('--lr', type=float, default=0.0001, help='Base learning rate')
        g.add_argument('--beta1', type=float, default=0.5, help='Momentum term of adam')
        g.add_argument('--max_iter', type=int, default=100000, help='Maximum number of iterations (batches) to train on')
        g = self.parser.add_argument_group('Loss parameters')
        g.add_argument('--alpha', type=float, default=1.0, help='Image loss weight')
        g.add_argument('--beta', type=float, default=0.02, help='GAN loss weight')
        g = self.parser.add_argument_group('Training frequency parameters')
        g.add_argument('--print_freq', type=int, default=100)
        g.add_argument('--save_latest_freq', type=int, default=1000)
        g.add_argument('--validate_freq', type=int, default=10000)
        g = self.parser.add_argument_group('Adversarial training parameters')
        g.add_argument('--df_dim', type=int, default=64, help='Number of filters in first conv layer of the discriminator')
        g.add_argument('--Ip', type=int, default=3, help='Power iterations of the spectral-normalized discriminator')
        g.add_argument('--disc_window_size', type=int, default=3, help='Frames the discriminator sees at a time')
        g = self.parser.add_argument_group('Training data loading parameters')
        g.add_argument('--alt_K', type=int, default=None)
        g.add_argument('--alt_T', type=int, default=None)
        g.add_argument('--alt_F', type=int, default=None)
        for name in ('train_video_list_path', 'val_video_list_path', 'val_video_list_alt_T_path',
                     'val_video_list_alt_K_F_path', 'vis_video_list_path', 'vis_video_list_alt_T_path',
                     'vis_video_list_alt_K_F_path'):
            g.add_argument('--' + name, type=str, default=None)
        g.add_argument('--val_synthetic', type=int, default=0, metavar='N_CLIPS',
                       help='(this build) validate on N seeded synthetic clips (a seed other than the training clips\') instead of '
                            'the --val_video_list* lists: every --validate_freq updates, the (K, T, F) leg, the (K, alt_T, F) leg when '
                            '--alt_T is given and the (alt_K, T, alt_F) leg when --alt_K and --alt_F are')
        g.add_argument('--serial_batches', action='store_true')
        g.add_argument('--no_backwards', action='store_true')
        g.add_argument('--no_flip', action='store_true')
        g.add_argument('--sample_KTF', action='store_true',
                       help='Sample the number of preceding, middle, and following frames in each minibatch')
        g.add_argument('--graph_step', action='store_true',
                       help='Capture one whole update as a hipGraph per (K, T, F) and replay it (one process per node only)')
        g.add_argument('--resumable', action='store_true',
                       help='(this build) exact resume: snapshots carry run_state (spectral-norm vectors, every generator state, the clip '
                            "order's position, a state digest computed on the GPU) and a run stopped after any update and continued in a new "
                            'process ends with the same bits as the uninterrupted one; the clip order becomes a counter-based one (the draws '
                            'of a position depend on (seed, rank, epoch, position) only, not on --num_threads); SIGTERM, SIGINT and '
                            '--max_wall_minutes end the run after the update in flight with model_latest.ckpt written; the previous '
                            'model_latest.ckpt is kept as model_latest.prev.ckpt and a start falls back to it when the latest one does not '
                            'load or does not match its digest; printed lines end with state=<digest>.  Off = the run as before')
        g.add_argument('--guard', action='store_true',
                       help='(this build) look at the gradients between each backward pass and its optimizer step (grad_guard.py, one HIP '
                            'launch per optimizer: tai_grad_stats): an optimizer whose gradients hold a NaN or an Inf does not step in that '
                            'update (weights, Adam moments and step counter stay as they were), a snapshot whose state holds one is not '
                            'written, and printed lines gain gnorm_G= gnorm_D= skipped=.  Refuses --graph_step.  Off = the update as before')
        g.add_argument('--clip_grad_norm', type=float, default=None, metavar='X',
                       help="(this build, with --guard) scale the generator's and the discriminator's gradients, each as a whole, to an "
                            'L2 norm of at most X before the step (the norm is a fixed-order float64 sum, so a clipped --resumable run '
                            'stays bit-exact)')
        g.add_argument('--guard_patience', type=int, default=8, metavar='N',
                       help='(this build, with --guard) end the run with an error, writing no snapshot, after N consecutive updates in '
                            'which a step was skipped')
        g.add_argument('--fused_step', action='store_true',
                       help='(this build) both optimizers step through one HIP launch each (fused_step.py: tai_step_verdict + tai_fused_step): clip '
                            'scaling, the Adam update and the weight average, on a verdict (ok / clipped / skipped) that stays on the device, so '
                            'the host does not wait between backward() and the step; with --guard its counters live on the device and are read '
                            'at printed lines, validation and saves.  The arithmetic is a written definition (include/tai_sepconv.h), close to '
                            "but not bit-equal with torch.optim.Adam's.  Refuses --graph_step.  Off = optimizer.step() as before")
        g.add_argument('--ema_decay', type=float, default=None, metavar='d',
                       help="(this build, with --fused_step) keep an exponential moving average of the generator's weights, "
                            'e <- e + (1 - d)(p - e) after every step, 0 < d < 1: snapshots gain generator_ema, validation scores the '
                            'averaged weights and model_best.ckpt is chosen by them (predict.py --weights ema)')
        g.add_argument('--lr_D', type=float, default=None, metavar='X',
                       help="(this build) the discriminator's base learning rate; default: --lr.  Works with or without --fused_step")
        g.add_argument('--lr_schedule', type=str, default='constant', choices=['constant', 'step', 'cosine'],
                       help='(this build, with --fused_step) the learning rate over the steps TAKEN (a skipped step does not advance it), '
                            'for both optimizers: constant (default), step = x --lr_gamma every --lr_decay_every steps, cosine = from the '
                            'base rate down to --lr_min_ratio of it at --max_iter.  The schedule is the fused step\'s scalar table '
                            '(include/tai_sepconv.h); printed lines gain lr_G= lr_D=')
        g.add_argument('--warmup_updates', type=int, default=0, metavar='W',
                       help='(this build, with --fused_step) the rate rises linearly over the first W steps, t / W of the base rate at step t')
        g.add_argument('--lr_decay_every', type=int, default=10000, metavar='E', help='(with --lr_schedule step) steps between two decays; >= 1')
        g.add_argument('--lr_gamma', type=float, default=0.5, metavar='g', help='(with --lr_schedule step) the factor of a decay; 0 <= g <= 1')
        g.add_argument('--lr_min_ratio', type=float, default=0.01, metavar='r',
                       help='(with --lr_schedule cosine) the final rate over the base rate; 0 <= r <= 1')
        g.add_argument('--weight_decay', type=float, default=0.0, metavar='wd',
                       help="(this build, with --fused_step) decoupled weight decay (AdamW), p <- p - lr wd p in front of the Adam update, for "
                            "the generator's parameters with two or more dimensions (convolution and ConvLSTM weights): never a bias, never "
                            'the discriminator, whose weights are spectrally normalised.  One HIP launch, tai_fused_step_decay.  0 = off')
        g.add_argument('--ssim_weight', type=float, default=0.0, metavar='G',
                       help="(this build) add G (1 - mean SSIM) of every prediction against the ground truth to the generator's loss "
                            '(losses.SSIMLoss: 7x7 window, float frames in [0, 1] with L = 1, unclipped, float64 window arithmetic; loss and '
                            'gradient from one HIP launch, tai_ssim_loss); printed lines gain G_ssim= (TAI: G_ssim_forward= G_ssim_backward= '
                            'as well).  0 (default) = the loss as before: nothing is launched, no key is added')
        g.add_argument('--lap_weight', type=float, default=0.0, metavar='G',
                       help="(this build) add G times the Laplacian-pyramid L1 distance of every prediction to the ground truth to the "
                            "generator's loss (losses.LapLoss: 5-tap binomial pyramid of --lap_levels levels on float frames in [0, 1], "
                            'unclipped, level l weighted 2^l, float64 arithmetic; loss and gradient from one HIP launch, tai_lap_loss); '
                            'printed lines gain G_lap= (TAI: G_lap_forward= G_lap_backward= as well).  0 (default) = the loss as before: '
                            'nothing is launched, no key is added')
        g.add_argument('--lap_levels', type=int, default=5, metavar='L',
                       help='(this build, with --lap_weight) levels of the pyramid, 1..6; the frames must be at least 2^(L-1) pixels each way')
        g.add_argument('--image_loss', type=str, default='l2', choices=['l2', 'l1', 'charbonnier'],
                       help="(this build) the pointwise term of the generator's image loss alpha (Lp + GDL), applied to every prediction: "
                            'l2 (default) = the reference\'s MSELoss + GDL modules, untouched; l1 = mean |d|; charbonnier = mean '
                            'sqrt(d^2 + eps^2) (--charbonnier_eps), d the difference of the frames in [0, 1].  l1 / charbonnier take Lp and '
                            'GDL from losses.ImageLoss: one HIP launch (tai_image_loss) writes the losses and gradients of all predictions '
                            'of an update on the model\'s own layout; the printed keys G_Lp= G_gdl= (_forward, _backward) carry the chosen terms')
        g.add_argument('--charbonnier_eps', type=float, default=1e-3, metavar='E',
                       help='(this build, with --image_loss charbonnier) the eps of sqrt(d^2 + eps^2); finite and > 0')
        g.add_argument('--temporal_weight', type=float, default=0.0, metavar='G',
                       help="(this build) add G times the temporal-difference term of every prediction to the generator's loss "
                            '(losses.TemporalLoss: the frame-to-frame difference of the error over the gap, the error taken as zero on the '
                            'known frames on both sides, so flicker and the two seams are penalised and a constant error is not counted '
                            'again; float frames in [0, 1], unclipped; losses and gradients of all predictions from one HIP launch, '
                            'tai_temporal_loss, on the model\'s own layouts); printed lines gain G_temporal= (TAI: G_temporal_forward= '
                            'G_temporal_backward= as well).  0 (default) = the loss as before: nothing is launched, no key is added')
        g.add_argument('--temporal_kind', type=str, default='charbonnier', choices=['l2', 'l1', 'charbonnier'],
                       help='(this build, with --temporal_weight) the distance on the temporal difference d: l2 = d^2, l1 = |d|, '
                            'charbonnier (default) = sqrt(d^2 + eps^2) (--temporal_eps)')
        g.add_argument('--temporal_eps', type=float, default=1e-3, metavar='E',
                       help='(this build, with --temporal_kind charbonnier) the eps of sqrt(d^2 + eps^2); finite and > 0')
        g.add_argument('--census_weight', type=float, default=0.0, metavar='G',
                       help="(this build) add G times the census (soft ternary) term of every prediction to the generator's loss "
                            '(losses.CensusLoss: per pixel, the softened signs of its differences to the 48 neighbours of its 7x7 window, '
                            'compared between prediction and ground truth on gray frames in [0, 1], unclipped, so a brightness offset '
                            'costs nothing; losses and gradients of all predictions from one HIP launch, tai_census_loss, on the '
                            'model\'s own layouts); printed lines gain G_census= (TAI: G_census_forward= G_census_backward= as well).  '
                            '0 (default) = the loss as before: nothing is launched, no key is added')
        g.add_argument('--max_wall_minutes', type=float, default=None, metavar='M',
                       help='(this build, with --resumable) stop as after SIGTERM once the run has lasted M minutes')
        g.add_argument('--miopen_find_mode', type=str, default=None, choices=['NORMAL', 'FAST', 'HYBRID', 'DYNAMIC_HYBRID'],
                       help='MIOPEN_FIND_MODE for this run (package default FAST: first update 1.4 s instead of 22 s, later updates '
                            '2-3 %% slower; NORMAL pays the search once and is the choice for a long run)')
        g = self.parser.add_argument_group('Training augmentation parameters (this build; training clips only -- validation legs and '
                                           'predict.py never augment; host path and --device_preprocess give the same bits; with every '
                                           'flag at its default nothing is drawn or launched)')
        g.add_argument('--aug_crop', type=float, default=1.0, metavar='SMIN',
                       help='per clip, resize a random window of the source frame instead of the whole frame: its side is a uniform share '
                            'in [SMIN, 1] of the frame, the same window for all frames of the clip; SMIN in (0, 1], 1 = off')
        g.add_argument('--aug_vflip', action='store_true', help='per clip, flip top-bottom with probability 1/2')
        g.add_argument('--aug_brightness', type=float, default=0.0, metavar='B',
                       help='per clip, an additive offset uniform in [-B, B] on the [0, 1] scale; 0 <= B < 1')
        g.add_argument('--aug_contrast', type=float, default=0.0, metavar='C',
                       help='per clip, a gain uniform in [1 - C, 1 + C] about 0.5; 0 <= C < 1')
        g.add_argument('--aug_gamma', type=float, default=0.0, metavar='G',
                       help='per clip, gamma = (1 + G)^u with u uniform in [-1, 1]; G >= 0')
        g.add_argument('--aug_flicker', type=float, default=0.0, metavar='F',
                       help='per FRAME, a further additive offset uniform in [-F, F]: the exposure difference between frames that the '
                            'census term (--census_weight) does not charge; 0 <= F < 1')
        g = self.parser.add_argument_group('Training visualization parameters')
        g.add_argument('--tensorboard_dir', type=str, default='tb')

    def parse(self, args=None, allow_unknown=False, require_gpu=True):
        opt = super().parse(args, allow_unknown, require_gpu)
        from .data import ClipAugment
        try:                                   # an augmentation setting outside its range is refused here, with the flag named
            ClipAugment.from_options(opt)
        except ValueError as e:
            self.parser.error(str(e))
        return opt


class TestOptions(BaseOptions):
    def __init__(self):
        super().__init__()
        g = self.parser.add_argument_group('Test data loading parameters')
        g.add_argument('--test_video_list_path', type=str, default=None,
                       help='The path to the text file containing the list of test video (clips)')
        g.add_argument('--disjoint_clips', action='store_true')
        g = self.parser.add_argument_group('Snapshot parameters')
        g.add_argument('--snapshot_file_name', type=str, default='model_best.ckpt')
        g = self.parser.add_argument_group('Qualitative result destination parameters')
        g.add_argument('--qual_result_root', type=str, required=True,
                       help='The root path where qualitative results will be stored')
        g = self.parser.add_argument_group('Output parameters')
        g.add_argument('--intermediate_preds', action='store_true',
                       help='Flag to write intermediate predictions in addition to final ones')
        g.add_argument('--random_init', action='store_true',
                       help='(this build) skip the snapshot load and keep the seeded xavier initialisation')
        g.add_argument('--weights', type=str, default='raw', choices=['raw', 'ema'],
                       help="(this build) which weights of the snapshot to run: raw = its generator (default), ema = its generator_ema, "
                            'the weight average a run with train.py --ema_decay keeps')
        g.add_argument('--conv_precision', type=str, default='fp32', choices=['fp32', 'bf16'],
                       help='(this build) precision of the inference convolutions: fp32 (default) or bf16 = opt-in: the layers with at '
                            'least 16 input and output channels and k in {3, 5, 7} take bf16 operands (rounded to nearest even), exact '
                            'products and fp32 sums (conv_ops.set_conv_precision)')


class RestoreOptions(BaseOptions):
    """restore.py: the model and snapshot flags of TestOptions, and what the repair of one damaged video needs."""

    def __init__(self):
        super().__init__()
        g = self.parser.add_argument_group('Snapshot parameters')
        g.add_argument('--snapshot_file_name', type=str, default='model_best.ckpt')
        g.add_argument('--random_init', action='store_true', help='skip the snapshot load and keep the seeded xavier initialisation')
        g.add_argument('--weights', type=str, default='raw', choices=['raw', 'ema'],
                       help="which weights of the snapshot to run: raw = its generator (default), ema = its generator_ema")
        g.add_argument('--conv_precision', type=str, default='fp32', choices=['fp32', 'bf16'],
                       help='precision of the inference convolutions (as predict.py)')
        g = self.parser.add_argument_group('Restoration parameters')
        g.add_argument('--input', type=str, required=True,
                       help='the damaged video: a directory of frame images (names that all end in a number are indexed by that number, '
                            'absent numbers are missing frames), an AVI (zero-length chunks are missing frames), a .npy / .npz frame array')
        g.add_argument('--output_dir', type=str, required=True, help='where frame_%%06d.png and report.json are written')
        g.add_argument('--detect', type=str, default='missing',
                       help='comma-separated detectors out of missing,dup,blank (or none).  missing = the source has no such frame; '
                            'dup = at most --dup_share of the bytes differ from the previous frame by more than --dup_tol (defaults: an '
                            'exact repeat, the signature of a dropped frame -- note that this flags EVERY frame of a static scene, by '
                            'definition); blank = the variance of the frame is at most --blank_var (default: a constant frame)')
        g.add_argument('--gaps', type=str, default='', metavar='a-b,c-d',
                       help='frames to treat as damaged whatever the detectors say (0-based, inclusive)')
        g.add_argument('--dup_tol', type=int, default=0, help='(dup) a byte differs when it moved by more than this; 0..254')
        g.add_argument('--dup_share', type=float, default=0.0, help='(dup) share of the bytes that may differ in a repeat; 0..1')
        g.add_argument('--blank_var', type=float, default=0.0, help='(blank) largest variance, in squared grey levels, of a blank frame')
        g.add_argument('--max_T', type=int, default=None, help='longest gap that is filled; default --T')
        g.add_argument('--chunk_frames', type=int, default=256, help='frames decoded, uploaded and scanned at a time')
        g.add_argument('--dry_run', action='store_true', help='scan, plan and write report.json only; needs no GPU')
        g = self.parser.add_argument_group('Partly damaged frames (off unless --detect_blocks or --damage_map is given)')
        g.add_argument('--detect_blocks', type=str, default='',
                       help='comma-separated block detectors out of dup,blank (or none; default: off).  Per block of --block_size source '
                            'pixels: blank = the variance of the block is at most --block_blank_var (default: a constant block, what a '
                            'decoder paints); dup = at most --block_dup_share of the block\'s bytes differ from the same block of the '
                            'previous frame by more than --dup_tol (default: an exact repeat, what concealment by copying leaves).  A '
                            'flagged block counts as damage only in a run of at most --max_T frames that touches neither the first nor '
                            'the last frame: letterbox bars and static backgrounds are flagged in long runs and are content, by '
                            'definition.  Neither detector sees noisy damage or damage that fills only part of a block; a block that '
                            'really is constant or still for a few frames IS flagged')
        g.add_argument('--block_size', type=int, default=16, choices=[8, 16, 32], help='block size in SOURCE pixels')
        g.add_argument('--feather', type=int, default=4,
                       help='width in model pixels of the ramp between the prediction and the kept pixels; 0..15, 0 = a hard replace')
        g.add_argument('--block_share', type=float, default=0.5,
                       help='a frame with more than this share of its blocks damaged is replaced whole, like any gap frame; 0..1')
        g.add_argument('--block_dup_share', type=float, default=0.0, help='(block dup) share of a block\'s bytes that may differ; 0..1')
        g.add_argument('--block_blank_var', type=float, default=0.0, help='(block blank) largest variance of a blank block')
        g.add_argument('--damage_map', type=str, default=None, metavar='FILE.npy',
                       help='uint8 or bool [n_frames, Bh, Bw], non-zero = damaged: blocks to treat as damaged whatever the detectors '
                            'say (not filtered by the run rule, as --gaps is not)')
