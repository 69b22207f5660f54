"""Evaluation and training environments of the bi-TAI path (reference src/environments/environments.py:55-485).

Same object protocol as the reference so ``predict.py`` / ``train.py``-style drivers read the same:
  eval:   env = create_eval_environment(model, checkpoints_dir, name, snapshot_file_name, padding_size)
          env.set_test_inputs(P, F); env.T = T; env.eval(); env.forward_test(); env.gen_output['pred']
  train:  env = create_training_environment(...); env.set_train_inputs(P, F, GT); env.K, env.T, env.F = ...
          env.train(); env.forward_train(); env.optimize_parameters(); env.get_current_errors()
Checkpoints keep the reference's dict layout {updates, sum_avg_psnr_err, sum_avg_ssim_err, generator, optimizer_G,
discriminator, optimizer_D} (environments.py:178-194, 290-297); evaluation loads ``snapshot['generator']`` only (:113).

What differs (same arithmetic):
  * no ``Variable`` / ``volatile``: inference runs under ``torch.no_grad()`` and, with ``use_graph=True``, as a replayed
    hipGraph (graph.py) keyed by the input shapes;
  * the device is explicit, so one process per GPU can own ``cuda:LOCAL_RANK``;
  * ``optimize_parameters`` all-reduces generator and discriminator gradients across data-parallel ranks (parallel.py)
    right after each backward, in the reference's G-then-D order; with one process it is the reference's step.
"""
import os

import numpy as np
import torch

from . import conv_ops, parallel, run_state
from . import fused_step as fused_step_module
from .graph import GraphedForward
from .losses import GDL, IMAGE_LOSS_KINDS, CensusLoss, ImageLoss, LapLoss, SSIMLoss, TemporalLoss
from .mcnet import MCNetFillInModel
from .sn_discriminator import SNDiscriminator
from .ablations import (BidirectionalSimpleAverageFillInModel, BidirectionalTimeWeightedAverageFillInModel,
                        TimeWeightedInterpolationFillInModel, TimeWeightedPFFillInModel)
from .tai import TAIFillInModel
from .util import inverse_transform, move_to_devices, weights_init


def create_eval_environment(fill_in_model, checkpoints_dir, name, snapshot_file_name, padding_size, device=None,
                            load_snapshot=True, use_graph=False, weights='raw'):
    env = BaseVideoFillInEnvironment(fill_in_model, checkpoints_dir, name, padding_size, device=device,
                                     use_graph=use_graph)
    env.weights = weights          # 'ema': the snapshot's generator_ema (train.py --ema_decay) instead of its generator
    if load_snapshot and not isinstance(fill_in_model, TimeWeightedPFFillInModel):   # environments.py:57-58
        env.load(snapshot_file_name)
    print('Loaded evaluation environment')
    return env


def create_training_environment(fill_in_model, c_dim, checkpoints_dir, name, max_K, max_T, max_F, image_size, alpha,
                                beta, lr, beta1, df_dim, Ip, disc_window_size, padding_size, device=None, graph_step=False,
                                resumable=False, guard=None, fused_step=False, ema_decay=None, max_iter=100000, ssim_weight=0.0,
                                image_loss='l2', charbonnier_eps=1e-3, lap_weight=0.0, lap_levels=5, temporal_weight=0.0,
                                temporal_kind='charbonnier', temporal_eps=1e-3, census_weight=0.0, lr_D=None, lr_schedule=None,
                                weight_decay=0.0):
    if not ssim_weight >= 0.0:
        raise ValueError('ssim_weight must not be negative, found %r' % (ssim_weight,))
    if not lap_weight >= 0.0:
        raise ValueError('lap_weight must not be negative, found %r' % (lap_weight,))
    if image_loss not in IMAGE_LOSS_KINDS:
        raise ValueError('image_loss must be one of %s, found %r' % (', '.join(IMAGE_LOSS_KINDS), image_loss))
    if not (charbonnier_eps > 0.0 and charbonnier_eps != float('inf')):
        raise ValueError('charbonnier_eps must be finite and > 0, found %r' % (charbonnier_eps,))
    if not temporal_weight >= 0.0:
        raise ValueError('temporal_weight must not be negative, found %r' % (temporal_weight,))
    if temporal_kind not in IMAGE_LOSS_KINDS:
        raise ValueError('temporal_kind must be one of %s, found %r' % (', '.join(IMAGE_LOSS_KINDS), temporal_kind))
    if not (temporal_eps > 0.0 and temporal_eps != float('inf')):
        raise ValueError('temporal_eps must be finite and > 0, found %r' % (temporal_eps,))
    if not (census_weight >= 0.0 and census_weight != float('inf')):
        raise ValueError('census_weight must be finite and not negative, found %r' % (census_weight,))
    if guard is not None and graph_step:
        raise ValueError('a guarded update cannot be a captured one: a replayed update cannot leave out an optimizer step')
    if fused_step and graph_step:
        raise ValueError('a fused step cannot be part of a captured update: its tables and their copies do not belong inside a capture')
    if ema_decay is not None and not fused_step:
        raise ValueError('--ema_decay needs --fused_step: the average is kept by the fused optimizer step')
    fused_step_module.check_ema_decay(ema_decay)
    # lr_schedule: a fused_step.Schedule (train.py --lr_schedule --warmup_updates --lr_decay_every --lr_gamma --lr_min_ratio) or None
    (lr_schedule or fused_step_module.Schedule()).check()
    fused_step_module.check_weight_decay(weight_decay)
    if not fused_step and fused_step_module.needs_fused_step(lr_schedule, weight_decay):
        raise ValueError(fused_step_module.needs_fused_step(lr_schedule, weight_decay))
    if isinstance(fill_in_model, (TAIFillInModel, TimeWeightedInterpolationFillInModel,
                                  BidirectionalSimpleAverageFillInModel, BidirectionalTimeWeightedAverageFillInModel)):
        env = TAITrainingEnvironment(      # environments.py:29-31
            fill_in_model, checkpoints_dir, name, image_size, c_dim, alpha, beta, lr, beta1,
                                     df_dim, Ip, disc_window_size, max_K, max_T, max_F, padding_size, device=device,
                                     graph_step=graph_step, ssim_weight=ssim_weight, image_loss=image_loss,
                                     charbonnier_eps=charbonnier_eps, lap_weight=lap_weight, lap_levels=lap_levels,
                                     temporal_weight=temporal_weight, temporal_kind=temporal_kind, temporal_eps=temporal_eps,
                                     census_weight=census_weight)
    elif isinstance(fill_in_model, MCNetFillInModel):
        env = MCNetTrainingEnvironment(fill_in_model, checkpoints_dir, name, image_size, c_dim, alpha, beta, lr, beta1,
                                       df_dim, Ip, disc_window_size, max_K, max_T, max_F, padding_size, device=device,
                                       graph_step=graph_step, ssim_weight=ssim_weight, image_loss=image_loss,
                                     charbonnier_eps=charbonnier_eps, lap_weight=lap_weight, lap_levels=lap_levels,
                                     temporal_weight=temporal_weight, temporal_kind=temporal_kind, temporal_eps=temporal_eps,
                                     census_weight=census_weight)
    else:
        raise RuntimeError('Tried to create a training environment for object of unsupported type %s'
                           % type(fill_in_model).__name__)
    env.resumable = bool(resumable)
    env.guard = guard
    if lr_D is not None and hasattr(env, 'optimizer_D'):      # only another number handed to the second optimizer
        env.optimizer_D.param_groups[0]['lr'] = float(lr_D)
    if fused_step:
        env.fused = fused_step_module.FusedStep(env.device, max_iter, guard=guard, ema_decay=ema_decay, schedule=lr_schedule,
                                                weight_decay=weight_decay)
        env.fused.attach('G', env.generator, env.optimizer_G)
        if hasattr(env, 'optimizer_D'):
            env.fused.attach('D', env.discriminator, env.optimizer_D)
    remove_stale_temporaries(env.save_dir)
    names = [n for n in (LATEST, PREVIOUS if env.resumable else None) if n and os.path.isfile(os.path.join(env.save_dir, n))]
    for i, file_name in enumerate(names):
        print('Loading latest snapshot...')
        try:
            env.load(file_name)
            break
        except Exception as e:
            # a truncated file (a process killed inside a save before saves were atomic, a full disk) or a state that does not
            # hash to the digest it was saved with: the snapshot before it is the one to continue from
            if not env.resumable or i + 1 == len(names):
                raise
            print('%s cannot be used (%s: %s): falling back to %s' % (file_name, type(e).__name__, e, names[i + 1]))
    print('Loaded training environment')
    return env


LATEST, PREVIOUS = 'model_latest.ckpt', 'model_latest.prev.ckpt'
_TMP_MARK = '.tmp.'


def remove_stale_temporaries(save_dir):
    """Temporary files a killed ``save`` left behind (``<snapshot>.tmp.<pid>``)."""
    if parallel.rank() != 0 or not os.path.isdir(save_dir):
        return
    for f in os.listdir(save_dir):
        if '.ckpt' + _TMP_MARK in f:
            try:
                os.remove(os.path.join(save_dir, f))
            except OSError:
                pass


def atomic_save(obj, path, keep_previous_as=None):
    """``torch.save`` that never leaves a partial file under ``path``: written beside it, flushed to the disk, renamed over it.  A reader
    (the next start) finds the old snapshot or the new one.  ``keep_previous_as``: the file that was at ``path`` moves there first."""
    tmp = '%s%s%d' % (path, _TMP_MARK, os.getpid())
    try:
        with open(tmp, 'wb') as f:
            torch.save(obj, f)
            f.flush()
            os.fsync(f.fileno())
        if keep_previous_as is not None and os.path.isfile(path):
            os.replace(path, keep_previous_as)
        os.replace(tmp, path)
    except Exception:
        try:
            os.remove(tmp)
        except OSError:
            pass
        raise


class SnapshotRefused(RuntimeError):
    """A snapshot whose state does not hash to the digest it was saved with (``load``), or a state that holds a NaN or an Inf and is
    not written over a healthy snapshot (``save`` with a guard)."""


class _parameters_frozen(object):
    """``with _parameters_frozen(module):`` -- the module's parameters do not require grad inside the block."""

    def __init__(self, module):
        self.params = [p for p in module.parameters() if p.requires_grad]

    def __enter__(self):
        for p in self.params:
            p.requires_grad_(False)

    def __exit__(self, *exc):
        for p in self.params:
            p.requires_grad_(True)
        return False


class BaseVideoFillInEnvironment(object):
    """environments.py:64-119."""

    def __init__(self, video_fill_in_model, checkpoints_dir, name, padding_size, device=None, use_graph=False):
        self.save_dir = os.path.join(checkpoints_dir, name)
        self.padding_size = padding_size
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.generator = move_to_devices(video_fill_in_model, self.device)
        self.generator.apply(weights_init)
        self.K = self.T = self.F = None
        self.use_graph = use_graph
        self._graphs = {}

    def set_test_inputs(self, preceding_frames, following_frames):
        self.preceding_frames = preceding_frames.contiguous().to(self.device, non_blocking=True)
        self.following_frames = following_frames.contiguous().to(self.device, non_blocking=True)

    def set_gt_middle_frames_test(self, gt_middle_frames):
        self.gt_middle_frames = gt_middle_frames.contiguous().to(self.device, non_blocking=True)

    def forward_test(self):
        if self.use_graph:
            # the convolution precision is part of the key: a switch captures anew instead of replaying the other arithmetic
            key = (self.T, tuple(self.preceding_frames.shape), tuple(self.following_frames.shape), conv_ops.get_conv_precision())
            if key not in self._graphs:
                self._graphs[key] = GraphedForward(self.generator, self.T, self.preceding_frames, self.following_frames)
            self.gen_output = self._graphs[key](self.preceding_frames, self.following_frames)
        else:
            with torch.no_grad():
                self.gen_output = self.generator(self.T, self.preceding_frames, self.following_frames)

    def load(self, snapshot_file_name):
        save_path = os.path.join(self.save_dir, snapshot_file_name)
        if os.path.isfile(save_path):
            print('=> loading snapshot from {}'.format(save_path))
            try:
                snapshot = torch.load(save_path, map_location=self.device, weights_only=False)
            except UnicodeDecodeError:
                # the published checkpoints were pickled by Python 2.7 / torch 0.3.1 (bashes/download/
                # download_model_checkpoints.bash): their byte strings need latin1
                snapshot = torch.load(save_path, map_location=self.device, weights_only=False, encoding='latin1')
        else:
            raise RuntimeError('Failed to find snapshot at path %s' % save_path)
        key = 'generator_ema' if getattr(self, 'weights', 'raw') == 'ema' else 'generator'
        if key not in snapshot:
            raise RuntimeError("%s holds no '%s': it was not written by a run with train.py --ema_decay" % (save_path, key))
        self.generator.load_state_dict(snapshot[key])
        conv_ops.invalidate_derived(self.generator)
        self._graphs.clear()
        return snapshot

    def eval(self):
        self.generator.eval()


class BaseTrainingEnvironment(BaseVideoFillInEnvironment):
    """environments.py:122-259."""

    STEP_GRAPH_WARMUP = 2      # eager updates per (K, T, F, batch shape) before the update is captured
    MAX_STEP_GRAPHS = 2        # a captured update keeps its activations (tens of GB at cfg3): further shapes (--sample_KTF) stay eager

    def __init__(self, fill_in_model, checkpoints_dir, name, lr, beta1, max_K, max_T, max_F, padding_size, device=None,
                 graph_step=False):
        super().__init__(fill_in_model, checkpoints_dir, name, padding_size, device=device)
        # graph_step: ``train_step`` captures one whole update (forward, both backward passes, both Adam steps: ~10,000
        # kernel launches) as a hipGraph after STEP_GRAPH_WARMUP eager updates and replays it; Adam then keeps its step
        # counter on the device (``capturable``).  Off by default: the eager sequence is the reference's.
        self.graph_step = bool(graph_step)
        self._step_graphs = {}
        # resumable (train.py --resumable): snapshots carry ``run_state`` (run_state.py) and ``load`` restores it; off = the reference's keys
        self.resumable = False
        self.data_state_source = None      # train.py: a callable -> the clip order's position, saved with the snapshot
        self.restored_data_state = None    # ... and what ``load`` found for this rank, for train.py to position its clip order with
        self.exact_resume = False          # the last ``load`` restored a run_state
        # guard (train.py --guard): a grad_guard.GradGuard that looks at the gradients between each backward pass and its optimizer step
        # and leaves the step out when they hold a NaN or an Inf; None = the reference's update, nothing looked at
        self.guard = None
        # fused (train.py --fused_step [--ema_decay d]): a fused_step.FusedStep that makes both optimizers' steps, one HIP launch each, on a
        # verdict that stays on the device, and keeps the generator's weight average; None = ``optimizer.step()``
        self.fused = None
        self.start_update = 0
        self.total_updates = 0
        self.start_sum_avg_psnr_err = 0
        self.start_sum_avg_ssim_err = 0
        self.max_K, self.max_T, self.max_F = max_K, max_T, max_F
        self.optimizer_G = torch.optim.Adam(self.generator.parameters(), lr=lr, betas=(beta1, 0.999), capturable=self.graph_step)
        self._reducer_G = parallel.GradAllReducer(self.generator.parameters())
        # The reference draws (K, T, F) from the global numpy RNG (environments.py:417-427).  Data-parallel replicas must
        # draw the SAME values every step, and anything else that touches the global RNG on one rank only (a data-loader
        # retry, user code) would make them diverge for the rest of the run: a private stream, seeded identically on
        # every rank (``seed_KTF`` to change it).
        self._ktf_rng = np.random.RandomState(0)

    def seed_KTF(self, seed):
        self._ktf_rng = np.random.RandomState(seed)

    def sample_KTF(self, allow_random_sampling):
        if allow_random_sampling:
            K = self._ktf_rng.randint(1, self.max_K + 1)
            T = self._ktf_rng.randint(1, self.max_T + 1)
            F = self._ktf_rng.randint(1, self.max_F + 1)
        else:
            K, T, F = self.max_K, self.max_T, self.max_F
        return K, T, F

    def set_train_inputs(self, preceding_frames, following_frames, gt_middle_frames):
        self.preceding_frames = preceding_frames.contiguous().to(self.device, non_blocking=True)
        self.following_frames = following_frames.contiguous().to(self.device, non_blocking=True)
        self.gt_middle_frames = gt_middle_frames.contiguous().to(self.device, non_blocking=True)

    def forward_train(self):
        self.gen_output = self.generator(self.T, self.preceding_frames, self.following_frames)

    # attributes an update produces (tensors of the captured graph's pool when the update is replayed).  Every tensor with autograd
    # history that an update leaves on the environment belongs here -- a new loss term's values included: train_step detaches these
    # before a capture ends, and one that is missing outlives the capture and faults the HIP runtime when it is closed
    _STEP_OUTPUTS = ('gen_output', 'loss_G', 'Lp', 'gdl', 'L_GAN', 'loss_d_fake', 'loss_d_real', 'loss_D', 'Lp_forward',
                     'Lp_backward', 'gdl_forward', 'gdl_backward', 'ssim', 'ssim_forward', 'ssim_backward', 'lap', 'lap_forward', 'lap_backward',
                     'temporal', 'temporal_forward', 'temporal_backward', 'census', 'census_forward', 'census_backward')

    def train_step(self, preceding_frames, following_frames, gt_middle_frames):
        """One update on a batch: set_train_inputs + forward_train + optimize_parameters (src/train.py:147-169), with
        ``self.K, self.T, self.F`` set by the caller.  With ``graph_step`` (one process; data-parallel runs stay eager) the
        update is captured once per (K, T, F, batch shape) and replayed from static input buffers."""
        if not self.graph_step or parallel.world_size() > 1:
            self.set_train_inputs(preceding_frames, following_frames, gt_middle_frames)
            self.forward_train()
            self.optimize_parameters()
            return
        key = (self.K, self.T, self.F, tuple(preceding_frames.shape), tuple(following_frames.shape), tuple(gt_middle_frames.shape))
        state = self._step_graphs.setdefault(key, {'eager': 0})
        captured = sum(1 for v in self._step_graphs.values() if 'graph' in v)
        if state['eager'] < self.STEP_GRAPH_WARMUP or ('graph' not in state and captured >= self.MAX_STEP_GRAPHS):
            # MIOpen's algorithm search, lazy allocations, Adam's state -- or no room for another captured update
            state['eager'] += 1
            self.set_train_inputs(preceding_frames, following_frames, gt_middle_frames)
            self.forward_train()
            self.optimize_parameters()
            return
        if 'graph' not in state:
            self.set_train_inputs(preceding_frames, following_frames, gt_middle_frames)
            state['inputs'] = (self.preceding_frames.clone(), self.following_frames.clone(), self.gt_middle_frames.clone())
            self.preceding_frames, self.following_frames, self.gt_middle_frames = state['inputs']
            self._prepare_capture()
            torch.cuda.synchronize(self.device)
            graph = torch.cuda.CUDAGraph()
            # No tensor that carries autograd history may be released inside the capture or outlive it: the previous
            # (eager) update's outputs are detached before, this update's before the capture ends.  Either one left alone
            # ends in a fault inside the HIP runtime when the capture is closed (tools/graph_op_bisect.py gen_keep_out*,
            # tools/graph_step_bisect.py m0).
            self._detach_step_outputs()
            # ... and whatever autograd graph pieces are only kept alive by reference cycles go NOW, not at some allocation
            # inside the capture.  What this cannot see is a caller that still holds a tensor with history from an earlier eager
            # update (a loss, ``env.gen_output['pred']``): the capturing call is made with such references dropped or detached.
            import gc
            gc.collect()
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('train_step: already inside a stream capture; a step graph cannot be nested')
            with torch.cuda.graph(graph):
                self.forward_train()
                self.optimize_parameters()
                self._detach_step_outputs()
            state['graph'] = graph
            state['outputs'] = {k: getattr(self, k) for k in self._STEP_OUTPUTS if hasattr(self, k)}
        else:
            p, f, g = state['inputs']
            p.copy_(preceding_frames, non_blocking=True)
            f.copy_(following_frames, non_blocking=True)
            g.copy_(gt_middle_frames, non_blocking=True)
            self.preceding_frames, self.following_frames, self.gt_middle_frames = p, f, g
            for k, v in state['outputs'].items():
                setattr(self, k, v)
        state['graph'].replay()
        # the replay recomputed the derived weights (Winograd-domain filters) BEFORE its optimizer steps and moved no
        # version counter: whatever runs eagerly next (validation, a snapshot's forward) must rebuild them
        conv_ops.invalidate_derived()

    def _detach_step_outputs(self):
        for k in self._STEP_OUTPUTS:
            v = getattr(self, k, None)
            if isinstance(v, dict):
                setattr(self, k, {name: t.detach() for name, t in v.items()})
            elif torch.is_tensor(v):
                setattr(self, k, v.detach())

    def _prepare_capture(self):
        """Host-side work a captured update may not do (host-to-device copies): done here, once."""

    def get_current_state_dict(self, total_updates, sum_avg_psnr_err, sum_avg_ssim_err):
        state = {
            'updates': total_updates,
            'sum_avg_psnr_err': sum_avg_psnr_err,
            'sum_avg_ssim_err': sum_avg_ssim_err,
            'generator': self.generator.state_dict(),
            'optimizer_G': self._optimizer_state_dict(self.optimizer_G),
        }
        if self.fused is not None and self.fused.ema_decay is not None:
            state['generator_ema'] = self.fused.ema_state_dict(self.generator)
        if self.resumable:
            # the one key beyond the reference's; a collective in a data-parallel run (every rank's generator states go to rank 0)
            state['run_state'] = run_state.capture(self)
        return state

    def _optimizer_state_dict(self, optimizer):
        return optimizer.state_dict() if self.fused is None else self.fused.optimizer_state_dict(optimizer)

    def load(self, snapshot_file_name):
        snapshot = super().load(snapshot_file_name)
        self.start_update = snapshot['updates']
        self.start_sum_avg_psnr_err = snapshot['sum_avg_psnr_err']
        self.start_sum_avg_ssim_err = snapshot['sum_avg_ssim_err']
        self._step_graphs.clear()
        if self.resumable and snapshot.get('run_state') is not None:
            # another schedule (a cosine over another --max_iter too) is another run: refused before anything is loaded
            saved = snapshot['run_state'].get('lr_schedule')
            if self.fused is not None:
                self.fused.check_continues(saved)
            elif saved is not None:
                raise ValueError('the snapshot was written with a learning-rate schedule or weight decay (%s), this run has neither: '
                                 'it cannot be continued exactly' % ' '.join('--%s %s' % kv for kv in sorted(saved.items())))
        self._load_training_state(snapshot)
        if self.fused is not None:
            self.fused.after_load(snapshot, (snapshot.get('run_state') or {}).get('ema') if self.resumable else None)
        self._restore_run_state(snapshot, snapshot_file_name)       # last: the generator states are set behind everything that could draw
        if self.fused is not None:
            self.fused.push_counters()
        return snapshot

    def _load_training_state(self, snapshot):
        self.optimizer_G.load_state_dict(snapshot['optimizer_G'])

    def _restore_run_state(self, snapshot, snapshot_file_name):
        self.exact_resume, self.restored_data_state = False, None
        if not self.resumable:
            return
        state = snapshot.get('run_state')
        if state is None:
            print('%s carries no run_state: the run continues from its weights and optimizer state, but NOT exactly (spectral-norm '
                  'vectors, generator states and the clip order start afresh)' % snapshot_file_name)
            return
        try:
            data_state = run_state.restore(self, state)
        except run_state.RunStateRefused as e:
            print('%s: %s: the run continues from its weights and optimizer state, but NOT exactly' % (snapshot_file_name, e))
            return
        want = state['ranks'][parallel.rank()]['digest']
        have = run_state.digest(self, data_state, guard_counters=state.get('guard'),      # the table of the run that wrote it
                                ema=fused_step_module.snapshot_ema_entries(snapshot))
        if have != want:
            raise SnapshotRefused('state digest %016x after loading, %016x when it was saved' % (have, want))
        self.exact_resume, self.restored_data_state = True, data_state

    def save(self, snapshot_file_name, total_updates, sum_avg_psnr_err, sum_avg_ssim_err):
        if parallel.rank() != 0 and not (self.resumable and parallel.world_size() > 1):
            return
        if self.fused is not None:
            self.sync_guard(agree=self.resumable and parallel.world_size() > 1)
        if self.guard is not None:
            self._refuse_non_finite_state(snapshot_file_name)
        state = self.get_current_state_dict(total_updates, sum_avg_psnr_err, sum_avg_ssim_err)
        if parallel.rank() != 0:
            return
        os.makedirs(self.save_dir, exist_ok=True)
        keep = os.path.join(self.save_dir, PREVIOUS) if self.resumable and snapshot_file_name == LATEST else None
        atomic_save(state, os.path.join(self.save_dir, snapshot_file_name), keep_previous_as=keep)

    def _guarded_state(self):
        """(name, tensor) of the float state a snapshot holds: weights, Adam moments, spectral-norm vectors."""
        named = [('generator.' + k, v) for k, v in self.generator.state_dict().items()]
        optimizers = [('optimizer_G', self.optimizer_G)]
        disc = getattr(self, 'discriminator', None)
        if disc is not None:
            named += [('discriminator.' + k, v) for k, v in disc.state_dict().items()]
            optimizers.append(('optimizer_D', self.optimizer_D))
        for tag, optimizer in optimizers:
            for i, p in enumerate(p for group in optimizer.param_groups for p in group['params']):
                named += [('%s.%d.%s' % (tag, i, k), optimizer.state[p][k]) for k in ('exp_avg', 'exp_avg_sq') if p in optimizer.state]
        named += [('u.' + k, u) for k, u in run_state.sn_vectors(disc).items() if u is not None]
        if self.fused is not None:
            named += self.fused.named_ema()
        return named

    def _refuse_non_finite_state(self, snapshot_file_name):
        from . import grad_guard
        found = grad_guard.first_nonfinite(self._guarded_state())
        every_rank = self.resumable and parallel.world_size() > 1        # ... is here (``save`` is a collective then): one answer
        if (self.guard.agree(int(found is not None)) if every_rank else found is not None):
            raise SnapshotRefused('%s is not written: the state holds non-finite values (%s)' % (
                snapshot_file_name, '%d in %s' % (found[1], found[0]) if found else 'on another rank'))

    def _step(self, which, module, optimizer):
        """``optimizer.step()``; with a guard, only when the gradients it is about to use are finite (clipped first, if asked)."""
        if self.fused is not None:
            self.fused.step(which, last=which == 'D' or not hasattr(self, 'optimizer_D'))
        elif self.guard is None or self.guard.check(which, module.named_parameters()):
            optimizer.step()

    def sync_guard(self, agree=False):
        """With a fused step: wait for the last launched update's verdict record and bring the guard's counters, norms and message up to
        it; raises GuardGaveUp if the device has given up.  Called where the run waits anyway: a printed line, validation, ``save``.
        ``agree``: every rank is here (a collective that checks that the ranks' counters are the same)."""
        if self.fused is not None:
            self.fused.read(wait=True, agree=agree)

    def _zero_grad(self, optimizer, reducer):
        """One process: the reference's ``optimizer.zero_grad()``.  Data parallel: gradients live in the reducer's flat
        buckets and each bucket's all-reduce starts during the backward pass (parallel.GradAllReducer)."""
        if parallel.world_size() > 1:
            reducer.zero_grad()
        else:
            optimizer.zero_grad()

    def optimize_parameters(self):
        self._zero_grad(self.optimizer_G, self._reducer_G)
        self.compute_loss_G()
        self.loss_G.backward()
        self._reducer_G.allreduce_()
        self._step('G', self.generator, self.optimizer_G)
        if self.guard is not None and self.fused is None and not hasattr(self, 'optimizer_D'):
            self.guard.end_update()

    def compute_loss_G(self):
        self.loss_G = torch.zeros(1, device=self.device)

    def get_current_errors(self):
        return {'G_loss': float(self.loss_G.item())}

    def train(self):
        self.generator.train()


class L2GDLDiscTrainingEnvironment(BaseTrainingEnvironment):
    """environments.py:262-397: loss_G = alpha (MSE + GDL)(pred) + beta BCE(D(cat[P, pred, F]), 1);
    loss_D = BCE(D(fake.detach()), window labels) + BCE(D(real), 1)."""

    def __init__(self, fill_in_model, checkpoints_dir, name, image_size, c_dim, alpha, beta, lr, beta1, df_dim, Ip,
                 disc_t, max_K, max_T, max_F, padding_size, device=None, graph_step=False, ssim_weight=0.0, image_loss='l2',
                 charbonnier_eps=1e-3, lap_weight=0.0, lap_levels=5, temporal_weight=0.0, temporal_kind='charbonnier', temporal_eps=1e-3,
                 census_weight=0.0):
        super().__init__(fill_in_model, checkpoints_dir, name, lr, beta1, max_K, max_T, max_F, padding_size, device=device,
                         graph_step=graph_step)
        # ssim_weight (train.py --ssim_weight G) > 0: loss_G gains G (1 - mean SSIM) per prediction (losses.SSIMLoss, one HIP launch for
        # the loss and its gradient); 0 = the reference's loss: no module, no launch, no extra key in get_current_errors
        self.ssim_weight = float(ssim_weight)
        self.loss_ssim = SSIMLoss() if self.ssim_weight > 0 else None
        # image_loss (train.py --image_loss) 'l1' / 'charbonnier': Lp and gdl of every prediction come from losses.ImageLoss on the model's
        # own [B, T, C, H, W] layout (one HIP launch for the losses and their gradients, no time-major copies); 'l2' = the reference's
        # MSELoss + GDL composition below: no module, no launch
        self.loss_image = ImageLoss(image_loss, charbonnier_eps) if image_loss != 'l2' else None
        # lap_weight (train.py --lap_weight G) > 0: loss_G gains G times the Laplacian-pyramid L1 distance per prediction (losses.LapLoss
        # with lap_levels levels, one HIP launch for the loss and its gradient); 0 = no module, no launch, no extra key
        self.lap_weight = float(lap_weight)
        self.loss_lap = LapLoss(lap_levels) if self.lap_weight > 0 else None
        # temporal_weight (train.py --temporal_weight G) > 0: loss_G gains G times the temporal-difference term of every prediction
        # (losses.TemporalLoss: one HIP launch for all predictions of an update, each read in its own layout -- gen_output['pred'] is a
        # time-major view and is not copied); 0 = no module, no launch, no extra key
        self.temporal_weight = float(temporal_weight)
        self.loss_temporal = TemporalLoss(temporal_kind, temporal_eps) if self.temporal_weight > 0 else None
        # census_weight (train.py --census_weight G) > 0: loss_G gains G times the census (soft ternary) term of every prediction
        # (losses.CensusLoss: one HIP launch for all predictions of an update, each read in its own layout); 0 = no module, no launch, no
        # extra key
        self.census_weight = float(census_weight)
        self.loss_census = CensusLoss() if self.census_weight > 0 else None
        self._fake_labels = {}
        self.loss_Lp = torch.nn.MSELoss()
        self.loss_gdl = GDL()
        self.loss_d = torch.nn.BCEWithLogitsLoss()
        self.alpha, self.beta, self.disc_t = alpha, beta, disc_t
        discriminator = SNDiscriminator((image_size[0] + padding_size[0], image_size[1] + padding_size[1]), c_dim,
                                        disc_t, df_dim, Ip)
        discriminator = move_to_devices(discriminator, self.device)
        discriminator.apply(weights_init)
        self.discriminator = discriminator
        self.optimizer_D = torch.optim.Adam(self.discriminator.parameters(), lr=lr, betas=(beta1, 0.999), capturable=self.graph_step)
        self._reducer_D = parallel.GradAllReducer(self.discriminator.parameters())

    def sync_replicas(self):
        """Data-parallel start-up: identical weights and identical SN ``u`` vectors on every rank (rank 0's)."""
        parallel.materialise_sn_vectors(self.discriminator)
        parallel.broadcast_module_state(self.generator)
        parallel.broadcast_module_state(self.discriminator)

    def get_current_state_dict(self, total_updates, sum_avg_psnr_err, sum_avg_ssim_err):
        state = super().get_current_state_dict(total_updates, sum_avg_psnr_err, sum_avg_ssim_err)
        state['discriminator'] = self.discriminator.state_dict()
        state['optimizer_D'] = self._optimizer_state_dict(self.optimizer_D)
        return state

    def _load_training_state(self, snapshot):
        super()._load_training_state(snapshot)
        self.discriminator.load_state_dict(snapshot['discriminator'])
        conv_ops.invalidate_derived(self.discriminator)
        self.optimizer_D.load_state_dict(snapshot['optimizer_D'])

    def create_fake_labels(self):
        """1 for windows made of real frames only (both ends), 0 for every window touching a generated frame
        (environments.py:308-323) -> [K+T+F-disc_t+1]."""
        ones_p = max(0, self.K - self.disc_t + 1)
        ones_f = max(0, self.F - self.disc_t + 1)
        n = self.K + self.T + self.F - self.disc_t + 1
        labels = torch.zeros(n)
        labels[:ones_p] = 1
        if ones_f > 0:
            labels[n - ones_f:] = 1
        return labels

    def _device_fake_labels(self):
        key = (self.K, self.T, self.F)
        if key not in self._fake_labels:
            self._fake_labels[key] = self.create_fake_labels().to(self.device)
        return self._fake_labels[key]

    def _prepare_capture(self):
        self._device_fake_labels()

    def compute_loss_D(self):
        fake = torch.cat([self.preceding_frames, self.gen_output['pred'], self.following_frames], dim=1).detach()
        h = self.discriminator(fake)
        labels = self._device_fake_labels().view(1, -1).expand(fake.size(0), -1)
        self.loss_d_fake = self.loss_d(h, labels)
        real = torch.cat([self.preceding_frames, self.gt_middle_frames, self.following_frames], dim=1).detach()
        h_ = self.discriminator(real)
        self.loss_d_real = self.loss_d(h_, torch.ones_like(h_))
        self.loss_D = self.loss_d_fake + self.loss_d_real

    def optimize_parameters(self):
        super().optimize_parameters()
        self._zero_grad(self.optimizer_D, self._reducer_D)
        self.compute_loss_D()
        self.loss_D.backward()
        self._reducer_D.allreduce_()
        self._step('D', self.discriminator, self.optimizer_D)
        if self.guard is not None and self.fused is None:
            self.guard.end_update()

    @staticmethod
    def _time_major_01(x):
        """[B,T,C,H,W] in [-1,1] -> [T*B,C,H,W] in [0,1] (environments.py:363-368)."""
        _, _, c, H, W = x.shape
        return inverse_transform(x.permute(1, 0, 2, 3, 4).contiguous().view(-1, c, H, W))

    _IMAGE_LOSS_KEYS = ('pred',)          # the predictions the image loss is applied to, the first one being ``pred``

    def compute_loss_G(self):
        super().compute_loss_G()
        if self.loss_image is not None:
            # every prediction in one launch; the terms are detached values for the printed line, the losses carry the gradient
            image_losses = self.loss_image(tuple(self.gen_output[k] for k in self._IMAGE_LOSS_KEYS), self.gt_middle_frames)
            self.Lp, self.gdl = self.loss_image.last_terms[0]
        else:
            gt = self._time_major_01(self.gt_middle_frames)
            outputs = self._time_major_01(self.gen_output['pred'])
            self.Lp = self.loss_Lp(outputs, gt)
            self.gdl = self.loss_gdl(outputs, gt)
        fake = torch.cat([self.preceding_frames, self.gen_output['pred'], self.following_frames], dim=1)
        # The reference lets this backward pass fill the discriminator's .grad as well and throws those values away
        # (optimizer_D.zero_grad() comes before they are ever read, environments.py:348-355): here the discriminator's
        # parameters are taken out of the graph for this evaluation, which skips a third of its weight-gradient work.
        with _parameters_frozen(self.discriminator):
            h = self.discriminator(fake)
        self.L_GAN = self.loss_d(h, torch.ones_like(h))
        if self.loss_image is not None:
            self.loss_G = self.loss_G + self.alpha * image_losses[0] + self.beta * self.L_GAN          # point + gdl, summed in float64
            self._add_further_image_losses(image_losses[1:])
        else:
            self.loss_G = self.loss_G + self.alpha * (self.Lp + self.gdl) + self.beta * self.L_GAN
        if self.loss_ssim is not None:
            # on the model's own [B, T, C, H, W] layout: the mean over planes does not care about their order
            self.ssim = self.loss_ssim(self.gen_output['pred'], self.gt_middle_frames)
            self.loss_G = self.loss_G + self.ssim_weight * self.ssim
        if self.loss_lap is not None:
            self.lap = self.loss_lap(self.gen_output['pred'], self.gt_middle_frames)
            self.loss_G = self.loss_G + self.lap_weight * self.lap
        if self.loss_temporal is not None:
            temporal = self.loss_temporal(tuple(self.gen_output[k] for k in self._IMAGE_LOSS_KEYS), self.gt_middle_frames)
            self.temporal = temporal[0]
            self.loss_G = self.loss_G + self.temporal_weight * self.temporal
            self._add_further_temporal_losses(temporal[1:])
        if self.loss_census is not None:
            census = self.loss_census(tuple(self.gen_output[k] for k in self._IMAGE_LOSS_KEYS), self.gt_middle_frames)
            self.census = census[0]
            self.loss_G = self.loss_G + self.census_weight * self.census
            self._add_further_census_losses(census[1:])

    def _add_further_census_losses(self, losses):
        """The census terms of ``_IMAGE_LOSS_KEYS[1:]`` (they came from the same launch as ``pred``'s): none here."""

    def _add_further_temporal_losses(self, losses):
        """The temporal terms of ``_IMAGE_LOSS_KEYS[1:]`` (they came from the same launch as ``pred``'s): none here."""

    def _add_further_image_losses(self, losses):
        """The image losses of ``_IMAGE_LOSS_KEYS[1:]`` (they came from the same launch as ``pred``'s): none here."""

    def get_current_errors(self):
        d = super().get_current_errors()
        d.update({'G_Lp': float(self.Lp.item()), 'G_gdl': float(self.gdl.item()),
                  'D_real': float(self.loss_d_real.item()), 'D_fake': float(self.loss_d_fake.item()),
                  'G_GAN': float(self.L_GAN.item())})
        if self.loss_ssim is not None:
            d['G_ssim'] = float(self.ssim.item())
        if self.loss_lap is not None:
            d['G_lap'] = float(self.lap.item())
        if self.loss_temporal is not None:
            d['G_temporal'] = float(self.temporal.item())
        if self.loss_census is not None:
            d['G_census'] = float(self.census.item())
        return d

    def train(self):
        super().train()
        self.discriminator.train()


class MCNetTrainingEnvironment(L2GDLDiscTrainingEnvironment):
    """environments.py:400-412."""

    def sample_KTF(self, allow_random_sampling):
        if allow_random_sampling:
            return (self._ktf_rng.randint(2, self.max_K + 1), self._ktf_rng.randint(1, self.max_T + 1),
                    self._ktf_rng.randint(1, self.max_F + 1))
        return self.max_K, self.max_T, self.max_F


class TAITrainingEnvironment(L2GDLDiscTrainingEnvironment):
    """environments.py:415-485: adds alpha (MSE + GDL) on the forward and on the backward intermediate prediction."""

    def sample_KTF(self, allow_random_sampling):
        if allow_random_sampling:
            return (self._ktf_rng.randint(2, self.max_K + 1), self._ktf_rng.randint(1, self.max_T + 1),
                    self._ktf_rng.randint(2, self.max_F + 1))
        return self.max_K, self.max_T, self.max_F

    _IMAGE_LOSS_KEYS = ('pred', 'pred_forward', 'pred_backward')

    def compute_loss_G(self):
        super().compute_loss_G()
        if self.loss_image is None:
            gt = self._time_major_01(self.gt_middle_frames)
            out_f = self._time_major_01(self.gen_output['pred_forward'])
            out_b = self._time_major_01(self.gen_output['pred_backward'])
            self.Lp_forward = self.loss_Lp(out_f, gt)
            self.Lp_backward = self.loss_Lp(out_b, gt)
            self.gdl_forward = self.loss_gdl(out_f, gt)
            self.gdl_backward = self.loss_gdl(out_b, gt)
            self.loss_G = self.loss_G + self.alpha * (self.Lp_forward + self.Lp_backward + self.gdl_forward + self.gdl_backward)
        if self.loss_ssim is not None:
            self.ssim_forward = self.loss_ssim(self.gen_output['pred_forward'], self.gt_middle_frames)
            self.ssim_backward = self.loss_ssim(self.gen_output['pred_backward'], self.gt_middle_frames)
            self.loss_G = self.loss_G + self.ssim_weight * (self.ssim_forward + self.ssim_backward)
        if self.loss_lap is not None:
            self.lap_forward = self.loss_lap(self.gen_output['pred_forward'], self.gt_middle_frames)
            self.lap_backward = self.loss_lap(self.gen_output['pred_backward'], self.gt_middle_frames)
            self.loss_G = self.loss_G + self.lap_weight * (self.lap_forward + self.lap_backward)

    def _add_further_image_losses(self, losses):
        (self.Lp_forward, self.gdl_forward), (self.Lp_backward, self.gdl_backward) = self.loss_image.last_terms[1:]
        self.loss_G = self.loss_G + self.alpha * (losses[0] + losses[1])

    def _add_further_temporal_losses(self, losses):
        self.temporal_forward, self.temporal_backward = losses
        self.loss_G = self.loss_G + self.temporal_weight * (self.temporal_forward + self.temporal_backward)

    def _add_further_census_losses(self, losses):
        self.census_forward, self.census_backward = losses
        self.loss_G = self.loss_G + self.census_weight * (self.census_forward + self.census_backward)

    def get_current_errors(self):
        d = super().get_current_errors()
        d.update({'G_Lp_forward': float(self.Lp_forward.item()), 'G_gdl_forward': float(self.gdl_forward.item()),
                  'G_Lp_backward': float(self.Lp_backward.item()), 'G_gdl_backward': float(self.gdl_backward.item())})
        if self.loss_ssim is not None:
            d.update({'G_ssim_forward': float(self.ssim_forward.item()), 'G_ssim_backward': float(self.ssim_backward.item())})
        if self.loss_lap is not None:
            d.update({'G_lap_forward': float(self.lap_forward.item()), 'G_lap_backward': float(self.lap_backward.item())})
        if self.loss_temporal is not None:
            d.update({'G_temporal_forward': float(self.temporal_forward.item()), 'G_temporal_backward': float(self.temporal_backward.item())})
        if self.loss_census is not None:
            d.update({'G_census_forward': float(self.census_forward.item()), 'G_census_backward': float(self.census_backward.item())})
        return d
