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
import collections
import functools
import operator
import os

import numpy as np
import torch

from . import conv_ops, parallel, run_state
from . import fused_step as fused_step_module
from .graph import GraphedForward
from .losses import GDL, CensusLoss, ImageLoss, LapLoss, LossSettings, SSIMLoss, TemporalLoss
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
                                resumable=False, guard=None, fused_step=False, ema_decay=None, max_iter=100000, losses=None,
                                lr_D=None, lr_schedule=None, weight_decay=0.0, **loss_settings):
    # losses: a losses.LossSettings (train.py's loss flags); its fields are also taken as keywords (ssim_weight=0.2).  Neither = the
    # reference's loss
    if losses is not None and loss_settings:
        raise TypeError('create_training_environment: losses= and %s are two ways to say one thing' % ', '.join(sorted(loss_settings)))
    losses = losses or LossSettings(**loss_settings)
    losses.check()
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
        environment = TAITrainingEnvironment      # environments.py:29-31
    elif isinstance(fill_in_model, MCNetFillInModel):
        environment = MCNetTrainingEnvironment
    else:
        raise RuntimeError('Tried to create a training environment for object of unsupported type %s'
                           % type(fill_in_model).__name__)
    env = environment(fill_in_model, checkpoints_dir, name, image_size, c_dim, alpha, beta, lr, beta1, df_dim, Ip, disc_window_size,
                      max_K, max_T, max_F, padding_size, device=device, graph_step=graph_step, losses=losses)
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


# one term of loss_G (L2GDLDiscTrainingEnvironment.__init__ says what the fields mean)
_Term = collections.namedtuple('_Term', 'name weight module together adds shows')


def _one_by_one(module):
    """``module(prediction, gt)`` behind the signature of the terms that take every prediction in one call."""
    return lambda predictions, gt: tuple(module(p, gt) for p in predictions)


def _sum(values):
    """Left to right: loss_G is an fp32 fold, so the order of the addends is part of what an update computes."""
    return functools.reduce(operator.add, values)


def _further(values):
    """The sum that goes into loss_G for the predictions behind ``pred``, value by value: Lp_forward + Lp_backward + gdl_forward + ..."""
    return _sum(v for column in zip(*values) for v in column)


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

    PREDICTIONS = ('pred',)    # the keys of ``gen_output`` the loss terms are applied to, ``pred`` first
    _terms = ()                # the loss terms of an update (L2GDLDiscTrainingEnvironment builds the table)

    def _term_values(self, printed=False):
        """The attributes the loss terms write in an update, or those of them that are ``printed``: each value's name, with ``_forward``
        and ``_backward`` behind it for the further predictions."""
        return [name + key[len('pred'):] for term in self._terms
                for name in (term.shows if printed else dict.fromkeys(term.adds + term.shows)) for key in self.PREDICTIONS]

    # attributes an update produces (tensors of the captured graph's pool when the update is replayed): train_step detaches them before
    # a capture ends, because a tensor with autograd history that outlives the capture faults the HIP runtime when it is closed.  Every
    # value a loss term leaves on the environment is written under a name of the term table, so the list follows from the table
    @property
    def _STEP_OUTPUTS(self):
        return ('gen_output', 'loss_G', 'L_GAN', 'loss_d_fake', 'loss_d_real', 'loss_D') + tuple(self._term_values())

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
                 disc_t, max_K, max_T, max_F, padding_size, device=None, graph_step=False, losses=None):
        super().__init__(fill_in_model, checkpoints_dir, name, lr, beta1, max_K, max_T, max_F, padding_size, device=device,
                         graph_step=graph_step)
        losses = losses or LossSettings()
        self._fake_labels = {}
        self.loss_Lp = torch.nn.MSELoss()
        self.loss_gdl = GDL()
        self.loss_d = torch.nn.BCEWithLogitsLoss()
        self.alpha, self.beta, self.disc_t = alpha, beta, disc_t
        self.ssim_weight, self.lap_weight = float(losses.ssim_weight), float(losses.lap_weight)
        self.temporal_weight, self.census_weight = float(losses.temporal_weight), float(losses.census_weight)
        # a term that is off builds nothing: no module, no launch, no key in get_current_errors.  'l2' is the reference's image loss
        self.loss_image = ImageLoss(losses.image_loss, losses.charbonnier_eps) if losses.image_loss != 'l2' else None
        self.loss_ssim = SSIMLoss() if self.ssim_weight > 0 else None
        self.loss_lap = LapLoss(losses.lap_levels) if self.lap_weight > 0 else None
        self.loss_temporal = TemporalLoss(losses.temporal_kind, losses.temporal_eps) if self.temporal_weight > 0 else None
        self.loss_census = CensusLoss() if self.census_weight > 0 else None
        # The terms of loss_G in the order compute_loss_G adds them.  ``module(predictions, gt)`` -> per prediction the values named by
        # ``adds``, whose sum times ``weight`` goes into loss_G; ``shows``: the values get_current_errors prints.  ``together``: one call
        # (one HIP launch for the losses and gradients, each tensor read in its own layout) takes every prediction of the update; else
        # the module sees one prediction per call.  An ImageLoss carries the gradient in ``image`` and prints its detached Lp and gdl.
        if self.loss_image is None:
            self._terms = [_Term('image', alpha, self._mse_and_gdl, False, ('Lp', 'gdl'), ('Lp', 'gdl'))]
        else:
            self._terms = [_Term('image', alpha, self.loss_image, True, ('image',), ('Lp', 'gdl'))]
        for term_name, weight, module, together in (('ssim', self.ssim_weight, self.loss_ssim, False), ('lap', self.lap_weight, self.loss_lap, False),
                                                    ('temporal', self.temporal_weight, self.loss_temporal, True),
                                                    ('census', self.census_weight, self.loss_census, True)):
            if module is not None:
                self._terms.append(_Term(term_name, weight, module if together else _one_by_one(module), together, (term_name,), (term_name,)))
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

    def _mse_and_gdl(self, predictions, gt):
        """The reference's image loss (environments.py:363-372) -> (Lp, gdl) per prediction."""
        gt = self._time_major_01(gt)
        return tuple((self.loss_Lp(x, gt), self.loss_gdl(x, gt)) for x in [self._time_major_01(p) for p in predictions])

    def _evaluate(self, term, keys):
        """One call of the term's module on the predictions ``keys``; its values stay on the environment under their names -> per
        prediction the values loss_G adds."""
        values = [v if isinstance(v, tuple) else (v,) for v in term.module(tuple(self.gen_output[k] for k in keys), self.gt_middle_frames)]
        for i, key in enumerate(keys):
            named = list(zip(term.adds, values[i]))
            if term.shows != term.adds:                 # an ImageLoss: the detached terms of the same launch
                named += zip(term.shows, term.module.last_terms[i])
            for name, v in named:
                setattr(self, name + key[len('pred'):], v)
        return values

    def compute_loss_G(self):
        super().compute_loss_G()
        for term in self._terms:
            values = self._evaluate(term, self.PREDICTIONS if term.together else self.PREDICTIONS[:1])
            self.loss_G = self.loss_G + term.weight * _sum(values[0])
            if term.name == 'image':
                fake = torch.cat([self.preceding_frames, self.gen_output['pred'], self.following_frames], dim=1)
                # The reference lets this backward pass fill the discriminator's .grad as well and throws those values away
                # (optimizer_D.zero_grad() comes before they are ever read, environments.py:348-355): here the discriminator's
                # parameters are taken out of the graph for this evaluation, which skips a third of its weight-gradient work.
                with _parameters_frozen(self.discriminator):
                    h = self.discriminator(fake)
                self.L_GAN = self.loss_d(h, torch.ones_like(h))
                self.loss_G = self.loss_G + self.beta * self.L_GAN
            if values[1:]:
                self.loss_G = self.loss_G + term.weight * _further(values[1:])
        # the modules that see one prediction per call come to the further predictions behind every term's ``pred``
        for term in self._terms:
            if not term.together and self.PREDICTIONS[1:]:
                self.loss_G = self.loss_G + term.weight * _further(self._evaluate(term, self.PREDICTIONS[1:]))

    def get_current_errors(self):
        d = super().get_current_errors()
        d.update({'D_real': float(self.loss_d_real.item()), 'D_fake': float(self.loss_d_fake.item()), 'G_GAN': float(self.L_GAN.item())})
        d.update(('G_' + name, float(getattr(self, name).item())) for name in self._term_values(printed=True))
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

    PREDICTIONS = ('pred', 'pred_forward', 'pred_backward')
