"""bi-TAI fill-in model: the MI355X-side mirror of the reference's ``src/models/tai/tai.py``.

``TAIFillInModel.forward(T, preceding_frames, following_frames)`` keeps the reference's contract (tai.py:52-120):
inputs ``[B, K|F, C, H, W]`` in [-1, 1] (BGR when C = 3), output dict with ``pred``, ``pred_forward``,
``pred_backward``, ``interp_net_outputs_1``, ``interp_net_outputs_2``, each ``[B, T, C, H, W]``.  State-dict keys are
the reference's: ``generator.*`` (MCNet), ``merge_residual{1,2,3}.res.{0,2}``, ``kernelnet.moduleConv.i.{0,2,4}``,
``kernelnet.moduleDeconv.i.{0,2,4}``, ``kernelnet.moduleUpsample.i.1``,
``kernelnet.module{Vertical,Horizontal}{1,2}.{0,2,4,7}``.

What is arranged differently from the reference (same arithmetic):
  * the two MC-Net passes (forward in time on the preceding frames, backward in time on the reversed following
    frames) are independent until the blend, so they run as ONE pass at batch 2B through the shared-weight generator
    when K == F: half the kernel launches and twice the rows per MIOpen call;
  * the T kernel-network evaluations (and their 2T separable convolutions) are independent of each other once the
    MC-Net passes are done, so they run as one batch of T*B;
  * ``merge_residual1`` is constructed (its weights are part of the checkpoint schema) but never evaluated: the
    reference computes it and never reads the result (tai.py:93, :224-226 only index 2 and 1);
  * the time ratio enters as a constant extra channel only where the reference injects it (decoder block 3 of the
    5-block gray model; the 4-block colour model never reaches that index, tai.py:213-217), built on the input's
    device without a host round trip;
  * torch 0.3.1's bilinear upsample is what modern PyTorch calls ``align_corners=True``; it runs on its own HIP
    kernel (upsample.py): the stock ATen kernel was 25 % of the forward on MI355X;
  * the separable convolutions call the HIP kernels through the C ABI (separable_convolution.py) on the current
    stream: the whole forward is hipGraph-capturable (graph.py).
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .conv_ops import conv_bias_act, mark_outside_recurrence
from .mcnet import IndexedConvs, MCNet, Residual, _conv_relu_chain
from .separable_convolution import SeparableConvolution
from .upsample import upsample2x
from .util import gray01


class _ReplicatePadFixedOrder(torch.autograd.Function):
    """``F.pad(x, [p] * 4, mode='replicate')`` whose backward sums in a fixed order.  ATen's backward scatters every padded position
    into its source pixel with float atomics -- a corner pixel of a 51-tap pad collects 26 x 26 of them in arrival order -- and this is
    where the gradient enters MC-Net, so one update is then not reproducible from identical state in any generator weight.  Here the
    border is folded back by two reductions (rows, then columns): the values differ from the atomic form's in the last bits only."""

    @staticmethod
    def forward(ctx, x, p):
        ctx.p = p
        return F.pad(x, [p] * 4, mode='replicate')

    @staticmethod
    def backward(ctx, g):
        p = ctx.p
        H, W = g.shape[-2] - 2 * p, g.shape[-1] - 2 * p
        if H == 1:
            g = g.sum(-2, keepdim=True)
        else:
            g = torch.cat([g[..., :p + 1, :].sum(-2, keepdim=True), g[..., p + 1:p + H - 1, :], g[..., p + H - 1:, :].sum(-2, keepdim=True)], dim=-2)
        if W == 1:
            g = g.sum(-1, keepdim=True)
        else:
            g = torch.cat([g[..., :p + 1].sum(-1, keepdim=True), g[..., p + 1:p + W - 1], g[..., p + W - 1:].sum(-1, keepdim=True)], dim=-1)
        return g, None


_FIXED_ORDER_PAD = [False]


def set_reproducible_backward(on):
    """Fixed-order backward of the replication padding in front of the separable convolutions (train.py --resumable: a resumed run can
    only repeat the uninterrupted one if an update is a function of the state).  Off by default: ATen's form.  Returns the previous
    setting."""
    previous, _FIXED_ORDER_PAD[0] = _FIXED_ORDER_PAD[0], bool(on)
    return previous


def _replicate_pad(x, p):
    if _FIXED_ORDER_PAD[0] and x.requires_grad and torch.is_grad_enabled():
        return _ReplicatePadFixedOrder.apply(x, p)
    return F.pad(x, [p] * 4, mode='replicate')


def _up2(x):
    return upsample2x(x)


def create_basic_conv_block(num_layers, num_in_channels, num_out_channels):
    """tai.py:244-263: num_layers x (conv3x3 + ReLU); parameterised layers sit at indices 0, 2, 4, ..."""
    layers = []
    for i in range(num_layers):
        cin = num_in_channels if i == 0 else num_out_channels
        layers.append((2 * i, nn.Conv2d(cin, num_out_channels, 3, stride=1, padding=1)))
    return IndexedConvs(layers)


class KernelGeneratorBlock(IndexedConvs):
    """tai.py:266-286: num_layers x (conv3x3 + ReLU) ending in ks channels, bilinear x2, conv3x3 ks->ks (no
    activation).  Layer indices 0, 2, ..., 2(num_layers-1) and 2*num_layers + 1."""

    def __init__(self, num_layers, kf_dim, ks):
        layers = []
        for i in range(num_layers):
            cout = ks if i == num_layers - 1 else kf_dim * 2
            layers.append((2 * i, nn.Conv2d(kf_dim * 2, cout, 3, stride=1, padding=1)))
        layers.append((2 * num_layers + 1, nn.Conv2d(ks, ks, 3, stride=1, padding=1)))
        super().__init__(layers)

    def forward(self, x):
        convs = self.convs()
        x = _conv_relu_chain(x, convs[:-1])
        return conv_bias_act(_up2(x), convs[-1].weight, convs[-1].bias, 1, None).contiguous()


def create_1d_kernel_generator_block(num_layers, kf_dim, ks):
    return KernelGeneratorBlock(num_layers, kf_dim, ks)


class UpsampleBlock(IndexedConvs):
    """tai.py:334-346: bilinear x2 -> conv3x3 -> ReLU; the conv is layer index 1."""

    def __init__(self, cin, cout):
        super().__init__([(1, nn.Conv2d(cin, cout, 3, stride=1, padding=1))])

    def forward(self, x):
        c = self.convs()[0]
        return conv_bias_act(_up2(x), c.weight, c.bias, 1, 'relu')


def create_encoder_blocks(start_i, end_i, layers, if_dim, kf_dim):
    """tai.py:289-310."""
    blocks = []
    for i in range(start_i, end_i):
        cin = if_dim if i == start_i else kf_dim * (2 ** (i - 1))
        blocks.append(create_basic_conv_block(layers, cin, kf_dim * (2 ** i)))
    return blocks


def create_decoder_blocks(num_block, kf_dim, layers, rc_loc):
    """tai.py:313-348: block i maps kf*2^(num_block-i+1) -> kf*2^(num_block-i) (block 0 keeps its width); the
    upsample conv of block rc_loc-1 takes one extra (time-ratio) input channel."""
    deconv, upsample = [], []
    for i in range(num_block):
        c_out = kf_dim * 2 ** (num_block - i)
        c_in = c_out if i == 0 else kf_dim * 2 ** (num_block - i + 1)
        deconv.append(create_basic_conv_block(layers, c_in, c_out))
        upsample.append(UpsampleBlock(c_out + 1 if i == rc_loc - 1 else c_out, c_out))
    return deconv, upsample


class TAI(nn.Module):
    """Time-aware interpolation ("kernel") network, tai.py:123-237."""

    def __init__(self, gf_dim, ks, num_block, layers, kf_dim, rc_loc=4):
        super().__init__()
        assert layers >= 1, 'layers in per block should be no smaller than 1, but layers=[%d]' % layers
        assert num_block >= 4, '# blocks should be no less than 3, but num_block=%d' % num_block
        self.kf_dim, self.ks, self.layers, self.num_block = kf_dim, ks, layers, num_block
        self.rc_loc = rc_loc      # 4 for TAI (tai.py:152); -1 = never inject the time ratio (TWI, twi.py:162)
        self.moduleConv = nn.ModuleList(create_encoder_blocks(3, num_block, layers, gf_dim * 8 * 2, kf_dim))
        deconv, upsample = create_decoder_blocks(num_block - 1, kf_dim, layers, self.rc_loc)
        self.moduleDeconv = nn.ModuleList(deconv)
        self.moduleUpsample = nn.ModuleList(upsample)
        self.moduleVertical1 = create_1d_kernel_generator_block(layers, kf_dim, ks)
        self.moduleVertical2 = create_1d_kernel_generator_block(layers, kf_dim, ks)
        self.moduleHorizontal1 = create_1d_kernel_generator_block(layers, kf_dim, ks)
        self.moduleHorizontal2 = create_1d_kernel_generator_block(layers, kf_dim, ks)
        self.pad = int(math.floor(ks / 2.0))
        self.separableConvolution = SeparableConvolution.apply

    def forward(self, variableInput1, variableInput2, variableDyn1, variableDyn2, variableCont1, variableCont2,
                variableRes, ratio=0):
        """variableRes is indexable by 1 and 2 (the merged 1/2- and 1/4-resolution residuals); index 0 is never read."""
        nb = self.num_block
        x = (variableDyn1, variableDyn2, variableCont1, variableCont2)      # their concatenation, never materialised
        enc = []
        for i in range(nb - 3):
            conv = _conv_relu_chain(x, self.moduleConv[i].convs())
            enc.append(conv)
            x = F.avg_pool2d(conv, kernel_size=2, stride=2)
        for i in range(nb - 1):
            d = _conv_relu_chain(x, self.moduleDeconv[i].convs())
            if i == self.rc_loc - 1:
                if torch.is_tensor(ratio):      # one ratio per sample (time steps batched together)
                    rc = ratio.to(d.dtype).view(-1, 1, 1, 1).expand(d.shape[0], 1, d.shape[2], d.shape[3])
                else:
                    rc = d.new_full((d.shape[0], 1, d.shape[2], d.shape[3]), float(ratio))
                d = torch.cat([d, rc], dim=1)
            u = self.moduleUpsample[i](d)
            x = u + (enc[nb - 3 - i - 1] if i < nb - 3 else variableRes[nb - i - 1])
        dot1 = self.separableConvolution(_replicate_pad(variableInput1, self.pad), self.moduleVertical1(x),
                                         self.moduleHorizontal1(x), self.ks)
        dot2 = self.separableConvolution(_replicate_pad(variableInput2, self.pad), self.moduleVertical2(x),
                                         self.moduleHorizontal2(x), self.ks)
        return dot1, dot2


def bidirectional_inputs(preceding_frames, following_frames):
    """Content frames and gray difference frames of both temporal directions (tai.py:63-74; the same block opens
    twi.py, bi_sa.py and bi_twa.py): -> (diff_in, xt, diff_in_F, xt_F)."""
    xt = preceding_frames[:, -1]
    xt_F = following_frames[:, 0]
    gray_p = gray01(preceding_frames)
    diff_in = gray_p[:, 1:] - gray_p[:, :-1]
    gray_f = torch.flip(gray01(following_frames), dims=[1])
    diff_in_F = gray_f[:, 1:] - gray_f[:, :-1]
    return diff_in, xt, diff_in_F, xt_F


def generate_both_directions(generator, K, Fn, T, diff_in, xt, diff_in_F, xt_F, fuse=True):
    """The two shared-weight MC-Net passes (forward in time, backward in time), batched into one when K == F;
    the backward lists are returned already reversed into forward time order (tai.py:77-83)."""
    if fuse and K == Fn:
        B = xt.shape[0]
        pred, dyn, cont, res = generator(K, T, torch.cat([diff_in, diff_in_F], 0), torch.cat([xt, xt_F], 0))
        lo = lambda r: None if r is None else r[:B]        # (res[t][0] is None when the generator drops it: keep_res1)
        hi = lambda r: None if r is None else r[B:]
        fwd = ([p[:B] for p in pred], [d[:B] for d in dyn], [c[:B] for c in cont], [[lo(r) for r in rs] for rs in res])
        bwd = ([p[B:] for p in pred], [d[B:] for d in dyn], [c[B:] for c in cont], [[hi(r) for r in rs] for rs in res])
    else:
        fwd, bwd = generator(K, T, diff_in, xt), generator(Fn, T, diff_in_F, xt_F)
    return fwd, tuple(x[::-1] for x in bwd)


def middle_frame_weights(T):
    """w[t] = (t+1)/(T+1): weight of the FOLLOWING side at middle frame t (tai.py:90)."""
    return np.linspace(0, 1, num=T + 2).tolist()[1:-1]


class TAIFillInModel(nn.Module):
    """tai.py:14-120."""

    def __init__(self, gf_dim, c_dim, feature_size, ks, num_block=5, kf_dim=32, layers=3, forget_bias=1, bias=True):
        super().__init__()
        self.c_dim = c_dim
        self.conv_lstm_state_size = 8 * gf_dim
        self.generator = MCNet(gf_dim, c_dim, feature_size, forget_bias=forget_bias, bias=bias)
        self.generator.keep_res1 = False      # merge_residual1 is never evaluated (see above): res[t][0] has no reader
        self.merge_residual3 = Residual(gf_dim * 8, kf_dim * 4)
        self.merge_residual2 = Residual(gf_dim * 4, kf_dim * 2)
        self.merge_residual1 = Residual(gf_dim * 2, kf_dim * 1)   # in the checkpoint schema; output never consumed
        self.kernelnet = TAI(gf_dim, ks, num_block, layers, kf_dim)
        # outside MC-Net's recurrence: these layers may take the 4 x 4 Winograd tile at any width (conv_ops.mark_outside_recurrence)
        for m in (self.kernelnet, self.merge_residual1, self.merge_residual2, self.merge_residual3):
            mark_outside_recurrence(m)
        self.fuse_directions = True
        self.batch_time_steps = True
        self.merge_per_step = True
        self._ratio_cache = {}

    def _ratio_per_sample(self, T, B, w, device):
        """[T*B] fp32 time ratios 1 - w[t] (time-major), the values the per-step path passes as Python floats.  Cached per
        (T, B, device): built by a host-to-device copy, which must not happen inside a hipGraph capture (the eager warm-up
        that precedes every capture fills the cache)."""
        key = (T, B, str(device))
        if key not in self._ratio_cache:
            vals = np.repeat(np.array([1 - wt for wt in w], dtype=np.float64), B).astype(np.float32)
            self._ratio_cache[key] = torch.from_numpy(vals).to(device)
        return self._ratio_cache[key]

    def forward(self, T, preceding_frames, following_frames):
        K = preceding_frames.size(1)
        Fn = following_frames.size(1)
        diff_in, xt, diff_in_F, xt_F = bidirectional_inputs(preceding_frames, following_frames)
        (f_pred, f_dyn, f_cont, f_res), (b_pred, b_dyn, b_cont, b_res) = generate_both_directions(
            self.generator, K, Fn, T, diff_in, xt, diff_in_F, xt_F, fuse=self.fuse_directions)

        w = middle_frame_weights(T)
        if self.batch_time_steps:
            # The T kernel-network evaluations depend only on the finished MC-Net passes, not on each other: run them as
            # ONE batch of T*B (time-major), i.e. a fifth of the launches and larger MIOpen problems for the small maps.
            B = preceding_frames.shape[0]
            cat = lambda xs: torch.cat(list(xs), dim=0)
            # the merge blocks run per time step (their inputs are the largest tensors of the model: batching them would
            # mean copying ~1 GB into time-major stacks) and write straight into their slice of the time-major result
            merged = {}
            if not self.merge_per_step:
                merged = {1: self.merge_residual2(cat(r[1] for r in f_res), cat(r[1] for r in b_res)),
                          2: self.merge_residual3(cat(r[2] for r in f_res), cat(r[2] for r in b_res))}
            for idx, block in (((1, self.merge_residual2), (2, self.merge_residual3)) if self.merge_per_step else ()):
                r0 = f_res[0][idx]
                outc = block.res.convs()[-1].weight.shape[0]
                buf = r0.new_empty((T * B, outc) + tuple(r0.shape[2:]))
                for t in range(T):
                    block.forward_into(f_res[t][idx], b_res[t][idx], buf[t * B:(t + 1) * B])
                merged[idx] = buf
            ratio = self._ratio_per_sample(T, B, w, preceding_frames.device)
            dot1, dot2 = self.kernelnet(cat(f_pred).contiguous(), cat(b_pred).contiguous(), cat(f_dyn), cat(b_dyn),
                                        cat(f_cont), cat(b_cont), merged, ratio=ratio)
            blend = 0.5 * dot1 + 0.5 * dot2
            tb = lambda x: x.view(T, B, *x.shape[1:]).transpose(0, 1)
            return {
                'pred': tb(blend),
                'pred_forward': torch.stack(f_pred, dim=1),
                'pred_backward': torch.stack(b_pred, dim=1),
                'interp_net_outputs_1': tb(dot1),
                'interp_net_outputs_2': tb(dot2),
            }
        combination, out1, out2 = [], [], []
        for t in range(T):
            merged = {1: self.merge_residual2(f_res[t][1], b_res[t][1]),
                      2: self.merge_residual3(f_res[t][2], b_res[t][2])}
            dot1, dot2 = self.kernelnet(f_pred[t].contiguous(), b_pred[t].contiguous(), f_dyn[t], b_dyn[t], f_cont[t],
                                        b_cont[t], merged, ratio=1 - w[t])
            out1.append(dot1)
            out2.append(dot2)
            combination.append(0.5 * dot1 + 0.5 * dot2)

        return {
            'pred': torch.stack(combination, dim=1),
            'pred_forward': torch.stack(f_pred, dim=1),
            'pred_backward': torch.stack(b_pred, dim=1),
            'interp_net_outputs_1': torch.stack(out1, dim=1),
            'interp_net_outputs_2': torch.stack(out2, dim=1),
        }
