"""Image gradient difference loss (reference src/losses/losses.py:4-44, Mathieu et al.), and this build's opt-in losses: SSIMLoss
(train.py --ssim_weight), ImageLoss (train.py --image_loss l1 / charbonnier), LapLoss (train.py --lap_weight), TemporalLoss
(train.py --temporal_weight) and CensusLoss (train.py --census_weight), each a written definition with a HIP kernel behind it."""
import collections

import torch
import torch.nn as nn


class GDL(nn.Module):
    """L1 distance between the horizontal and vertical finite differences of prediction and target, each cropped to the
    common (H-1) x (W-1) window, summed; mean over everything when ``reduce`` (losses.py:30-43)."""

    def __init__(self, reduce=True):
        super().__init__()
        self.reduce = reduce

    def forward(self, input, target):
        B = input.size(0)
        H, W = input.shape[-2:]
        lead = input.shape[:-2]
        a = input.reshape(-1, H, W)
        b = target.reshape(-1, H, W)
        # d/dx (sign as in the reference: left minus right), rows 1..H-1;  d/dy (lower minus upper), cols 1..W-1
        dw = ((a[:, 1:, :-1] - a[:, 1:, 1:]) - (b[:, 1:, :-1] - b[:, 1:, 1:])).abs()
        dh = ((a[:, 1:, 1:] - a[:, :-1, 1:]) - (b[:, 1:, 1:] - b[:, :-1, 1:])).abs()
        loss = (dw + dh).reshape(*lead, H - 1, W - 1)
        return loss.reshape(B, -1).mean() if self.reduce else loss


def _ssim_planes(pred, gt):
    """S per window, [planes, 1, H-6, W-6] in float64, by torch ops (``avg_pool2d(7, 1)``): the definition of ``tai_ssim_loss``
    (include/tai_sepconv.h) up to the order of the window sums; differentiable by autograd."""
    import torch.nn.functional as F
    H, W = pred.shape[-2:]
    x = ((pred + 1) / 2).double().reshape(-1, 1, H, W)            # util.inverse_transform in the tensors' own precision, not clipped
    y = ((gt + 1) / 2).double().reshape(-1, 1, H, W)
    mean = lambda t: F.avg_pool2d(t, 7, 1)
    ux, uy, uxx, uyy, uxy = mean(x), mean(y), mean(x * x), mean(y * y), mean(x * y)
    c, C1, C2 = 49.0 / 48.0, 0.01 * 0.01, 0.03 * 0.03
    vx, vy, vxy = c * (uxx - ux * ux), c * (uyy - uy * uy), c * (uxy - ux * uy)
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


# What one fused loss hands to _FusedLoss: the entry's name; the arguments of its ``*_workspace_bytes`` query and (format, values) of the
# ValueError when that refuses them; how many float64 detail values and totals the launch writes; ``args(pred, gt, detail, totals, map,
# workspace, strides)`` -> the launch's argument list; ``views(detail, totals)`` -> what the call returns, the loss(es) first; ``table``:
# 1-3 predictions passed as pointer tables (else one, passed itself); ``strided``: tensors are read where they lie (_block_strides).
_Call = collections.namedtuple('_Call', 'entry query refused detail totals args views table strided', defaults=(False, False))


class _FusedLoss(torch.autograd.Function):
    """One launch of a fused loss+gradient entry on the current stream behind autograd.  ``call`` (a _Call) says what differs between the
    losses; the rest is here: one float64 tensor for detail and totals, the float64 workspace, and an fp32 gradient map in its prediction's
    layout for every prediction that needs a gradient when ``want_maps`` (inside Function.forward grad mode is always off and
    needs_input_grad ignores no_grad, so the caller passes its mode in).  The maps come from the same launch and are what ``backward``
    scales.  Every allocation is torch's, so under capture it comes from the graph's pool; nothing waits for the device."""

    @staticmethod
    def forward(ctx, call, want_maps, gt, *preds):
        import ctypes
        from . import _native
        n = len(preds)
        nbytes = getattr(_native.lib(), call.entry + '_workspace_bytes')(*call.query)
        if nbytes < 0:
            raise ValueError(call.refused[0] % call.refused[1])
        dev = gt.device
        tensors, strides = [], []
        for t in preds + (gt,):
            t = t.detach()
            where = _block_strides(t) if call.strided else None
            if where is None:
                t = t.contiguous()
                where = _block_strides(t) if call.strided else ()
            tensors.append(t)
            strides.extend(where)
        workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        out = torch.empty(call.detail + call.totals, dtype=torch.float64, device=dev)          # detail, then totals
        maps = [torch.empty_strided(p.shape, p.stride(), dtype=torch.float32, device=dev) if want_maps and ctx.needs_input_grad[3 + i] else None
                for i, p in enumerate(tensors[:n])]
        pred_arg, map_arg = tensors[0], maps[0]
        if call.table:
            pred_arg = (ctypes.c_void_p * n)(*[p.data_ptr() for p in tensors[:n]])
            map_arg = (ctypes.c_void_p * n)(*[m.data_ptr() if m is not None else None for m in maps])
        detail, totals = out[:call.detail], out[call.detail:]
        stride_table = (ctypes.c_longlong * len(strides))(*strides) if call.strided else None
        _native.launch(call.entry, dev, *call.args(pred_arg, tensors[n], detail, totals, map_arg, workspace, stride_table))
        ctx.maps = maps
        results = call.views(detail, totals)
        ctx.mark_non_differentiable(*results[1:])
        return results

    @staticmethod
    def backward(ctx, grad_losses, *_):
        one = grad_losses.dim() == 0
        return (None, None, None) + tuple(None if m is None else (grad_losses if one else grad_losses[i]) * m for i, m in enumerate(ctx.maps))


def _check_kind(what, kind):
    if kind not in IMAGE_LOSS_KINDS:
        raise ValueError('%s must be one of %s, found %r' % (what, ', '.join(IMAGE_LOSS_KINDS), kind))


def _check_eps(what, eps):
    if not (eps > 0.0 and eps != float('inf')):
        raise ValueError('%s must be finite and > 0, found %r' % (what, eps))


def _check_levels(what, levels):
    if not (isinstance(levels, int) and 1 <= levels <= LAP_MAX_LEVELS):
        raise ValueError('%s must be an integer from 1 to %d, found %r' % (what, LAP_MAX_LEVELS, levels))


def _kind_and_eps(name, kind, eps):
    """(kind, eps) of ImageLoss and TemporalLoss, checked."""
    _check_kind(name + ': kind', kind)
    eps = float(eps)
    _check_eps(name + ': eps', eps)
    return kind, eps


class LossSettings(collections.namedtuple('LossSettings', 'ssim_weight image_loss charbonnier_eps lap_weight lap_levels temporal_weight '
                                                          'temporal_kind temporal_eps census_weight',
                                          defaults=(0.0, 'l2', 1e-3, 0.0, 5, 0.0, 'charbonnier', 1e-3, 0.0))):
    """train.py's loss flags, each field under its flag's name; the defaults are the reference's loss.  What
    ``environments.create_training_environment`` takes as ``losses``."""
    __slots__ = ()

    @classmethod
    def from_options(cls, opt):
        return cls(*(getattr(opt, field) for field in cls._fields))

    def check(self):
        """Raises ValueError naming the flag whose value is refused."""
        for flag in ('ssim_weight', 'lap_weight', 'temporal_weight'):
            if not getattr(self, flag) >= 0.0:
                raise ValueError('--%s must not be negative, found %r' % (flag, getattr(self, flag)))
        if not (self.census_weight >= 0.0 and self.census_weight != float('inf')):
            raise ValueError('--census_weight must be finite and not negative, found %r' % (self.census_weight,))
        _check_kind('--image_loss', self.image_loss)
        _check_eps('--charbonnier_eps', self.charbonnier_eps)
        if self.lap_weight > 0.0:                                 # the levels of a pyramid that is not built are not looked at
            _check_levels('--lap_levels', self.lap_levels)
        _check_kind('--temporal_kind', self.temporal_kind)
        _check_eps('--temporal_eps', self.temporal_eps)


def _predictions(name, preds):
    """(single, tuple of 1-3 predictions) of what ImageLoss, TemporalLoss and CensusLoss take: one tensor or a tuple."""
    single = torch.is_tensor(preds)
    preds = (preds,) if single else tuple(preds)
    if not 1 <= len(preds) <= 3:
        raise ValueError('%s: takes 1 to 3 predictions, got %d' % (name, len(preds)))
    return single, preds


class SSIMLoss(nn.Module):
    """1 - mean SSIM of prediction against target, the definition of ``tai_ssim_loss`` (include/tai_sepconv.h): frames mapped to [0, 1]
    in fp32 and NOT clipped, 7x7 uniform window over the valid interior, L = 1, float64 window arithmetic, mean over every plane of
    ``[..., C, H, W]`` (any leading dimensions).  CUDA fp32 tensors go through the HIP kernel, which writes the loss and its gradient
    map in one launch; anything else (CPU, float64) evaluates the same definition with torch ops and is differentiated by autograd.
    ``plane_ssim`` keeps the last call's per-plane values (float64, detached).  No parameters, no buffers."""

    def __init__(self):
        super().__init__()
        self.plane_ssim = None

    def forward(self, input, target):
        if input.shape != target.shape or input.dim() < 3:
            raise ValueError('SSIMLoss: input %s and target %s must have one shape [..., C, H, W]'
                             % (tuple(input.shape), tuple(target.shape)))
        H, W = input.shape[-2:]
        if H < 7 or W < 7 or input.numel() == 0:
            raise ValueError('SSIMLoss: needs at least one plane and H, W >= 7 (the 7x7 window), got %s' % (tuple(input.shape),))
        if input.is_cuda and input.dtype == torch.float32 and target.is_cuda and target.dtype == torch.float32:
            C = input.shape[-3]
            N = input.numel() // (C * H * W)
            call = _Call('tai_ssim_loss', (N, C, H, W), ('SSIMLoss: [%d, %d, %d, %d] is outside what tai_ssim_loss takes', (N, C, H, W)), N * C, 2,
                         lambda p, g, planes, totals, m, ws, _: (p, g, planes, totals, m, ws, N, C, H, W),
                         lambda planes, totals: (totals[1].to(torch.float32), planes))                     # totals: mean_ssim and loss
            loss, planes = _FusedLoss.apply(call, True, target, input)                 # (a map whenever the input requires grad, whatever the mode)
            self.plane_ssim = planes.detach()
            return loss
        S = _ssim_planes(input, target.to(device=input.device, dtype=input.dtype))
        planes = S.mean(dim=(1, 2, 3))
        self.plane_ssim = planes.detach()
        return (1.0 - planes.mean()).to(input.dtype)


IMAGE_LOSS_KINDS = ('l2', 'l1', 'charbonnier')          # kind 0, 1, 2 of tai_image_loss


def _image_loss_terms(pred, gt, kind, eps):
    """(point, gdl, plane_terms [P, 2]) in float64 by torch ops, differentiable by autograd: the definition of ``tai_image_loss``
    (include/tai_sepconv.h) up to the order of the sums; the element-wise terms are formed in the tensors' own precision."""
    H, W = pred.shape[-2:]
    x = ((pred + 1) / 2).reshape(-1, H, W)                        # util.inverse_transform, not clipped
    y = ((gt + 1) / 2).reshape(-1, H, W)
    P = x.shape[0]
    d = x - y
    if kind == 0:
        rho = d * d
    elif kind == 1:
        rho = d.abs()                                             # autograd's derivative is sign(d): 0 at 0
    else:
        e = torch.tensor(eps, dtype=pred.dtype)
        rho = torch.sqrt(d * d + float(e * e))
    gw = ((x[:, 1:, :-1] - x[:, 1:, 1:]) - (y[:, 1:, :-1] - y[:, 1:, 1:])).abs()          # losses.GDL's operand order
    gh = ((x[:, 1:, 1:] - x[:, :-1, 1:]) - (y[:, 1:, 1:] - y[:, :-1, 1:])).abs()
    plane_point = rho.double().sum(dim=(1, 2))
    plane_gdl = gw.double().sum(dim=(1, 2)) + gh.double().sum(dim=(1, 2))
    point = plane_point.sum() / (float(P) * H * W)
    gdl = plane_gdl.sum() / (float(P) * (H - 1) * (W - 1))
    return point, gdl, torch.stack([plane_point, plane_gdl], dim=1)


class ImageLoss(nn.Module):
    """Pointwise term + gradient-difference term of 1-3 predictions against one target, the definition of ``tai_image_loss``
    (include/tai_sepconv.h): frames mapped to [0, 1] as ``inverse_transform`` does and NOT clipped; the point term is the mean of d^2
    (``l2``), |d| (``l1``) or sqrt(d^2 + eps^2) (``charbonnier``) and the other the mean of ``GDL``'s |gw| + |gh| over the (H-1) x (W-1)
    window, both over every plane of ``[..., H, W]`` (any leading dimensions, in the tensors' own layout).  ``forward(preds, target)``
    takes one tensor or a tuple of 1-3 and returns one scalar ``point + gdl`` per prediction (a tuple for a tuple).  CUDA fp32 tensors go
    through ONE launch of the HIP kernel for all predictions, which writes the losses and their gradient maps; anything else (CPU,
    float64) evaluates the same definition with torch ops and is differentiated by autograd.  ``last_terms`` keeps the last call's
    (point, gdl) per prediction and ``plane_terms`` its per-plane sums [n, P, 2] (float64), detached.  No parameters, no buffers."""

    def __init__(self, kind='charbonnier', eps=1e-3):
        super().__init__()
        self.kind, self.eps = _kind_and_eps('ImageLoss', kind, eps)
        self.last_terms = None
        self.plane_terms = None

    def forward(self, preds, target):
        single, preds = _predictions('ImageLoss', preds)
        for p in preds:
            if p.shape != target.shape or p.dim() < 2:
                raise ValueError('ImageLoss: prediction %s and target %s must have one shape [..., H, W]' % (tuple(p.shape), tuple(target.shape)))
        H, W = target.shape[-2:]
        if H < 2 or W < 2 or target.numel() == 0:
            raise ValueError('ImageLoss: needs at least one plane and H, W >= 2 (the gradient-difference term), got %s' % (tuple(target.shape),))
        kind = IMAGE_LOSS_KINDS.index(self.kind)
        if all(t.is_cuda and t.dtype == torch.float32 for t in preds + (target,)):
            n, P, eps = len(preds), target.numel() // (H * W), self.eps

            def views(planes, totals):                                                  # totals: (point, gdl, loss) per prediction
                t32 = totals.view(n, 3).to(torch.float32)
                return t32[:, 2].contiguous(), t32[:, :2], planes.view(n, P, 2)
            call = _Call('tai_image_loss', (n, P, H, W),
                         ('ImageLoss: %d predictions of %d planes of %d x %d are outside what tai_image_loss takes', (n, P, H, W)), n * P * 2, n * 3,
                         lambda ps, g, planes, totals, ms, ws, _: (ps, n, g, kind, eps, planes, totals, ms, ws, P, H, W), views, table=True)
            losses, terms, planes = _FusedLoss.apply(call, torch.is_grad_enabled(), target, *preds)
            self.last_terms = [(terms[i, 0], terms[i, 1]) for i in range(len(preds))]
            self.plane_terms = planes
            out = tuple(losses[i] for i in range(len(preds)))
        else:
            out, self.last_terms, planes = [], [], []
            for p in preds:
                point, gdl, pt = _image_loss_terms(p, target.to(device=p.device, dtype=p.dtype), kind, self.eps)
                out.append((point + gdl).to(p.dtype))
                self.last_terms.append((point.detach().to(p.dtype), gdl.detach().to(p.dtype)))
                planes.append(pt.detach())
            self.plane_terms = torch.stack(planes)
            out = tuple(out)
        return out[0] if single else out


LAP_MAX_LEVELS = 6              # tai_lap_loss: up to here every value of the gradient's adjoint pyramid is exact in float64


def _lap_check(shape, levels):
    H, W = shape[-2:]
    if min(H, W) < 2 ** (levels - 1) or min(shape) == 0:
        raise ValueError('LapLoss: %d levels need at least one plane with H, W >= %d, got %s' % (levels, 2 ** (levels - 1), tuple(shape)))


def _lap_reduce_axis(g, axis):
    """One pass of D along ``axis``: out[i] = sum_{a=0..4} k[a] g[clamp(2i + a - 2)], k = (1, 4, 6, 4, 1) / 16, left to right."""
    n = g.shape[axis]
    base = 2 * torch.arange((n + 1) // 2, device=g.device)
    acc = None
    for a, k in enumerate((1.0 / 16.0, 4.0 / 16.0, 6.0 / 16.0, 4.0 / 16.0, 1.0 / 16.0)):
        term = k * g.index_select(axis, (base + (a - 2)).clamp(0, n - 1))
        acc = term if acc is None else acc + term
    return acc


def _lap_expand_axis(g, n, axis):
    """One pass of U along ``axis``, from ceil(n/2) entries to n: even 2i = (g[i-1]/8 + 6 g[i]/8) + g[i+1]/8, odd 2i+1 = g[i]/2 +
    g[i+1]/2, indices clamped."""
    m = g.shape[axis]
    i = torch.arange(m, device=g.device)
    before, after = g.index_select(axis, (i - 1).clamp(0, m - 1)), g.index_select(axis, (i + 1).clamp(0, m - 1))
    even = (before / 8.0 + (6.0 * g) / 8.0) + after / 8.0
    odd = (g / 2.0 + after / 2.0).narrow(axis, 0, n // 2)
    if n == 2 * m:
        return torch.stack([even, odd], dim=axis + 1).flatten(axis, axis + 1)
    head = torch.stack([even.narrow(axis, 0, m - 1), odd], dim=axis + 1).flatten(axis, axis + 1)
    return torch.cat([head, even.narrow(axis, m - 1, 1)], dim=axis)


class _DivideGradient(torch.autograd.Function):
    """Identity whose backward divides by ``count``.  It puts the loss's 1 / (P H W) behind the adjoint sums, as the definition does:
    those sums are then exact in float64 and the gradient is rounded once."""

    @staticmethod
    def forward(ctx, x, count):
        ctx.count = count
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g / ctx.count, None


class _DivideValue(torch.autograd.Function):
    """``x / count`` whose backward passes the gradient through: the other half of ``_DivideGradient``."""

    @staticmethod
    def forward(ctx, x, count):
        return x / count

    @staticmethod
    def backward(ctx, g):
        return g, None


def _lap_terms(pred, gt, levels):
    """(loss, terms [L], plane_terms [P, L]) in float64 by torch ops, differentiable by autograd: the definition of ``tai_lap_loss``
    (include/tai_sepconv.h), element-wise operations in its order; only the order of the sums of |L_l| is torch's."""
    H, W = pred.shape[-2:]
    d = (((pred + 1) / 2) - ((gt + 1) / 2)).reshape(-1, H, W)     # util.inverse_transform in the tensors' own precision, not clipped
    P = d.shape[0]
    count = (float(P) * float(H)) * float(W)
    G = [_DivideGradient.apply(d.double(), count)]
    for _ in range(1, levels):
        G.append(_lap_reduce_axis(_lap_reduce_axis(G[-1], 1), 2))
    plane_terms = []
    for l in range(levels):
        L = G[l]
        if l < levels - 1:
            L = L - _lap_expand_axis(_lap_expand_axis(G[l + 1], G[l].shape[1], 1), G[l].shape[2], 2)
        plane_terms.append(L.abs().sum(dim=(1, 2)))               # autograd's derivative is sign(L): 0 at 0
    plane_terms = torch.stack(plane_terms, dim=1)
    terms = torch.stack([_DivideValue.apply(2.0 ** l * plane_terms[:, l].sum(), count) for l in range(levels)])
    loss = terms[0]
    for l in range(1, levels):
        loss = loss + terms[l]
    return loss, terms, plane_terms


class LapLoss(nn.Module):
    """L1 distance between the Laplacian pyramids of prediction and target, the definition of ``tai_lap_loss`` (include/tai_sepconv.h):
    frames mapped to [0, 1] as ``inverse_transform`` does and NOT clipped, ``levels`` levels (1..6) of the 5-tap binomial pyramid with
    replicated edges built on the difference in float64, level l weighted 2^l, summed and divided by the number of full-resolution pixels
    of every plane of ``[..., H, W]`` (any leading dimensions, in the tensors' own layout); ``levels = 1`` is the mean of |d|.  CUDA fp32
    tensors go through the HIP kernel, which writes the loss and its gradient map in one launch; anything else (CPU, float64) evaluates
    the same definition with torch ops and is differentiated by autograd.  ``last_terms`` keeps the last call's per-level terms [L] and
    ``plane_terms`` its per-plane sums of |L_l| [P, L] (float64), detached.  No parameters, no buffers."""

    def __init__(self, levels=5):
        super().__init__()
        _check_levels('LapLoss: levels', levels)
        self.levels = levels
        self.last_terms = None
        self.plane_terms = None

    def forward(self, input, target):
        if input.shape != target.shape or input.dim() < 2:
            raise ValueError('LapLoss: input %s and target %s must have one shape [..., H, W]' % (tuple(input.shape), tuple(target.shape)))
        _lap_check(input.shape, self.levels)
        if input.is_cuda and input.dtype == torch.float32 and target.is_cuda and target.dtype == torch.float32:
            (H, W), levels = input.shape[-2:], self.levels
            P = input.numel() // (H * W)

            def views(planes, totals):                                                  # totals: the terms, then the loss
                t32 = totals.to(torch.float32)
                return t32[levels].clone(), t32[:levels], planes.view(P, levels)
            call = _Call('tai_lap_loss', (P, H, W, levels),
                         ('LapLoss: %d planes of %d x %d with %d levels are outside what tai_lap_loss takes', (P, H, W, levels)), P * levels, levels + 1,
                         lambda p, g, planes, totals, m, ws, _: (p, g, levels, planes, totals, m, ws, P, H, W), views)
            loss, terms, planes = _FusedLoss.apply(call, torch.is_grad_enabled(), target, input)
            self.last_terms, self.plane_terms = terms.detach(), planes.detach()
            return loss
        loss, terms, planes = _lap_terms(input, target.to(device=input.device, dtype=input.dtype), self.levels)
        self.last_terms, self.plane_terms = terms.detach().to(input.dtype), planes.detach()
        return loss.to(input.dtype)


def _temporal_terms(pred, gt, kind, eps):
    """(loss, terms [T + 1], seq_terms [B * C, T + 1]) in float64 by torch ops, differentiable by autograd: the definition of
    ``tai_temporal_loss`` (include/tai_sepconv.h) up to the order of the sums; the element-wise terms are formed in the tensors' own
    precision."""
    B, T, C, H, W = pred.shape
    e = (pred + 1) / 2 - (gt + 1) / 2                             # util.inverse_transform, not clipped
    known = torch.zeros_like(e[:, :1])                            # e_{-1} = e_T = 0: the known frames on both sides of the gap
    e = torch.cat([known, e, known], dim=1)
    d = e[:, 1:] - e[:, :-1]                                      # d_0 .. d_T
    if kind == 0:
        rho = d * d
    elif kind == 1:
        rho = d.abs()                                             # autograd's derivative is sign(d): 0 at 0
    else:
        import numpy as np
        e2 = float(np.float32(eps) * np.float32(eps))             # the definition's constant: eps * eps in fp32, in either precision
        # the square root is taken in float64 and rounded to the tensors' precision: correctly rounded, as the definition asks (53 bits
        # are more than twice 24 plus 2, so the second rounding cannot move it), which torch's fp32 square root on the host is not
        rho = torch.sqrt((d * d + e2).double()).to(pred.dtype)
    seq_terms = rho.double().sum(dim=(3, 4)).permute(0, 2, 1).reshape(B * C, T + 1)
    n_pos = float(B * C) * H * W
    return seq_terms.sum() / (n_pos * (T + 1)), seq_terms.sum(dim=0) / n_pos, seq_terms


def _block_strides(t):
    """(batch stride, time stride) in elements if ``t`` [B, T, C, H, W] can be read where it lies by ``tai_temporal_loss`` and
    ``tai_census_loss``: every
    [C, H, W] block dense, the (b, t) blocks apart from each other with one axis nested in the other; else None."""
    B, T, C, H, W = t.shape
    sb, st, sc, sh, sw = t.stride()
    if (W > 1 and sw != 1) or (H > 1 and sh != W) or (C > 1 and sc != H * W):
        return None
    chw = C * H * W
    if B == 1 and T == 1:
        return chw, chw
    if B == 1:
        return (T * st, st) if st >= chw else None
    if T == 1:
        return (sb, B * sb) if sb >= chw else None
    if (st >= chw and sb >= (T - 1) * st + chw) or (sb >= chw and st >= (B - 1) * sb + chw):
        return sb, st
    return None


class TemporalLoss(nn.Module):
    """Temporal-difference loss of 1-3 predictions ``[B, T, C, H, W]`` against one target, the definition of ``tai_temporal_loss``
    (include/tai_sepconv.h): frames mapped to [0, 1] as ``inverse_transform`` does and NOT clipped, e_t the error of frame t and zero on
    the known frames on both sides of the gap, d_j = e_j - e_{j-1} for j = 0..T, and the loss the mean over the T + 1 positions and every
    pixel of d^2 (``l2``), |d| (``l1``) or sqrt(d^2 + eps^2) (``charbonnier``): an error that stays constant through the gap is counted
    at the two seams only, one that changes from frame to frame at every position.  ``forward(preds, target)`` takes one tensor or a tuple
    of 1-3 and returns one scalar per prediction (a tuple for a tuple).  CUDA fp32 tensors go through ONE launch of the HIP kernel for all
    predictions, which reads every tensor in its own layout and writes the losses and their gradient maps; anything else (CPU, float64)
    evaluates the same definition with torch ops and is differentiated by autograd.  ``last_terms`` keeps the last call's per-position
    means [n, T + 1] and ``seq_terms`` its per-sequence sums [n, B * C, T + 1] (float64), detached.  No parameters, no buffers."""

    def __init__(self, kind='charbonnier', eps=1e-3):
        super().__init__()
        self.kind, self.eps = _kind_and_eps('TemporalLoss', kind, eps)
        self.last_terms = None
        self.seq_terms = None

    def forward(self, preds, target):
        single, preds = _predictions('TemporalLoss', preds)
        for p in preds:
            if p.shape != target.shape or p.dim() != 5:
                raise ValueError('TemporalLoss: prediction %s and target %s must have one shape [B, T, C, H, W]'
                                 % (tuple(p.shape), tuple(target.shape)))
        if target.numel() == 0:
            raise ValueError('TemporalLoss: needs at least one pixel, got %s' % (tuple(target.shape),))
        kind = IMAGE_LOSS_KINDS.index(self.kind)
        if all(t.is_cuda and t.dtype == torch.float32 for t in preds + (target,)):
            n, eps, (B, T, C, H, W) = len(preds), self.eps, target.shape
            S = B * C

            def views(seqs, totals):                                                    # totals: the T + 1 position means, then the loss
                t32 = totals.view(n, T + 2).to(torch.float32)
                return t32[:, T + 1].contiguous(), t32[:, :T + 1], seqs.view(n, S, T + 1)
            call = _Call('tai_temporal_loss', (n, B, T, C, H, W),
                         ('TemporalLoss: %d predictions of %s are outside what tai_temporal_loss takes', (n, tuple(target.shape))),
                         n * S * (T + 1), n * (T + 2),
                         lambda ps, g, seqs, totals, ms, ws, strides: (ps, n, g, strides, kind, eps, seqs, totals, ms, ws, B, T, C, H, W),
                         views, table=True, strided=True)
            losses, terms, seqs = _FusedLoss.apply(call, torch.is_grad_enabled(), target, *preds)
            self.last_terms, self.seq_terms = terms.detach(), seqs.detach()
            out = tuple(losses[i] for i in range(len(preds)))
        else:
            out, terms, seqs = [], [], []
            for p in preds:
                loss, tm, sq = _temporal_terms(p, target.to(device=p.device, dtype=p.dtype), kind, self.eps)
                out.append(loss.to(p.dtype))
                terms.append(tm.detach().to(p.dtype))
                seqs.append(sq.detach())
            self.last_terms, self.seq_terms = torch.stack(terms), torch.stack(seqs)
            out = tuple(out)
        return out[0] if single else out


_CENSUS_GRAY = (0.1140, 0.5870, 0.2989)         # util.gray01's weights, in its operand order


def _census_terms(pred, gt):
    """(loss, frame_terms [B * T]) in float64 by torch ops, differentiable by autograd: the definition of ``tai_census_loss``
    (include/tai_sepconv.h) with the range map in the tensors' own precision and everything behind it in float64 (the constants are the
    definition's fp32 ones, widened)."""
    B, T, C, H, W = pred.shape
    f = lambda v: float(torch.tensor(v, dtype=torch.float32))

    def gray(frames):
        x = ((frames + 1) / 2).double()                           # util.inverse_transform, not clipped
        if C == 1:
            return x[:, :, 0]
        return (f(_CENSUS_GRAY[0]) * x[:, :, 0] + f(_CENSUS_GRAY[1]) * x[:, :, 1]) + f(_CENSUS_GRAY[2]) * x[:, :, 2]

    def soft_sign(I, dy, dx):                                     # t of every interior pixel for one offset
        s = 255.0 * (I[:, :, 3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] - I[:, :, 3:H - 3, 3:W - 3])
        return s / torch.sqrt(f(0.81) + s * s)
    I, J = gray(pred), gray(gt)
    phi_sum = None
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            if dy == 0 and dx == 0:
                continue
            d = soft_sign(I, dy, dx) - soft_sign(J, dy, dx)
            e = d * d
            phi = e / (f(0.1) + e)
            phi_sum = phi if phi_sum is None else phi_sum + phi
    frame_terms = (phi_sum / 49.0).sum(dim=(2, 3)).reshape(B * T) / float((H - 6) * (W - 6))
    return frame_terms.sum() / float(B * T), frame_terms


class CensusLoss(nn.Module):
    """Census (soft ternary) loss of 1-3 predictions ``[B, T, C, H, W]`` (C 1 or 3; H, W >= 7) against one target, the definition of
    ``tai_census_loss`` (include/tai_sepconv.h): frames mapped to [0, 1] as ``inverse_transform`` does and NOT clipped, gray for C = 3; per
    interior pixel and each of its 48 neighbours in the 7x7 window the softened sign t = s / sqrt(0.81 + s^2) of the 255-scaled intensity
    difference s, and the distance d^2 / (0.1 + d^2) between prediction's and target's t, averaged over the window's 49 positions, the
    interior and the frames.  A constant added to a frame changes no difference, so it costs nothing.  ``forward(preds, target)`` takes one
    tensor or a tuple of 1-3 and returns one scalar per prediction (a tuple for a tuple).  CUDA fp32 tensors go through ONE launch of the
    HIP kernel for all predictions, which reads every tensor in its own layout and writes the losses and their gradient maps; anything
    else (CPU, float64) evaluates the same definition with torch ops in float64 and is differentiated by autograd.  ``frame_terms`` keeps
    the last call's per-frame means [n, B * T] (float64), detached.  No parameters, no buffers."""

    def __init__(self):
        super().__init__()
        self.frame_terms = None

    def forward(self, preds, target):
        single, preds = _predictions('CensusLoss', preds)
        for p in preds:
            if p.shape != target.shape or p.dim() != 5:
                raise ValueError('CensusLoss: prediction %s and target %s must have one shape [B, T, C, H, W]'
                                 % (tuple(p.shape), tuple(target.shape)))
        B, T, C, H, W = target.shape
        if C not in (1, 3) or H < 7 or W < 7 or target.numel() == 0:
            raise ValueError('CensusLoss: needs at least one frame, C in {1, 3} and H, W >= 7 (the 7x7 window), got %s' % (tuple(target.shape),))
        if all(t.is_cuda and t.dtype == torch.float32 for t in preds + (target,)):
            n = len(preds)
            call = _Call('tai_census_loss', (n, B, T, C, H, W),
                         ('CensusLoss: %d predictions of %s are outside what tai_census_loss takes', (n, tuple(target.shape))), n * B * T, n,
                         lambda ps, g, frames, totals, ms, ws, strides: (ps, n, g, strides, frames, totals, ms, ws, B, T, C, H, W),
                         lambda frames, totals: (totals.to(torch.float32), frames.view(n, B * T)), table=True, strided=True)
            losses, frames = _FusedLoss.apply(call, torch.is_grad_enabled(), target, *preds)
            self.frame_terms = frames.detach()
            out = tuple(losses[i] for i in range(n))
        else:
            out, frames = [], []
            for p in preds:
                loss, ft = _census_terms(p, target.to(device=p.device, dtype=p.dtype))
                out.append(loss.to(p.dtype))
                frames.append(ft.detach())
            self.frame_terms = torch.stack(frames)
            out = tuple(out)
        return out[0] if single else out
