"""Image gradient difference loss (reference src/losses/losses.py:4-44, Mathieu et al.)."""
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


class _SSIMLossFunction(torch.autograd.Function):
    """``tai_ssim_loss`` on the current stream: (loss fp32 scalar, plane_ssim float64 [planes]); the gradient map comes from the same
    launch and is what ``backward`` scales.  Every allocation is torch's, so under capture it comes from the graph's pool."""

    @staticmethod
    def forward(ctx, pred, gt):
        from . import _native
        C, H, W = pred.shape[-3:]
        N = pred.numel() // (C * H * W)
        L = _native.lib()
        nbytes = L.tai_ssim_loss_workspace_bytes(N, C, H, W)
        if nbytes < 0:
            raise ValueError('SSIMLoss: [%d, %d, %d, %d] is outside what tai_ssim_loss takes' % (N, C, H, W))
        dev = pred.device
        p, g = pred.detach().contiguous(), gt.detach().contiguous()
        workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        out = torch.empty(N * C + 2, dtype=torch.float64, device=dev)          # plane_ssim, then mean_ssim and loss
        grad = torch.empty(pred.shape, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _native.check(L.tai_ssim_loss(p.data_ptr(), g.data_ptr(), out.data_ptr(), out[N * C:].data_ptr(),
                                          grad.data_ptr() if grad is not None else None, workspace.data_ptr(), N, C, H, W, stream),
                          'tai_ssim_loss')
        ctx.map = grad
        plane_ssim = out[:N * C]
        ctx.mark_non_differentiable(plane_ssim)
        return out[N * C + 1].to(torch.float32), plane_ssim

    @staticmethod
    def backward(ctx, grad_loss, _grad_planes):
        return (grad_loss * ctx.map if ctx.map is not None else None), None


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
            loss, planes = _SSIMLossFunction.apply(input, target)
            self.plane_ssim = planes.detach()
            return loss
        S = _ssim_planes(input, target.to(device=input.device, dtype=input.dtype))
        planes = S.mean(dim=(1, 2, 3))
        self.plane_ssim = planes.detach()
        return (1.0 - planes.mean()).to(input.dtype)
