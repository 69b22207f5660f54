"""Convolution + bias + activation as the generator uses it (reference: nn.Conv2d / nn.ConvTranspose2d followed by
nn.ReLU, nn.Tanh or nothing).  Inference on the GPU runs the bias-free MIOpen convolution and finishes it with the
single-pass HIP bias+activation kernel of the C ABI (ATen would add the bias and apply the ReLU in two more full passes);
anything that needs autograd, and CPU tensors, take the stock PyTorch ops -- same arithmetic, one rounding per add."""
import ctypes

import torch
import torch.nn.functional as F

from . import _native

_ACT = {None: 0, 'relu': 1, 'tanh': 2}


def _finish(y, bias, act):
    if act == 'relu':
        return torch.relu(y + bias.view(1, -1, 1, 1)) if bias is not None else torch.relu(y)
    if act == 'tanh':
        return torch.tanh(y + bias.view(1, -1, 1, 1)) if bias is not None else torch.tanh(y)
    return y + bias.view(1, -1, 1, 1) if bias is not None else y


def _as_conv_weight(weight, transposed):
    # ConvTranspose2d(cin, cout, 3, stride 1, padding 1)  ==  conv2d with weight[o, i, ky, kx] = wt[i, o, 2-ky, 2-kx]
    return weight.transpose(0, 1).flip(2, 3) if transposed else weight


_EPOCH = [0]


def invalidate_derived(module=None):
    """Drop the cached derived weights (Winograd-domain U, direct-conv layout of a transposed conv) of ``module``'s
    parameters, or of every weight when ``module`` is None.  The cache notices writes that move the tensor's version
    counter (optimizer steps, ``load_state_dict``, ``with torch.no_grad(): p.mul_(2)``) by itself; a write through
    ``p.data`` moves neither the counter nor the pointer (``p.data.normal_()``, ``dist.broadcast(p.data, ...)``, a user's
    EMA or clipping), and neither does a kernel or a numpy view that is handed the weight's raw pointer, so whoever writes
    that way calls this afterwards -- ``parallel.broadcast_module_state``, the environments' ``load``, a replayed captured
    update (``train_step``), ``fused_step.averaged_weights`` and ``FusedStep.step`` do: the fused optimizer step
    (``tai_fused_step`` on the device, ``host_step`` on numpy views) is a raw-pointer writer and drops the forms of the module it
    stepped after every launch, whatever the device-side verdict (tests/derived_cases.py lists the writers and the forms)."""
    if module is None:
        _EPOCH[0] += 1
        return
    for p in module.parameters():
        if hasattr(p, '_tai_derived'):
            p._tai_derived.clear()


WINOGRAD_ARITHMETICS = {'fp32': 0, 'bf16x3': 1}
_WINO_ARITH = [0]          # mirrors the library's mode: part of the cache tag of every F(2x2, 3x3) transformed-weight buffer


def set_winograd_arithmetic(name):
    """Arithmetic of the Winograd 3x3 GEMMs (``tai_conv3x3_wino_set_arithmetic``): ``'fp32'`` (default: the fp32 MFMA, the
    reference's arithmetic class and the one every parity statement is made on) or ``'bf16x3'`` (opt-in: every fp32 operand
    as three bf16 terms, six bf16 products per product, fp32 accumulation -- csrc/wino_split.hip.inc).  The transformed
    weights of the two arithmetics are cached side by side (the arithmetic is part of the cache tag), so a hipGraph captured
    before a switch keeps replaying the arithmetic it was captured with ON BUFFERS THAT STAY ALIVE (the switch used
    to drop the other arithmetic's buffers, which a captured graph would then have read after free).  Returns the previous name."""
    mode = WINOGRAD_ARITHMETICS[name]
    prev = _native.lib().tai_conv3x3_wino_set_arithmetic(mode)
    if prev < 0:
        raise ValueError(name)
    _WINO_ARITH[0] = mode
    return [k for k, v in WINOGRAD_ARITHMETICS.items() if v == prev][0]


def get_winograd_arithmetic():
    mode = _native.lib().tai_conv3x3_wino_get_arithmetic()
    return [k for k, v in WINOGRAD_ARITHMETICS.items() if v == mode][0]


CONV_PRECISIONS = ('fp32', 'bf16')
_CONV_PREC = ['fp32']


def set_conv_precision(name):
    """Precision of the inference convolutions, process-wide: ``'fp32'`` (default: the routes and bits of before) or ``'bf16'``
    (opt-in, inference only): every layer _bf16_ok takes -- C >= 16 and K >= 16, k in {3, 5, 7}, stride 1, padding k // 2, the
    stride-1 ConvTranspose2d included -- computes act(bias + sum bf16(x) bf16(w)) on csrc/conv_bf16.hip.inc (operands rounded to
    nearest even, products exact, fp32 sums in an order fixed by the layer's shape).  Where autograd needs a gradient every path
    runs as in fp32 mode.  With set_winograd_arithmetic('bf16x3') as well, that arithmetic applies only to the layers the bf16
    kernel does not take.  A hipGraph captured before a switch keeps replaying what it captured: the packed bf16 weights are
    cached beside the fp32 ones.  Returns the previous name."""
    if name not in CONV_PRECISIONS:
        raise ValueError(name)
    prev, _CONV_PREC[0] = _CONV_PREC[0], name
    return prev


def get_conv_precision():
    return _CONV_PREC[0]


def _bf16_ok(Ci, Co, k, padding):
    """Does the bf16 kernel take this layer (in 'bf16' mode)?  A rule on the weight alone -- never on N, H, W or a grid -- so one
    CPU emulation states what the GPU computes and an image's arithmetic does not depend on its batch."""
    return Ci >= 16 and Co >= 16 and k in (3, 5, 7) and padding == k // 2


def _bf16_route(Ci, Co, kh, kw, padding, *tensors):
    """bf16 mode, a no-grad call and a layer _bf16_ok takes"""
    return _CONV_PREC[0] == 'bf16' and kh == kw and _bf16_ok(Ci, Co, kh, padding) and _no_grad_needed(*tensors)


def _bf16_weights(weight, transposed):
    """The packed bf16 weights of tai_conv_bf16_forward (tai_conv_bf16_pack_weights folds in a ConvTranspose2d's transpose and flip)."""
    def make():
        w = weight.detach().contiguous()
        k = w.shape[2]
        K, C = (w.shape[1], w.shape[0]) if transposed else (w.shape[0], w.shape[1])
        L = _native.lib()
        n = L.tai_conv_bf16_weight_elems(K, C, k)
        _native.check(n if n < 0 else 0, 'tai_conv_bf16_weight_elems')
        Wp = torch.empty(n, dtype=torch.bfloat16, device=w.device)
        _native.launch('tai_conv_bf16_pack_weights', w.device, w, Wp, K, C, k, int(transposed))
        return Wp
    return _cached(weight, ('bf16', transposed), make)


def _bf16_conv(parts, weight, bias, act, transposed=False, out=None, pool=False, addx=None, keep_plain=True):
    """One tai_conv_bf16_forward over 1-4 channel parts.  Returns y; with ``pool`` (y, pooled); with ``addx``
    (y or None, y + fixed_unpool(addx)) as conv_bias_unpool_add."""
    x0 = parts[0]
    N, Cp, H, W = x0.shape
    k = weight.shape[2]
    Co, Ci = (weight.shape[1], weight.shape[0]) if transposed else (weight.shape[0], weight.shape[1])
    parts = [p.contiguous() for p in parts]
    y = out if _usable_out(out, (N, Co, H, W), x0) else torch.empty((N, Co, H, W), dtype=torch.float32, device=x0.device)
    yp = torch.empty((N, Co, H // 2, W // 2), dtype=torch.float32, device=x0.device) if pool else None
    y2 = None
    if addx is not None:
        addx = addx.contiguous()
        y2 = torch.empty_like(y) if keep_plain else None
    ptrs = (ctypes.c_void_p * len(parts))(*[p.data_ptr() for p in parts])
    _native.launch('tai_conv_bf16_forward', x0.device, ptrs, len(parts), _bf16_weights(weight, transposed), bias, y, yp, addx, y2,
                   N, Ci, Co, H, W, k, _ACT[act])
    if pool:
        return y, yp
    if addx is not None:
        return (y, y2) if keep_plain else (None, y)
    return y


_WINO_TILE = [4]
WINO43_MIN_CHANNELS = 64         # F(4x4, 3x3) where both C and K are at least this: every 3x3 layer of MC-Net but the first and the last.  (128 until
                                 # the kernel moved from Lavin's interpolation points to (0, +-3/4, +-3/2, inf), whose per-layer rounding is ~4x lower:
                                 # with it the end-to-end error against the CPU oracle is the F(2x2) one on every config at 64 as well --
                                 # profiles/r05_wino_f43_points_study.txt, r05_wino43_min_channels.txt; 49.7 -> 46.75 ms on the configs[1] forward)
WINO43_MIN_WORKGROUPS = 150      # ... and where its 64-channel x 32-tile workgroups occupy most of the chip (round 5's kernel, same box, the
                                 # replayed configs[1] forward: 400: 51.11 ms, 256: 50.78, 150: 50.57, 100: 51.32, 64: 51.75 -- tools/w43_threshold_ab.py)
WINO43_SPLIT_MIN_WORKGROUPS = 150   # MC-Net's own layers take the split over input channels (_wino43_launch) only from this many unsplit
                                 # workgroups: the layers the default dispatch puts on F(4x4, 3x3) by themselves.  A layer that is on it only
                                 # because a caller lowered WINO43_MIN_WORKGROUPS keeps the unsplit kernel and its bits.


def set_weight_gradient_tile(m):
    """Transform domain of the 3x3 weight-gradient kernel (wino_weight_grad): 4 (default): F(4x4, 3x3) -- csrc/wino43_conv.hip.inc,
    conv3x3_wrw_gen: the forward kernel's chunk loop with the tiles as the reduction, 1.78x fewer MFMAs, 1.15-1.5x faster per layer -- where
    H % 4 == 0 and the input is a plain tensor; 2: F(2x2, 3x3) everywhere (csrc/wino_wrw.hip.inc, rounds 2-5).  Both sum in a fixed order.
    Returns the previous value."""
    prev = _native.lib().tai_conv3x3_wino_wrw_set_tile(m)
    if prev < 0:
        raise ValueError(m)
    return prev


def set_winograd_tile(m):
    """Output tile of the Winograd 3x3 convolutions: 4 (default since the end of round 4): F(4x4, 3x3), csrc/wino43_conv.hip.inc, on the
    layers with C >= 64 and K >= 64 (WINO43_MIN_CHANNELS; the layers marked by mark_outside_recurrence at any width) and enough workgroups
    -- 1.78x fewer MFMAs, fp32 operands on the fp32 MFMA as everywhere else; on its interpolation points (0, +-3/4, +-3/2, inf) the
    rounding error is ~3-4x F(2x2, 3x3)'s per layer and the forward's end-to-end error against the CPU oracle is that of F(2x2, 3x3) on
    every config (profiles/r05_wino_f43_points_study.txt, r05_wino43_min_channels.txt) -- and F(2x2, 3x3), csrc/wino_conv.hip.inc, on
    every other layer; or 2: F(2x2, 3x3) on every layer (the arithmetic of rounds 1-3).  A hipGraph captured before a switch
    keeps replaying what it captured.  Returns the previous value."""
    if m not in (2, 4):
        raise ValueError(m)
    prev, _WINO_TILE[0] = _WINO_TILE[0], m
    return prev


def get_winograd_tile():
    return _WINO_TILE[0]


def mark_outside_recurrence(module):
    """Tell the dispatch that ``module``'s 3x3 layers may take F(4x4, 3x3) below WINO43_MIN_CHANNELS too (from 16 input channels).  The
    kernel network and the merge residuals feed the separable convolution once per output frame, outside MC-Net's recurrence (where
    every prediction is the next step's input): with all of them on the 4 x 4 tile the forward's end-to-end error against float64 is
    unchanged (profiles/r05_wino_f43_policy_study.txt, measured with Lavin's points, whose rounding was ~4x the present ones').
    TAIFillInModel marks kernelnet and merge_residual{1,2,3} (tai.py)."""
    for p in module.parameters():
        p._tai_f43_any_width = True


def _wino43_ok(N, Ci, Co, H, W, nparts=1, weight=None, split=True):
    """F(4x4, 3x3) for this layer?  ``split``: the caller launches through _wino43_launch (the split over input channels on small grids);
    the autograd paths pass False: their launches never split, so a layer's training arithmetic does not depend on the batch size."""
    any_width = getattr(weight, '_tai_f43_any_width', False)
    wide = (Ci >= WINO43_MIN_CHANNELS and Co >= WINO43_MIN_CHANNELS) or (Ci >= 16 and any_width)
    if not (_WINO_TILE[0] == 4 and wide and H % 4 == 0 and W % 4 == 0
            and Ci % nparts == 0 and ((Ci // nparts) % 4 == 0 or nparts == 1) and N * max(Ci, Co) * H * W < 2 ** 29):
        return False
    groups = ((N * (H // 4) * (W // 4) + 31) // 32) * ((Co + 63) // 64)
    if groups >= WINO43_MIN_WORKGROUPS:
        return True
    # below the threshold: a layer outside MC-Net's recurrence counts its workgroups after the split over input channels
    # (tai_conv3x3_wino43_splits); MC-Net's own layers there keep F(2x2, 3x3), whose rounding the T = 10 parity margin was measured on
    return split and bool(any_width) and groups * _native.lib().tai_conv3x3_wino43_splits(N, Ci, Co, H, W, nparts, None) >= WINO43_MIN_WORKGROUPS


def _wino43_launch(ptrs, nparts, U, bias, y, N, C, K, H, W, act, weight, ypool=None, addx=None, y2=None):
    """One F(4x4, 3x3) forward (tai_conv3x3_wino43_forward_ws).  Where the library splits the input channels over more workgroups
    (small grids) it needs a workspace for the partial tiles: allocated here with torch, so that under graph capture it comes
    from the graph's pool.  ``ptrs``: a ctypes array of the nparts input pointers."""
    groups = ((N * (H // 4) * (W // 4) + 31) // 32) * ((K + 63) // 64)
    if groups < WINO43_SPLIT_MIN_WORKGROUPS and not getattr(weight, '_tai_f43_any_width', False):
        _native.launch('tai_conv3x3_wino43_forward_ex', y.device, ptrs, nparts, U, bias, y, ypool, addx, y2, N, C, K, H, W, act)
        return
    n = _native.lib().tai_conv3x3_wino43_workspace_floats(N, C, K, H, W, nparts)
    _native.check(n if n < 0 else 0, 'tai_conv3x3_wino43_workspace_floats')
    ws = torch.empty(n, dtype=torch.float32, device=y.device) if n > 0 else None
    _native.launch('tai_conv3x3_wino43_forward_ws', y.device, ptrs, nparts, U, bias, y, ypool, addx, y2, ws, n, N, C, K, H, W, act)


def _cached(weight, tag, make):
    """Derived form of a weight, kept on the tensor object and rebuilt when the weight's version counter or storage
    moves, or after ``invalidate_derived``."""
    cache = getattr(weight, '_tai_derived', None)
    if cache is None:
        cache = {}
        weight._tai_derived = cache
    hit = cache.get(tag)
    key = (weight._version, weight.data_ptr(), _EPOCH[0])
    if hit is None or hit[0] != key:
        hit = (key, make())
        cache[tag] = hit
    return hit[1]


def _registered(U):
    """A transformed-weight buffer of the F(2x2, 3x3) entry points: the library keeps the addresses of the split-bf16 images it wrote (the
    forward entry points follow the buffer they are handed); the entry goes when the tensor does (the registry used to grow
    without bound and a recycled address could be read in the wrong layout)."""
    import weakref
    weakref.finalize(U, _native.lib().tai_conv3x3_wino_forget_weights, U.data_ptr())
    return U


def _transform(w, tile):
    """The Winograd-domain image of a contiguous [K, C, 3, 3] filter: ``tile`` 2 / 4 -- the F(2x2, 3x3) / F(4x4, 3x3) layout."""
    K, C = w.shape[0], w.shape[1]
    pre = 'tai_conv3x3_wino43' if tile == 4 else 'tai_conv3x3_wino'
    U = torch.empty(getattr(_native.lib(), pre + '_weight_floats')(K, C), dtype=torch.float32, device=w.device)
    if tile == 2:
        _registered(U)
    _native.launch(pre + '_transform_weights', w.device, w, U, K, C)
    return U


def _transformed_weights(weight, transposed, tile, blocks=False):
    """The cached transformed weights of a layer.  ``transposed``: of the weight transposed and flipped (a stride-1 ConvTranspose2d;
    the input-gradient convolution of the same weight, weight[k, c, a, b] -> [c, k, K-1-a, K-1-b]).  ``blocks``: the k x k filter
    (k = 5, 7) first rewritten as S x S blocks of 3 x 3 taps (_block3x3_weight: the shifted-copy stack of _kxk_as_wino, the displaced
    reads of tai_conv3x3_wino43_forward_blocks).  The F(2x2, 3x3) buffers depend on the arithmetic, which is part of their tag."""
    def make():
        w = _as_conv_weight(weight.detach(), transposed)
        return _transform(_block3x3_weight(w.contiguous() if transposed else w) if blocks else w.contiguous(), tile)
    name = ('wino43' if tile == 4 else 'wino') + ('_kxk' if blocks else '')
    return _cached(weight, (name, transposed) if tile == 4 else (name, transposed, _WINO_ARITH[0]), make)


def _wino_weights_kxk(weight, transposed=False):
    return _transformed_weights(weight, transposed, 2, blocks=True)


def _block3x3_weight(weight):
    """[K, C, k, k] (k = 5, 7) -> [K, S*S*C, 3, 3]: block (a, b) of 3x3 taps of the k x k filter, zero past k, for the
    stack of shifted inputs tai_conv_shift_stack builds (channel order (a*S + b)*C + c)."""
    K, C, k, _ = weight.shape
    S = (k + 2) // 3
    wp = F.pad(weight, (0, 3 * S - k, 0, 3 * S - k))                        # [K, C, 3S, 3S]
    wp = wp.view(K, C, S, 3, S, 3).permute(0, 2, 4, 1, 3, 5)                # [K, a, b, C, 3, 3]
    return wp.reshape(K, S * S * C, 3, 3).contiguous()


def _wino43_blocks_ok(N, Cin, Co, H, W):
    """MotionEnc's 5x5 / 7x7 layers on the 4 x 4 tile (displaced reads): the 7x7 (128 -> 256) is a wide layer, the 5x5 (64 -> 128) was
    measured parity-neutral too (profiles/r05_wino_f43_policy_study.txt: "big + MotionEnc 5x5")."""
    return (_WINO_TILE[0] == 4 and Cin % 4 == 0 and Cin >= 16 and H % 4 == 0 and W % 4 == 0
            and ((N * (H // 4) * (W // 4) + 31) // 32) * ((Co + 63) // 64) >= WINO43_MIN_WORKGROUPS)


def _kxk_as_blocks(x, weight, bias, act, transposed=False):
    """5x5 / 7x7 "same" convolution on the 4 x 4 tile: x copied into a zero-haloed plane, read S x S times by displaced 3 x 3 blocks
    (tai_conv3x3_wino43_forward_blocks).  The training form's forward and input gradient (``transposed``)."""
    N, C, H, W = x.shape
    K, k = weight.shape[1 if transposed else 0], weight.shape[2]
    S, top, left, in_h, in_w = halo_geometry(H, W, k)
    plane = halo_plane(N, C, H, W, k, x.device)
    plane[:, :, top:top + H, left:left + W].copy_(x)
    y = torch.empty((N, K, H, W), dtype=x.dtype, device=x.device)
    _native.launch('tai_conv3x3_wino43_forward_blocks', x.device, plane, k, _transformed_weights(weight, transposed, 4, blocks=True), bias,
                   y, None, 0, 0, 0, 0, N, S * S * C, K, H, W, in_h, in_w, 1, 2, _ACT[act])
    return y


def _kxk_as_wino(x, weight, bias, act, pool, transposed=False, keep_stack=False):
    """5x5 / 7x7 "same" convolution as the Winograd 3x3 kernel over S*S shifted copies of the input (csrc/thin_conv.hip.inc,
    shift_stack): 1.56x / 1.36x fewer multiplies than the direct form MIOpen runs.  Returns y or (y, pooled).
    ``transposed``: convolve with the transposed and flipped filter (the input gradient of the same layer)."""
    N, C, H, W = x.shape
    K, k = weight.shape[1 if transposed else 0], weight.shape[2]
    S = (k + 2) // 3
    x = x.contiguous()
    stack = torch.empty((N, S * S * C, H + 2, W + 4), dtype=x.dtype, device=x.device)     # shifted copies, own halo
    U = _wino_weights_kxk(weight, transposed)
    y = torch.empty((N, K, H, W), dtype=x.dtype, device=x.device)
    yp = torch.empty((N, K, H // 2, W // 2), dtype=x.dtype, device=x.device) if pool else None
    _native.launch('tai_conv_shift_stack', x.device, x, stack, N, C, H, W, k)
    _native.launch('tai_conv3x3_wino_forward_window', x.device, stack, U, bias, y, yp, N, S * S * C, K, H, W, H + 2, W + 4, 1, 2, _ACT[act])
    if keep_stack:
        return y, stack
    return (y, yp) if pool else y


def _unblock3x3_weight(wb, C, k):
    """Inverse of _block3x3_weight for a gradient: [K, S*S*C, 3, 3] -> [K, C, k, k] (the taps past k are padding)."""
    K = wb.shape[0]
    S = (k + 2) // 3
    return wb.view(K, S, S, C, 3, 3).permute(0, 3, 1, 4, 2, 5).reshape(K, C, 3 * S, 3 * S)[:, :, :k, :k].contiguous()


_HALO_PLANES = {}


def halo_geometry(H, W, k):
    """The plane through which a k x k (k = 5, 7) "same" convolution over an H x W image reads its S x S blocks of 3 x 3
    taps as displaced 3 x 3 convolutions (tai_conv3x3_wino_forward_ex, shift_s): -> (S, top, left, in_h, in_w).  Image
    pixel (0, 0) sits at (top, left) = (k/2, k/2 + 1): block (0, 0)'s centre tap of output (0, 0) is then at (1, 2) -- the
    kernel's (in_oy, in_ox), in_ox even -- and block (a, b) reads 3a rows / 3b columns further, up to row H + 1 + 3 (S - 1)
    and column W + 3 + 3 (S - 1), all inside the plane; everything outside the image is zero."""
    S = (k + 2) // 3
    in_h, in_w = H + 2 + 3 * (S - 1), W + 4 + 3 * (S - 1)
    return S, k // 2, k // 2 + 1, in_h, in_w + (in_w & 1)


def halo_plane(N, C, H, W, k, device):
    """A cached zero-filled [N, C, in_h, in_w] buffer for halo_geometry(H, W, k): producers write the image into its
    interior (pooled-output window of the convolution before), the halo stays zero from the allocation on.  One buffer
    per (shape, device, stream): the consumer runs right behind the producer on that stream."""
    S, top, left, in_h, in_w = halo_geometry(H, W, k)
    key = (N, C, in_h, in_w, str(device), torch.cuda.current_stream(device).cuda_stream)
    buf = _HALO_PLANES.get(key)
    if buf is None:
        buf = torch.zeros((N, C, in_h, in_w), dtype=torch.float32, device=device)
        _HALO_PLANES[key] = buf
    return buf


def _no_grad_needed(*tensors):
    return not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors))


def motion_enc_chain(diff, conv1, conv2, conv3):
    """MotionEnc's three convolution + ReLU + 2x2 max pool stages (mcnet.py:28-60: 5x5 1 -> g, 5x5 g -> 2g, 7x7 2g -> 4g)
    with each pooled output written straight into the halo-carrying plane the next stage reads through displaced 3 x 3
    blocks: no pooled tensor is copied, padded or stacked in between.  Returns (pooled3, [c1, c2, c3]) or None when
    the shapes do not qualify (the caller then runs the stages one by one)."""
    if not (torch.is_tensor(diff) and diff.is_cuda and diff.dtype == torch.float32 and diff.dim() == 4 and diff.shape[1] == 1):
        return None
    if _CONV_PREC[0] == 'bf16':         # the stages one by one: the thin first layer in fp32, the 5x5 and 7x7 on the bf16 kernel
        return None
    ws = [conv1.weight, conv2.weight, conv3.weight]
    bs = [conv1.bias, conv2.bias, conv3.bias]
    if any(b is None for b in bs) or not _no_grad_needed(diff, *ws, *bs):
        return None
    N, _, H, W = diff.shape
    g = ws[0].shape[0]
    if not (tuple(ws[0].shape) == (g, 1, 5, 5) and tuple(ws[1].shape) == (2 * g, g, 5, 5) and tuple(ws[2].shape) == (4 * g, 2 * g, 7, 7)
            and conv1.padding[0] == 2 and conv2.padding[0] == 2 and conv3.padding[0] == 3
            and H % 8 == 0 and W % 8 == 0 and g % 8 == 0 and g >= 16):
        return None
    H2, W2, H4, W4 = H // 2, W // 2, H // 4, W // 4
    S2, top2, left2, ih2, iw2 = halo_geometry(H2, W2, 5)
    S3, top3, left3, ih3, iw3 = halo_geometry(H4, W4, 7)
    if not (_wino_ok(N, S2 * S2 * g, 2 * g, H2, W2, 3, 3, 1) and _wino_ok(N, S3 * S3 * 2 * g, 4 * g, H4, W4, 3, 3, 1)
            and N * g * ih2 * iw2 < 2 ** 29 and N * 2 * g * ih3 * iw3 < 2 ** 29 and N * g * H * W < 2 ** 29):
        return None
    dev = diff.device
    diff = diff.contiguous()
    c1 = torch.empty((N, g, H, W), dtype=torch.float32, device=dev)
    c2 = torch.empty((N, 2 * g, H2, W2), dtype=torch.float32, device=dev)
    c3 = torch.empty((N, 4 * g, H4, W4), dtype=torch.float32, device=dev)
    p3 = torch.empty((N, 4 * g, H4 // 2, W4 // 2), dtype=torch.float32, device=dev)
    plane2 = halo_plane(N, g, H2, W2, 5, dev)
    plane3 = halo_plane(N, 2 * g, H4, W4, 7, dev)
    U2 = None if _wino43_blocks_ok(N, g, 2 * g, H2, W2) else _wino_weights_kxk(ws[1])
    U3 = None if _wino43_blocks_ok(N, 2 * g, 4 * g, H4, W4) else _wino_weights_kxk(ws[2])
    xs2 = (ctypes.c_void_p * 1)(plane2.data_ptr())
    xs3 = (ctypes.c_void_p * 1)(plane3.data_ptr())
    _native.launch('tai_conv_cin1_forward_maxpool_window', dev, diff, ws[0].contiguous(), bs[0], c1, plane2, N, g, H, W, 5, 1,
                   ih2, iw2, top2, left2)
    if _wino43_blocks_ok(N, g, 2 * g, H2, W2):               # the 4 x 4 tile (set_winograd_tile): 1.78x fewer MFMAs
        _native.launch('tai_conv3x3_wino43_forward_blocks', dev, plane2, 5, _transformed_weights(ws[1], False, 4, blocks=True), bs[1],
                       c2, plane3, ih3, iw3, top3, left3, N, S2 * S2 * g, 2 * g, H2, W2, ih2, iw2, 1, 2, 1)
    else:
        _native.launch('tai_conv3x3_wino_forward_ex', dev, xs2, 1, 5, U2, bs[1], c2, plane3, ih3, iw3, top3, left3, None, None,
                       N, S2 * S2 * g, 2 * g, H2, W2, ih2, iw2, 1, 2, 1)
    if _wino43_blocks_ok(N, 2 * g, 4 * g, H4, W4):
        _native.launch('tai_conv3x3_wino43_forward_blocks', dev, plane3, 7, _transformed_weights(ws[2], False, 4, blocks=True), bs[2],
                       c3, p3, 0, 0, 0, 0, N, S3 * S3 * 2 * g, 4 * g, H4, W4, ih3, iw3, 1, 2, 1)
    else:
        _native.launch('tai_conv3x3_wino_forward_ex', dev, xs3, 1, 7, U3, bs[2], c3, p3, 0, 0, 0, 0, None, None,
                       N, S3 * S3 * 2 * g, 4 * g, H4, W4, ih3, iw3, 1, 2, 1)
    return p3, [c1, c2, c3]


def _kxk_ok(N, Ci, Co, H, W, kh, kw, padding):
    S = (kh + 2) // 3
    return (kh == kw and kh in (5, 7) and padding == kh // 2 and W % 4 == 0 and Ci >= 16
            and N * S * S * Ci * (H + 2) * (W + 4) < 2 ** 29 and _wino_ok(N, S * S * Ci, Co, H, W, 3, 3, 1))


# Below this the kernel leaves most of the 256 CUs idle and MIOpen is as fast (tools/conv_path_times.py).  72 rather than round
# 1's 96: configs[1]'s last MIOpen layers (the kernel network's 512 -> 512 at 4 x 4 over 160 samples: 80 workgroups) run 132 us here
# against 121-155 us there, and MIOpen's implicit-GEMM kernel sums with atomics -- with it the forward's kernel-network outputs
# differed by 1.5e-6 from replay to replay; without it 1,500 replays of the whole forward are bit-identical (tools/soak_forward.py).
WINO_MIN_WORKGROUPS = 72

# Planes with an odd side on the F(2x2, 3x3) kernel, the weight-gradient kernel on any row length, the discriminator's space-to-depth
# route on even (not only multiple-of-4) inputs and the 3-channel layers under autograd (min_ci 2 in _conv_bias_act's training branch):
# False restores the routes of before (MIOpen for those shapes) -- A/B timing (tools/published_shapes_bench.py)
RAGGED_ROUTES = [True]


def set_ragged_routes(on):
    """Switch the odd-plane / any-row-length routes on or off; returns the previous setting."""
    prev = RAGGED_ROUTES[0]
    RAGGED_ROUTES[0] = bool(on)
    return prev


# Training: convolutions of a tuple of channel parts go through _WinoConv3x3Parts (no torch.cat in the forward, one contiguous input
# gradient per part); False restores the concatenating path (A/B, tests)
PARTS_UNDER_AUTOGRAD = True


def _wino_ok(N, Ci, Co, H, W, kh, kw, padding, min_ci=8, ragged=False):
    """``min_ci``: the kernel pads the input channels to a multiple of 8 with zero weights, so fewer than 8 work -- at the cost of a
    whole chunk; the inference paths take that down to 2 (TAI_color's first ContentEnc layer, 3 -> 64 at 256 x 256: 276 us against
    MIOpen's 620), and so does the single-tensor training path (_WinoConv3x3: the 3-channel layers of c_dim 3, whose input or output
    gradient then runs one 64-row block of MFMA for 3 channels -- in exchange for an update without MIOpen's atomics).
    ``ragged=True`` (the callers of the plain convolution of plain or part-wise inputs): an odd H or W is taken as well (ceil(H / 2) x
    ceil(W / 2) tiles, row H and column W are padding); the default keeps even planes, which the other variants need -- pooled or
    unpooled epilogues, input windows, displaced reads -- and the split-bf16 arithmetic has even planes only."""
    even = H % 2 == 0 and W % 2 == 0
    if not even and not (ragged and RAGGED_ROUTES[0] and _WINO_ARITH[0] == 0):
        return False
    return (kh == kw == 3 and padding == 1 and Ci >= min_ci and N * max(Ci, Co) * H * W < 2 ** 29
            and ((N * ((H + 1) // 2) * ((W + 1) // 2) + 63) // 64) * ((Co + 63) // 64) >= WINO_MIN_WORKGROUPS)


def _usable_out(out, shape, like):
    return (out is not None and tuple(out.shape) == tuple(shape) and out.is_contiguous() and out.dtype == like.dtype
            and out.device == like.device)


def _wino_forward(x, U, bias, y, N, Ci, Co, H, W, act):
    """tai_conv3x3_wino_forward; a plane with an odd side through the general entry (tai_conv3x3_wino_forward_ex), which takes it"""
    if H % 2 == 0 and W % 2 == 0:
        _native.launch('tai_conv3x3_wino_forward', x.device, x, U, bias, y, N, Ci, Co, H, W, _ACT[act])
    else:
        xs = (ctypes.c_void_p * 1)(x.data_ptr())
        _native.launch('tai_conv3x3_wino_forward_ex', x.device, xs, 1, 0, U, bias, y, None, 0, 0, 0, 0, None, None,
                       N, Ci, Co, H, W, H, W, 0, 0, _ACT[act])


def _wino_launch(x, U, bias, N, Ci, Co, H, W, act):
    y = torch.empty((N, Co, H, W), dtype=x.dtype, device=x.device)
    _wino_forward(x, U, bias, y, N, Ci, Co, H, W, act)
    return y


# Under autograd the forward and the input gradient (the same convolution with the weight transposed and flipped) take the 4 x 4 tile on
# the layers the inference path gives it: the training forward then runs the arithmetic of the inference forward (False: F(2x2, 3x3)
# for everything under autograd, as in rounds 2-4)
WINO43_UNDER_AUTOGRAD = True


def _conv3x3_autograd_launch(x, weight, eff_transposed, bias, N, Ci, Co, H, W, act):
    """conv(x, w_eff) with w_eff = the weight in orientation ``eff_transposed``: F(4x4, 3x3) where _wino43_ok says so, else F(2x2, 3x3)."""
    if WINO43_UNDER_AUTOGRAD and _wino43_ok(N, Ci, Co, H, W, 1, weight, split=False):
        y = torch.empty((N, Co, H, W), dtype=x.dtype, device=x.device)
        _native.launch('tai_conv3x3_wino43_forward', x.device, x, _transformed_weights(weight, eff_transposed, 4), bias, y,
                       N, Ci, Co, H, W, _ACT[act])
        return y
    return _wino_launch(x, _transformed_weights(weight, eff_transposed, 2), bias, N, Ci, Co, H, W, act)


def wino_conv3x3_plain(x, weight, transposed=False):
    """conv2d(x, w_eff, padding=1) without bias, activation or autograd on the in-tree Winograd kernels (F(4x4, 3x3) / F(2x2, 3x3) as
    _conv3x3_autograd_launch chooses); ``transposed``: w_eff = the weight transposed and flipped (the input-gradient convolution of the
    same weight).  None where neither kernel takes the shape -- the caller then keeps its own route.  (The discriminator's 4x4 stride-2
    layers as 3x3 layers on space-to-depth planes: sn_discriminator.py.)"""
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and weight.dtype == torch.float32 and x.dim() == 4):
        return None
    N, Ci, H, W = x.shape
    Co = weight.shape[1] if transposed else weight.shape[0]
    if (weight.shape[0] if transposed else weight.shape[1]) != Ci or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError('wino_conv3x3_plain: weight %s does not fit input %s' % (tuple(weight.shape), tuple(x.shape)))
    if not ((WINO43_UNDER_AUTOGRAD and _wino43_ok(N, Ci, Co, H, W, 1, weight, split=False)) or _wino_ok(N, Ci, Co, H, W, 3, 3, 1, ragged=True)):
        return None
    return _conv3x3_autograd_launch(x, weight, transposed, _zero_bias(Co, x.device), N, Ci, Co, H, W, None)


_ZERO_BIAS = {}


def _zero_bias(n, device):
    """A cached all-zero fp32 bias (read-only) for the input-gradient convolutions: one fill kernel per call otherwise."""
    key = (n, device)
    z = _ZERO_BIAS.get(key)
    if z is None:
        z = torch.zeros(n, dtype=torch.float32, device=device)
        if not torch.cuda.is_current_stream_capturing():       # (a fill recorded into a graph has not run yet: do not keep it)
            _ZERO_BIAS[key] = z
    return z


class _GrowingWorkspace(object):
    """Per-device fp32 scratch that grows to the largest request.  A captured graph (environments.train_step with
    graph_step) bakes the buffer's raw pointer into its kernel nodes, so once any request has been served under capture a
    superseded buffer is retired to a keep-alive list instead of being released: a later, larger eager request must not
    hand the old block back to the caching allocator while replays still write partial sums into it."""

    def __init__(self):
        self.current, self.retired, self.captured = {}, [], False

    def get(self, device, floats):
        self.captured = self.captured or torch.cuda.is_current_stream_capturing()
        ws = self.current.get(device)
        if ws is None or ws.numel() < floats:
            if ws is not None and self.captured:
                self.retired.append(ws)
            ws = self.current[device] = torch.empty(floats, dtype=torch.float32, device=device)
        return ws


_WRW_WORKSPACE = _GrowingWorkspace()


def wino_weight_grad(x, grad_out, with_bias=False, window=None, ragged=False):
    """dL/dw [Co, Ci, 3, 3] of y = conv2d(x, w, padding=1) from x [N, Ci, H, W] and dL/dy [N, Co, H, W], by
    ``tai_conv3x3_wino_wrw`` (Winograd-domain weight gradient on the fp32 MFMA pipe); None if the shape is not supported (odd H,
    W above 16 and not a multiple of 16, a tensor of 2 GiB or more; rows of fewer than 16 pixels are widened with zeros).
    ``ragged=True`` (the autograd paths): every shape but tensors of 2 GiB or more -- the shapes off the kernel's native grid are
    extended inside the kernel to an even number of rows and a multiple of 16 columns, the way the widening here does it.  ``with_bias``: returns (dw, dbias), the bias gradient
    summed by the same kernel.  ``window`` = (in_oy, in_ox): x is a plane [N, Ci, in_h, in_w] that carries its own halo,
    with the pixel under output (0, 0) at (in_oy, in_ox) (the shifted-copy stack of the 5x5 / 7x7 layers).  The workspace
    (partial sums per workgroup) is kept per device and grows to the largest request."""
    N, Ci = x.shape[0], x.shape[1]
    Co, H, W = grad_out.shape[1], grad_out.shape[2], grad_out.shape[3]
    L = _native.lib()
    if window is None and W % 16 and W < 16 and H % 2 == 0 and x.dtype == torch.float32 and grad_out.dtype == torch.float32:
        # rows shorter than the kernel's 16 pixels (the 8 x 8 and 4 x 4 layers of the kernel network and of the discriminator): both planes
        # widened to 16 columns with zeros -- the added output-gradient columns contribute nothing, the added input columns are the zero
        # padding the last real column sees anyway -- instead of ATen's weight gradient, whose summation order changes from run to run
        x, grad_out, W = F.pad(x, (0, 16 - W)), F.pad(grad_out, (0, 16 - W)), 16
    if not (ragged and RAGGED_ROUTES[0]) and (H % 2 or W % 16):
        return None
    floats = L.tai_conv3x3_wino_wrw_workspace_floats(N, Ci, Co, H, W)
    if floats < 0 or N * Ci * x.shape[2] * x.shape[3] >= 2 ** 29:
        return None
    ws = _WRW_WORKSPACE.get(x.device, floats)
    dw = torch.empty((Co, Ci, 3, 3), dtype=torch.float32, device=x.device)
    db = torch.empty(Co, dtype=torch.float32, device=x.device) if with_bias else None
    if window is None:
        _native.launch('tai_conv3x3_wino_wrw', x.device, x, grad_out, dw, db, ws, N, Ci, Co, H, W)
    else:
        _native.launch('tai_conv3x3_wino_wrw_window', x.device, x, grad_out, dw, db, ws, N, Ci, Co, H, W,
                       x.shape[2], x.shape[3], window[0], window[1])
    return (dw, db) if with_bias else dw


class _WinoConv3x3(torch.autograd.Function):
    """Training form of the 3x3 convolution: the forward and the input gradient (the same convolution with the weight
    transposed and flipped) run on the Winograd-MFMA kernel, the weight gradient on its Winograd-domain counterpart
    (wino_weight_grad; MIOpen's aten.convolution_backward for shapes that one does not take).  ``transposed``: the weight is a ConvTranspose2d(k 3, stride 1, padding 1) weight."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, transposed):
        x = x.contiguous()
        Co, Ci = (weight.shape[1], weight.shape[0]) if transposed else (weight.shape[0], weight.shape[1])
        N, _, H, W = x.shape
        y = _conv3x3_autograd_launch(x, weight, transposed, bias, N, Ci, Co, H, W, act)
        ctx.act, ctx.transposed = act, transposed
        ctx.save_for_backward(x, weight, y if act is not None else None)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, y = ctx.saved_tensors
        g = grad_out.contiguous()
        if ctx.act == 'relu':
            g = torch.ops.aten.threshold_backward(g, y, 0)        # g where y > 0, else 0: one kernel
        elif ctx.act == 'tanh':
            g = torch.ops.aten.tanh_backward(g, y)                  # g * (1 - y^2): one kernel
        N, Ci, H, W = x.shape
        Co = g.shape[1]
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            # d/dx of conv(x, w_eff) is conv(g, w_eff transposed and flipped): the other orientation of the same weight
            zero = _zero_bias(Ci, g.device)
            gx = _conv3x3_autograd_launch(g, weight, not ctx.transposed, zero, N, Co, Ci, H, W, None)
        if ctx.needs_input_grad[1]:
            gw_eff = None
            if g.dtype == torch.float32 and x.dtype == torch.float32:
                if ctx.needs_input_grad[2]:
                    both = wino_weight_grad(x, g, with_bias=True, ragged=True)
                    if both is not None:
                        gw_eff, gb = both
                else:
                    gw_eff = wino_weight_grad(x, g, ragged=True)
            if gw_eff is None:                                    # shapes the Winograd weight-gradient kernel does not take
                w_eff = _as_conv_weight(weight, ctx.transposed)
                gw_eff = torch.ops.aten.convolution_backward(g, x, w_eff, [Co], [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                                             [False, True, False])[1]
            gw = _as_conv_weight(gw_eff, ctx.transposed)          # the transpose-and-flip is its own inverse
        if ctx.needs_input_grad[2] and gb is None:
            gb = g.sum((0, 2, 3))
        return gx, gw, gb, None, None


class _WinoConv3x3Parts(torch.autograd.Function):
    """``_WinoConv3x3`` on an input given as up to four equal channel parts (the operands of a ``torch.cat`` along the channels that is
    never materialised: Residual, CombLayers, the ConvLSTM's (input, h), the kernel network's 1024-channel input).  Under autograd the
    parts used to be concatenated first (one copy of the layer's whole input per call) and the input gradient came back as ONE tensor,
    whose channel slices every producer then had to copy into contiguous memory for its own backward.  Here the forward reads the parts
    where they lie (``tai_conv3x3_wino_forward_parts``: the same bits as the convolution of the concatenation), the input gradient of
    part i is its own launch of the Winograd kernel over the K-slice of the transposed, flipped weight that belongs to it (the layer's
    work split by output channels: no flop more, a contiguous result per part) and the weight gradient is taken per part and joined
    along the input channels (a [Co, Ci, 3, 3] copy)."""

    @staticmethod
    def forward(ctx, weight, bias, act, transposed, *parts):
        x0 = parts[0]
        Co, Ci = (weight.shape[1], weight.shape[0]) if transposed else (weight.shape[0], weight.shape[1])
        N, Cp, H, W = x0.shape
        y = torch.empty((N, Co, H, W), dtype=x0.dtype, device=x0.device)
        ptrs = (ctypes.c_void_p * len(parts))(*[p.data_ptr() for p in parts])
        if WINO43_UNDER_AUTOGRAD and _wino43_ok(N, Ci, Co, H, W, len(parts), weight, split=False):
            _native.launch('tai_conv3x3_wino43_forward_parts', x0.device, ptrs, len(parts), _transformed_weights(weight, transposed, 4), bias, y,
                           N, Ci, Co, H, W, _ACT[act])
        else:
            _native.launch('tai_conv3x3_wino_forward_parts', x0.device, ptrs, len(parts), _transformed_weights(weight, transposed, 2), bias, y,
                           N, Ci, Co, H, W, _ACT[act])
        ctx.act, ctx.transposed, ctx.nparts = act, transposed, len(parts)
        ctx.save_for_backward(weight, y if act is not None else None, *parts)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        weight, y, parts = saved[0], saved[1], saved[2:]
        g = grad_out.contiguous()
        if ctx.act == 'relu':
            g = torch.ops.aten.threshold_backward(g, y, 0)
        elif ctx.act == 'tanh':
            g = torch.ops.aten.tanh_backward(g, y)
        N, Cp, H, W = parts[0].shape
        Co, n = g.shape[1], ctx.nparts
        gparts = [None] * n
        for i in range(n):
            if ctx.needs_input_grad[4 + i]:
                if WINO43_UNDER_AUTOGRAD and _wino43_ok(N, Co, Cp, H, W, 1, weight, split=False):
                    gparts[i] = torch.empty((N, Cp, H, W), dtype=g.dtype, device=g.device)
                    _native.launch('tai_conv3x3_wino43_forward', g.device, g, _wino_weights_input_grad_part(weight, ctx.transposed, i, n, tile=4),
                                   _zero_bias(Cp, g.device), gparts[i], N, Co, Cp, H, W, 0)
                else:
                    gparts[i] = _wino_launch(g, _wino_weights_input_grad_part(weight, ctx.transposed, i, n), _zero_bias(Cp, g.device),
                                             N, Co, Cp, H, W, None)
        gw = gb = None
        if ctx.needs_input_grad[0]:
            want_bias = ctx.needs_input_grad[1]
            pieces = []
            for i in range(n):
                r = wino_weight_grad(parts[i], g, with_bias=(want_bias and i == 0), ragged=True)
                if r is None:
                    pieces = None
                    break
                if want_bias and i == 0:
                    r, gb = r
                pieces.append(r)
            if pieces is None:                                        # shapes the Winograd weight-gradient kernel does not take
                w_eff = _as_conv_weight(weight, ctx.transposed)
                gw_eff = torch.ops.aten.convolution_backward(g, torch.cat(parts, dim=1), w_eff, [Co], [1, 1], [1, 1], [1, 1], False,
                                                             [0, 0], 1, [False, True, False])[1]
            else:
                gw_eff = torch.cat(pieces, dim=1)
            gw = _as_conv_weight(gw_eff, ctx.transposed)
        if ctx.needs_input_grad[1] and gb is None:
            gb = g.sum((0, 2, 3))
        return (gw, gb, None, None) + tuple(gparts)


def _wino_weights_input_grad_part(weight, transposed, i, nparts, tile=2):
    """Transformed weights of the input-gradient convolution of channel part ``i`` of ``nparts``: conv(g, w_i transposed and flipped)
    with w_i the slice of the layer's effective weight [Co, Ci, 3, 3] over that part's input channels; ``tile`` 2 / 4: the F(2x2, 3x3) /
    F(4x4, 3x3) layout."""
    def make():
        w_eff = _as_conv_weight(weight.detach(), transposed)                              # [Co, Ci, 3, 3]
        Cp = w_eff.shape[1] // nparts
        return _transform(w_eff[:, i * Cp:(i + 1) * Cp].transpose(0, 1).flip(2, 3).contiguous(), tile)   # [Cp, Co, 3, 3]
    return _cached(weight, ('wino_input_grad_part', transposed, i, nparts, tile, _WINO_ARITH[0]), make)


class _WinoConvKxK(torch.autograd.Function):
    """Training form of the 5x5 / 7x7 convolutions (MotionEnc, mcnet.py:36-47): forward and input gradient as 3x3 blocks on
    the Winograd-MFMA kernel (_kxk_as_wino), weight and bias gradients on the Winograd-domain weight-gradient kernel over the
    same stack of shifted copies (MIOpen's where that kernel does not take the shape)."""

    @staticmethod
    def forward(ctx, x, weight, bias, act):
        x = x.contiguous()
        N, Ci, H, W = x.shape
        Co = weight.shape[0]
        ctx.act = act
        if WINO43_UNDER_AUTOGRAD and act in (None, 'relu') and _wino43_blocks_ok(N, Ci, Co, H, W):
            # the 4 x 4 tile over a halo plane; the stack of shifted copies the weight gradient reads is built in the backward pass
            # (134 / 151 MB per MotionEnc call no longer kept from forward to backward)
            y = _kxk_as_blocks(x, weight, bias, act)
            ctx.save_for_backward(x, weight, y if act is not None else None)
            return y
        y, stack = _kxk_as_wino(x, weight, bias, act, False, keep_stack=True)
        # the stack of shifted copies (S*S times the input) is kept for the weight gradient: 134 / 151 MB per MotionEnc call
        ctx.save_for_backward(x, weight, y if act is not None else None, stack)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        x, weight, y = saved[0], saved[1], saved[2]
        g = grad_out.contiguous()
        if ctx.act == 'relu':
            g = torch.ops.aten.threshold_backward(g, y, 0)
        elif ctx.act == 'tanh':
            g = torch.ops.aten.tanh_backward(g, y)                  # g * (1 - y^2): one kernel
        Co, Ci, k = weight.shape[0], weight.shape[1], weight.shape[2]
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            if WINO43_UNDER_AUTOGRAD and _wino43_blocks_ok(g.shape[0], Co, Ci, g.shape[2], g.shape[3]):
                gx = _kxk_as_blocks(g, weight, _zero_bias(Ci, g.device), None, transposed=True)
            else:
                gx = _kxk_as_wino(g, weight, _zero_bias(Ci, g.device), None, False, transposed=True)
        if ctx.needs_input_grad[1]:
            if len(saved) > 3:
                stack = saved[3]
            else:
                N, _, H, W = x.shape
                S = (k + 2) // 3
                stack = torch.empty((N, S * S * Ci, H + 2, W + 4), dtype=x.dtype, device=x.device)
                _native.launch('tai_conv_shift_stack', x.device, x, stack, N, Ci, H, W, k)
            # the weight gradient of the blocked 3x3 form over the stack (it carries its halo: origin (1, 2)), then un-blocked
            both = wino_weight_grad(stack, g, with_bias=True, window=(1, 2), ragged=True)
            if both is not None:
                gw, gb = _unblock3x3_weight(both[0], Ci, k), both[1]
            else:
                gw = torch.ops.aten.convolution_backward(g, x, weight, [Co], [1, 1], [k // 2, k // 2], [1, 1], False, [0, 0], 1,
                                                         [False, True, False])[1]
        if ctx.needs_input_grad[2] and gb is None:
            gb = g.sum((0, 2, 3))
        return gx, gw, gb, None


_THIN_WORKSPACE = _GrowingWorkspace()


def thin_weight_grad(big, thin, k):
    """(dw [Cb, k, k], db [Cb]) with dw[cb][a][b] = sum of big[n, cb, y, x] * thin[n, 0, y + a - k/2, x + b - k/2] and
    db[cb] = sum of big[n, cb]: one pass over ``big`` (tai_thin_conv_wrw)."""
    N, Cb, H, W = big.shape
    ws = _THIN_WORKSPACE.get(big.device, N * Cb * 32)
    dw = torch.empty((Cb, k, k), dtype=torch.float32, device=big.device)
    db = torch.empty(Cb, dtype=torch.float32, device=big.device)
    _native.launch('tai_thin_conv_wrw', big.device, big, thin, dw, db, ws, N, Cb, H, W, k)
    return dw, db


class _ThinInConv(torch.autograd.Function):
    """Training form of the one-input-channel layers (nn.Conv2d(1, gf, k) + ReLU, mcnet.py:28-31, 79-81): forward on
    tai_conv_cin1_forward, weight and bias gradients in one pass over the output gradient (thin_weight_grad); the input is
    a frame (difference), which needs no gradient -- if it does, ATen's."""

    @staticmethod
    def forward(ctx, x, weight, bias, act):
        x = x.contiguous()
        N, _, H, W = x.shape
        Co, k = weight.shape[0], weight.shape[2]
        y = torch.empty((N, Co, H, W), dtype=x.dtype, device=x.device)
        _native.launch('tai_conv_cin1_forward', x.device, x, weight.detach().contiguous(), bias, y, N, Co, H, W, k, _ACT[act])
        ctx.act = act
        ctx.save_for_backward(x, weight, y if act is not None else None)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, y = ctx.saved_tensors
        g = grad_out.contiguous()
        if ctx.act == 'relu':
            g = torch.ops.aten.threshold_backward(g, y, 0)
        Co, k = weight.shape[0], weight.shape[2]
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            # (the frame difference of an autoregressive step is itself generated)
            N, _, H, W = x.shape
            wf = weight.detach().flip(2, 3).transpose(0, 1).contiguous()                 # [1, Co, k, k]: the filter flipped
            gx = torch.empty_like(x)
            if k == 5:
                _native.launch('tai_conv_cout1_5x5_forward', x.device, g, wf, None, gx, N, Co, H, W)
            else:
                _native.launch('tai_conv_cout1_3x3_forward', x.device, g, wf, _zero_bias(1, x.device), gx, N, Co, H, W, 0)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, gb = thin_weight_grad(g, x, k)
            gw = dw.view_as(weight)
        return gx, gw, gb, None


class _ThinOutConv(torch.autograd.Function):
    """Training form of the one-output-channel layer (nn.ConvTranspose2d(gf, 1, 3, padding=1) + Tanh, mcnet.py:223-224):
    forward on tai_conv_cout1_3x3_forward; the input gradient is a one-input-channel convolution of the output gradient
    with the flipped filter (tai_conv_cin1_forward), the weight gradient one pass over the input (thin_weight_grad)."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, transposed):
        x = x.contiguous()
        N, Ci, H, W = x.shape
        wd = _cached(weight, ('direct', transposed), lambda: _as_conv_weight(weight.detach(), transposed).contiguous())   # [1, Ci, 3, 3]
        y = torch.empty((N, 1, H, W), dtype=x.dtype, device=x.device)
        _native.launch('tai_conv_cout1_3x3_forward', x.device, x, wd, bias, y, N, Ci, H, W, _ACT[act])
        ctx.act, ctx.transposed = act, transposed
        ctx.save_for_backward(x, weight, y if act is not None else None)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, y = ctx.saved_tensors
        g = grad_out.contiguous()
        if ctx.act == 'relu':
            g = torch.ops.aten.threshold_backward(g, y, 0)
        elif ctx.act == 'tanh':
            g = torch.ops.aten.tanh_backward(g, y)                  # g * (1 - y^2): one kernel
        N, Ci, H, W = x.shape
        wd = _cached(weight, ('direct', ctx.transposed), lambda: _as_conv_weight(weight.detach(), ctx.transposed).contiguous())
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            # d/dx_c of sum_c conv(x_c, wd[0, c]) is conv(g, wd[0, c] flipped): Ci output channels from the one-channel g
            wf = wd.flip(2, 3).transpose(0, 1).contiguous()                           # [Ci, 1, 3, 3]
            gx = torch.empty_like(x)
            zero = _zero_bias(Ci, x.device)
            _native.launch('tai_conv_cin1_forward', x.device, g, wf, zero, gx, N, Ci, H, W, 3, 0)
        if ctx.needs_input_grad[1]:
            # dwd[0][c][a][b] = sum g[y, x] x_c[y + a - 1, x + b - 1] = thin_weight_grad(x, g)[c][2 - a][2 - b]
            dwd = thin_weight_grad(x, g, 3)[0].flip(1, 2).unsqueeze(0)               # [1, Ci, 3, 3] in conv2d layout
            gw = _as_conv_weight(dwd, ctx.transposed).contiguous().view_as(weight)
        if ctx.needs_input_grad[2]:
            gb = g.sum().view(1)
        return gx, gw, gb, None, None


class _ActPool2x2(torch.autograd.Function):
    """(y, max_pool2d(y, 2)) with y = relu(z) or z, under autograd: one pass forward, and ONE pass backward for what ATen
    runs as max_pool2d backward + the sum of the two gradient paths into y + threshold_backward."""

    @staticmethod
    def forward(ctx, z, relu):
        z = z.contiguous()
        N, C, H, W = z.shape
        y = torch.empty_like(z)
        yp = torch.empty((N, C, H // 2, W // 2), dtype=z.dtype, device=z.device)
        _native.launch('tai_act_maxpool2x2_forward', z.device, z, y, yp, N * C, H, W, int(relu))
        ctx.relu = bool(relu)
        ctx.save_for_backward(y)
        return y, yp

    @staticmethod
    def backward(ctx, gy, gyp):
        y, = ctx.saved_tensors
        N, C, H, W = y.shape
        gy = gy.contiguous() if gy is not None else None
        gyp = gyp.contiguous() if gyp is not None else None
        gz = torch.empty_like(y)
        _native.launch('tai_act_maxpool2x2_backward', y.device, gy, gyp, y, gz, N * C, H, W, int(ctx.relu))
        return gz, None


class _Layer(object):
    """What one convolution call is -- asked once, for conv_route and for the launch that follows.  ``x``: a tensor or a list / tuple of up
    to four channel parts (``listed``); ``addx``: the tensor conv_bias_unpool_add unpools into the sum."""
    __slots__ = ('parts', 'listed', 'x0', 'weight', 'bias', 'padding', 'act', 'transposed', 'addx', 'Ci', 'Co', 'kh', 'kw',
                 'N', 'Cp', 'H', 'W', 'cuda_fp32', 'native')

    def __init__(self, x, weight, bias, padding, act, transposed=False, addx=None):
        self.listed = isinstance(x, (list, tuple))
        self.parts = list(x) if self.listed else [x]
        x0 = self.x0 = self.parts[0]
        self.weight, self.bias, self.padding, self.act, self.transposed, self.addx = weight, bias, padding, act, transposed, addx
        self.Co, self.Ci = (weight.shape[1], weight.shape[0]) if transposed else (weight.shape[0], weight.shape[1])
        self.kh, self.kw = weight.shape[2], weight.shape[3]
        self.cuda_fp32 = torch.is_tensor(x0) and x0.is_cuda and x0.dtype == torch.float32
        self.native = self.cuda_fp32 and bias is not None          # what every in-tree kernel needs: cuda, fp32, a bias
        # (a CPU tensor is never unpacked: it goes to ATen in whatever shape ATen takes)
        self.N, self.Cp, self.H, self.W = x0.shape if self.cuda_fp32 or self.listed or addx is not None else (None,) * 4

    def parts_fit(self):
        """at most four parts of one shape and dtype that make up the weight's input channels"""
        x0, n = self.x0, len(self.parts)
        return n <= 4 and self.Cp * n == self.Ci and all(p.shape == x0.shape and p.dtype == x0.dtype for p in self.parts)

    def parts_in_place(self):
        """... that the Winograd kernels read where they lie"""
        return self.parts_fit() and self.Cp % 8 == 0 and all(p.is_contiguous() for p in self.parts)

    def addx_fits(self):
        a = self.addx
        return a.is_cuda and a.dtype == torch.float32 and tuple(a.shape) == (self.N, self.Co, self.H // 2, self.W // 2)

    def no_grad(self):
        """no gradient is needed under the current grad mode"""
        return _no_grad_needed(self.weight, self.bias, self.addx, *self.parts)

    def bf16(self):
        """the bf16 kernel takes it (bf16 mode, no gradient needed, a layer _bf16_ok takes)"""
        return (_CONV_PREC[0] == 'bf16' and self.native and self.parts_fit()
                and _bf16_route(self.Ci, self.Co, self.kh, self.kw, self.padding, self.weight, self.bias, self.addx, *self.parts))

    def thin_in(self):
        """one input channel: csrc/thin_conv.hip.inc streams the wide output"""
        return self.Ci == 1 and self.kh == self.kw and self.kh in (3, 5) and self.padding == self.kh // 2 and self.Co >= 16

    def thin_out(self):
        return self.Co == 1 and self.kh == self.kw == 3 and self.padding == 1 and self.Ci >= 16


# route name -> what runs ("Convolution dispatch", has the conditions)
ROUTES = {
    'bf16': 'tai_conv_bf16_forward (_bf16_conv), every epilogue',
    'thin_in': 'tai_conv_cin1_forward / tai_conv_cin1_forward_maxpool',
    'thin_out': 'tai_conv_cout1_3x3_forward',
    'kxk': 'tai_conv_shift_stack + tai_conv3x3_wino_forward_window (_kxk_as_wino)',
    'wino43': 'F(4x4, 3x3): tai_conv3x3_wino43_forward_ws (_wino43_launch), every epilogue, 1-4 parts',
    'wino': 'F(2x2, 3x3): tai_conv3x3_wino_forward / _forward_maxpool / _forward_ex (unpool_add)',
    'wino_odd': 'F(2x2, 3x3) on a plane with an odd side: tai_conv3x3_wino_forward_ex',
    'wino_parts': 'F(2x2, 3x3) over 2-4 parts: tai_conv3x3_wino_forward_parts',
    'miopen': 'F.conv2d without bias + tai_bias_act_inplace',
    'cat': 'torch.cat of the parts, then the route of the concatenation',
    'autograd_3x3': '_WinoConv3x3', 'autograd_parts': '_WinoConv3x3Parts', 'autograd_kxk': '_WinoConvKxK',
    'autograd_thin_in': '_ThinInConv', 'autograd_thin_out': '_ThinOutConv',
    'aten': 'F.conv2d with bias + torch.relu / torch.tanh (CPU tensors, no bias, other dtypes, gradients no kernel takes)',
    'act_pool': 'pool: conv_bias_act without activation, then _ActPool2x2',
    'unfused': 'pool / unpool_add: conv_bias_act, then F.max_pool2d / unpool2x_add',
}


def conv_route(l, epilogue=None):
    """The route (a key of ROUTES) of layer ``l`` (_Layer) with ``epilogue`` None (conv_bias_act), 'pool' (conv_bias_act_maxpool) or
    'unpool_add' (conv_bias_unpool_add).  Needs no GPU.  _wino_ok and _wino43_ok are looked up in the module at every call and asked in
    a fixed order, each at most once per question: tests replace them to route a small batch like a large one and count the answers."""
    N, Ci, Co, H, W, kh, kw, padding, n = l.N, l.Ci, l.Co, l.H, l.W, l.kh, l.kw, l.padding, len(l.parts)
    if epilogue == 'unpool_add':
        if l.native and l.addx_fits():
            if H % 2 == 0 and W % 2 == 0 and l.bf16():
                return 'bf16'
            if (l.parts_fit() and (n == 1 or l.Cp % 8 == 0) and l.no_grad() and _wino_ok(N, Ci, Co, H, W, kh, kw, padding)
                    and N * Co * H * W < 2 ** 29):
                return 'wino43' if _wino43_ok(N, Ci, Co, H, W, n, l.weight) else 'wino'     # a 4 x 4 tile holds four unpooling cells
        return 'unfused'
    if epilogue == 'pool':
        if l.listed or not l.cuda_fp32:
            return 'unfused'
        if H % 2 == 0 and W % 2 == 0 and l.bf16():
            return 'bf16'
        if l.act in (None, 'relu') and H % 2 == 0 and W % 4 == 0:
            if l.native and l.no_grad():
                if l.thin_in():
                    return 'thin_in'
                if _kxk_ok(N, Ci, Co, H, W, kh, kw, padding):
                    return 'kxk'
                if _wino_ok(N, Ci, Co, H, W, kh, kw, padding):
                    return 'wino43' if _wino43_ok(N, Ci, Co, H, W, 1, l.weight) else 'wino'    # a 4 x 4 tile is four pooling windows
            if torch.is_grad_enabled():
                # training: the convolution without its activation, then activation + pool as one Function (one backward pass for
                # the pool's scatter, the sum of the two gradient paths into y and the ReLU mask)
                return 'act_pool'
        return 'unfused'
    if l.bf16():
        return 'bf16'
    if l.listed:
        if l.native and l.parts_in_place():
            if l.no_grad() and _wino_ok(N, Ci, Co, H, W, kh, kw, padding, ragged=True):
                return 'wino43' if _wino43_ok(N, Ci, Co, H, W, n, l.weight) else 'wino_parts'
            if (kh == kw == 3 and torch.is_grad_enabled() and _wino_ok(N, Ci, Co, H, W, 3, 3, padding, ragged=True)
                    and _wino_ok(N, Co, l.Cp, H, W, 3, 3, padding, ragged=True) and PARTS_UNDER_AUTOGRAD):
                return 'autograd_parts'                      # training: the parts are read where they lie
        return 'cat'
    if not l.native:
        return 'aten'
    if not l.no_grad():
        if kh == kw == 3:
            # (min_ci 2: the 3-channel layers of c_dim 3 -- ContentEnc's first, DecCnn's last -- run in-tree too: their input / output
            # gradient is a convolution with 3 output / input channels, padded to one 64-channel block; MIOpen's kernels sum with atomics)
            mc = 2 if RAGGED_ROUTES[0] else 8
            if _wino_ok(N, Ci, Co, H, W, 3, 3, padding, min_ci=mc, ragged=True) and _wino_ok(N, Co, Ci, H, W, 3, 3, padding, min_ci=mc, ragged=True):
                return 'autograd_3x3'
        if (not l.transposed and kh == kw and kh in (5, 7) and _kxk_ok(N, Ci, Co, H, W, kh, kh, padding)
                and _kxk_ok(N, Co, Ci, H, W, kh, kh, padding)):
            return 'autograd_kxk'
        if W % 4 == 0 and l.thin_in() and not l.transposed and l.act in (None, 'relu'):
            return 'autograd_thin_in'
        if W % 4 == 0 and l.thin_out():
            return 'autograd_thin_out'
        return 'aten'
    if W % 4 == 0 and l.thin_in() and l.act in (None, 'relu'):
        return 'thin_in'
    if W % 4 == 0 and l.thin_out():
        return 'thin_out'
    if not l.transposed and _kxk_ok(N, Ci, Co, H, W, kh, kw, padding):
        return 'kxk'
    if _wino_ok(N, Ci, Co, H, W, kh, kw, padding, min_ci=2, ragged=True):
        if _wino43_ok(N, Ci, Co, H, W, 1, l.weight):
            return 'wino43'
        return 'wino' if H % 2 == 0 and W % 2 == 0 else 'wino_odd'
    return 'miopen'


def _part_pointers(parts):
    return (ctypes.c_void_p * len(parts))(*[p.data_ptr() for p in parts])


def conv_bias_unpool_add(x, weight, bias, padding, addx, keep_plain=True):
    """(y, y + fixed_unpooling(addx)) with y = conv(x) + bias, no activation: the last convolution of a Residual block
    (mcnet.py:172-176) and DecCnn's unpool + residual add (mcnet.py:234-236) -- a Winograd tile is one unpooling cell, so
    the sum is a second output of the convolution's epilogue.  ``x`` may be a tuple of cat operands.  ``keep_plain=False``:
    only the sum is produced (returns (None, sum)): nothing reads the full-resolution residual itself."""
    l = _Layer(x, weight, bias, padding, None, addx=addx)
    route = conv_route(l, 'unpool_add')
    if route == 'bf16':
        return _bf16_conv(l.parts, weight, bias, None, addx=addx, keep_plain=keep_plain)
    if route == 'unfused':
        from .mcnet import unpool2x_add
        y = conv_bias_act(x, weight, bias, padding, None)
        return (y if keep_plain else None), unpool2x_add(addx, y)
    N, Ci, Co, H, W = l.N, l.Ci, l.Co, l.H, l.W
    parts = [q.contiguous() for q in l.parts]
    addx = addx.contiguous()
    y = torch.empty((N, Co, H, W), dtype=torch.float32, device=l.x0.device)
    y2 = torch.empty_like(y) if keep_plain else None
    ptrs = _part_pointers(parts)
    if route == 'wino43':
        _wino43_launch(ptrs, len(parts), _transformed_weights(weight, False, 4), bias, y, N, Ci, Co, H, W, 0, weight, addx=addx, y2=y2)
    else:
        _native.launch('tai_conv3x3_wino_forward_ex', y.device, ptrs, len(parts), 0, _transformed_weights(weight, False, 2), bias, y,
                       None, 0, 0, 0, 0, addx, y2, N, Ci, Co, H, W, H, W, 0, 0, 0)
    return (y, y2) if keep_plain else (None, y)


def conv_bias_act_maxpool(x, weight, bias, padding, act):
    """(y, max_pool2d(y, 2)) with y = conv_bias_act(x, ...): the kernels that own a whole 2x2 window per lane (Winograd,
    one-input-channel) write the pooled tensor in their epilogue instead of leaving a second pass over y to ATen."""
    l = _Layer(x, weight, bias, padding, act)
    route = conv_route(l, 'pool')
    if route == 'bf16':
        return _bf16_conv([x], weight, bias, act, pool=True)
    if route == 'kxk':
        return _kxk_as_wino(x, weight, bias, act, True)
    if route == 'act_pool':
        return _ActPool2x2.apply(conv_bias_act(x, weight, bias, padding, None), act == 'relu')
    if route == 'unfused':
        y = conv_bias_act(x, weight, bias, padding, act)
        return y, F.max_pool2d(y, 2)
    N, Ci, Co, H, W = l.N, l.Ci, l.Co, l.H, l.W
    x = x.contiguous()
    y = torch.empty((N, Co, H, W), dtype=x.dtype, device=x.device)
    yp = torch.empty((N, Co, H // 2, W // 2), dtype=x.dtype, device=x.device)
    if route == 'thin_in':
        _native.launch('tai_conv_cin1_forward_maxpool', x.device, x, weight.contiguous(), bias, y, yp, N, Co, H, W, l.kh, _ACT[act])
    elif route == 'wino43':
        _wino43_launch(_part_pointers([x]), 1, _transformed_weights(weight, False, 4), bias, y, N, Ci, Co, H, W, _ACT[act], weight, ypool=yp)
    else:
        _native.launch('tai_conv3x3_wino_forward_maxpool', x.device, x, _transformed_weights(weight, False, 2), bias, y, yp,
                       N, Ci, Co, H, W, _ACT[act])
    return y, yp


def conv_bias_act(x, weight, bias, padding, act, transposed=False, out=None):
    """act(conv2d(x, weight, stride 1, padding) + bias), act in {None, 'relu', 'tanh'}.  ``transposed``: ``weight`` is
    the [in, out, 3, 3] weight of a ConvTranspose2d(k 3, stride 1, padding 1), which is the same convolution with the
    weight transposed and flipped.  ``x`` may be a list of up to four tensors, meaning their concatenation along the
    channels; the Winograd kernel reads the parts where they lie, every other path concatenates them first.
    ``out``: a contiguous tensor (e.g. a batch slice of a larger buffer) to receive the result; the Winograd paths write it
    directly, every other path copies into it."""
    if out is not None:
        y = _conv_bias_act(x, weight, bias, padding, act, transposed, out)
        if y is not out:
            out.copy_(y)
        return out
    return _conv_bias_act(x, weight, bias, padding, act, transposed, None)


def _conv_bias_act(x, weight, bias, padding, act, transposed, out):
    l = _Layer(x, weight, bias, padding, act, transposed)
    route = conv_route(l)
    if route == 'bf16':
        return _bf16_conv(l.parts, weight, bias, act, transposed, out)
    if route == 'cat':
        return _conv_bias_act(torch.cat(l.parts, dim=1), weight, bias, padding, act, transposed, out)
    if route == 'aten':
        y = F.conv2d(x, _as_conv_weight(weight, transposed), bias, stride=1, padding=padding)
        return torch.relu(y) if act == 'relu' else (torch.tanh(y) if act == 'tanh' else y)
    if route == 'autograd_parts':
        return _WinoConv3x3Parts.apply(weight, bias, act, transposed, *l.parts)
    if route == 'autograd_3x3':
        return _WinoConv3x3.apply(x, weight, bias, act, transposed)      # training: autograd through the HIP kernel
    if route == 'autograd_kxk':
        return _WinoConvKxK.apply(x, weight, bias, act)
    if route == 'autograd_thin_in':
        return _ThinInConv.apply(x, weight, bias, act)
    if route == 'autograd_thin_out':
        return _ThinOutConv.apply(x, weight, bias, act, transposed)
    if route == 'kxk':
        return _kxk_as_wino(x, weight, bias, act, False)
    N, Ci, Co, H, W = l.N, l.Ci, l.Co, l.H, l.W
    if route in ('thin_in', 'thin_out'):
        # one input or one output channel: no GEMM in it, a stream of the wide tensor (csrc/thin_conv.hip.inc)
        x = x.contiguous()
        w = _cached(weight, ('direct', transposed), lambda: _as_conv_weight(weight.detach(), transposed).contiguous())
        y = torch.empty((N, Co, H, W), dtype=x.dtype, device=x.device)
        if route == 'thin_in':
            _native.launch('tai_conv_cin1_forward', x.device, x, w, bias, y, N, Co, H, W, l.kh, _ACT[act])
        else:
            _native.launch('tai_conv_cout1_3x3_forward', x.device, x, w, bias, y, N, Ci, H, W, _ACT[act])
        return y
    if route == 'miopen':
        w = _cached(weight, ('direct', transposed), lambda: _as_conv_weight(weight.detach(), transposed).contiguous()) \
            if transposed else weight
        y = F.conv2d(x, w, None, stride=1, padding=padding)
        if not y.is_contiguous():
            y = y.contiguous()
        N, C, H, W = y.shape
        _native.launch('tai_bias_act_inplace', y.device, y, bias, N, C, H * W, _ACT[act])
        return y
    # the Winograd kernels on the fp32 MFMA pipe (csrc/wino43_conv.hip.inc, csrc/wino_conv.hip.inc); they write ``out`` directly
    parts = [p.contiguous() for p in l.parts]
    x0 = parts[0]
    y = out if _usable_out(out, (N, Co, H, W), x0) else torch.empty((N, Co, H, W), dtype=x0.dtype, device=x0.device)
    if route == 'wino43':            # wide layer: F(4x4, 3x3) (set_winograd_tile)
        _wino43_launch(_part_pointers(parts), len(parts), _transformed_weights(weight, transposed, 4), bias, y, N, Ci, Co, H, W,
                       _ACT[act], weight)
    elif route == 'wino_parts':
        _native.launch('tai_conv3x3_wino_forward_parts', y.device, _part_pointers(parts), len(parts),
                       _transformed_weights(weight, transposed, 2), bias, y, N, Ci, Co, H, W, _ACT[act])
    else:
        _wino_forward(x0, _transformed_weights(weight, transposed, 2), bias, y, N, Ci, Co, H, W, act)
    return y
