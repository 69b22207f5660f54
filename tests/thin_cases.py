"""Case generators for the kernel-level tests of the thin-layer and pointwise kernels (tests/test_gpu_thin_kernels.py):
csrc/thin_conv.hip.inc, csrc/bias_act.hip.inc, the window_scale_* tails of csrc/spectral_norm.hip.inc and the `pairs` kernel
of csrc/upsample.hip.inc.  Their conditions are checked without a GPU in tests/test_thin_cases_cpu.py.

Data:
  * ``conv_int_case`` / ``wrw_int_case``: small integers stored in fp32 (operands in [-4, 4], weights in [-3, 3] and never
    zero, bias in [-8, 8]) with +-OUTLIER on the pixels where a kernel changes hands: both outer columns of the quads of lanes 0
    and 63 of a wave, row ends, image corners, the first and last row of every thin_wrw row segment, the last work item of the
    first grid-stride pass and the first of the second.  Every partial sum is an integer below 2^24 (asserted per case in
    test_thin_cases_cpu.py), so any fp32 order, fused or not, gives the fp64 reference's value: the comparison is torch.equal.
  * ``conv_float_case``: tests/test_gpu_thin_conv.py's data (N(0, 1) operands, weights N(0, 0.1)) for the tanh form.
  * the pointwise kernels are one fp32 operation per element and take any finite floats; ``quantised`` makes the operands of
    the window_scale forward (a product and a sum, which a compiler may or may not contract) exact either way.

The launch constants restate csrc/capi_pointwise.inc's launchers and the kernels' own arithmetic; the CPU test reads them back
from the sources, so that a changed cap fails there first.

The upsample's gradient kernel caps its grid at 65,536 blocks: crossing that needs 16.8 M work items of four gradient
elements each, a 1 GB gradient.  It is left out.
"""
import torch
import torch.nn.functional as F

THREADS = 256           # every kernel here: __launch_bounds__(256), launched with 256 threads
WAVE = 64
OUTLIER = 512.0
CAP = float(2 ** 24)
CGROUPS = 4             # conv_cin1 / conv_cin1_pool: gridDim.y when the output channels are split ...
CGROUP_MIN_CO = 16      # ... which needs at least this many of them ...
CGROUP_MAX_WORK = 4 * 262144        # ... and fewer work items than this
WRW_LANES = 256         # thin_wrw: nsub = max(1, 256 / (W / 4)) row segments per plane
UPS_XBLOCKS = 64        # upsample2x_align_corners_pairs: x-blocks per plane

# launcher -> cap of gridDim.x (blocks of 256 work items; for the scalar window_scale forms: planes, one per block)
BLOCK_CAPS = {
    'cin1': 8192, 'cin1_pool': 8192, 'cout1_3x3': 8192, 'cout1_5x5': 8192,
    'bias_act_vec4': 16384, 'bias_act_scalar': 16384, 'unpool': 16384, 'convlstm': 16384, 'act_pool': 16384,
    'shift_stack': 16384, 'window_scale': 16384, 'window_scale_scalar': 16384, 'upsample_pairs': UPS_XBLOCKS,
}


def shape_id(s):
    return 'x'.join(str(d) for d in s)


# ---- what a launch does with a shape -------------------------------------------------------------------------------------

def work(launcher, shape):
    """Work items the launcher counts its blocks from (per plane for the upsample, planes for the scalar window_scale)."""
    if launcher == 'cin1':
        N, Co, H, W, k = shape
        return N * H * (W // 4)
    if launcher == 'cin1_pool':
        N, Co, H, W, k = shape
        return N * (H // 2) * (W // 4)
    if launcher in ('cout1_3x3', 'cout1_5x5'):
        N, Ci, H, W = shape
        return N * H * (W // 4)
    if launcher == 'bias_act_vec4':
        N, C, HW = shape
        assert HW % 4 == 0
        return N * C * HW // 4
    if launcher == 'bias_act_scalar':
        N, C, HW = shape
        return N * C * HW
    if launcher == 'unpool':
        planes, h, w = shape
        return planes * 2 * h * (2 * w // 4)
    if launcher == 'convlstm':
        N, Fe, HW = shape
        return N * Fe * (HW // 4)
    if launcher == 'act_pool':
        planes, H, W = shape
        return planes * (H // 2) * (W // 4)
    if launcher == 'shift_stack':
        N, C, H, W, k = shape
        S = {5: 2, 7: 3}[k]
        return N * S * S * C * (H + 2) * ((W + 4) // 4)
    if launcher == 'window_scale':
        nw, B, C, HW = shape
        return nw * B * C * (HW // 4)
    if launcher == 'window_scale_scalar':
        nw, B, C, HW = shape
        return nw * B * C
    if launcher == 'upsample_pairs':
        planes, H, W = shape
        return H * (2 * W // 4)
    raise KeyError(launcher)


def pass_items(launcher):
    """Work items one pass of the capped grid covers."""
    return BLOCK_CAPS[launcher] * (1 if launcher == 'window_scale_scalar' else THREADS)


def passes(launcher, shape):
    """Largest number of iterations of the grid-stride loop any thread (or, scalar window_scale, any block) runs."""
    return -(-work(launcher, shape) // pass_items(launcher))


def strides(launcher, shape):
    return passes(launcher, shape) > 1


def second_pass(launcher, shape):
    """(first, last) work item of the second pass."""
    assert passes(launcher, shape) == 2
    return pass_items(launcher), work(launcher, shape) - 1


def item_slices(launcher, shape, idx):
    """Where work item `idx` writes -> (view shape of the output, index).  The output of cin1_pool / act_pool meant here is
    the full-resolution one; of convlstm: new_c (new_h alike); of unpool / bias_act / window_scale: the one tensor."""
    if launcher in ('cin1', 'cout1_3x3', 'cout1_5x5'):
        N, C, H, W = shape[:4]
        qw = W // 4
        q, yy, n = idx % qw, idx // qw % H, idx // (qw * H)
        return (N, -1, H, W), (n, slice(None), yy, slice(4 * q, 4 * q + 4))
    if launcher == 'cin1_pool':
        N, C, H, W = shape[:4]
        qw, hh = W // 4, H // 2
        q, yr, n = idx % qw, idx // qw % hh, idx // (qw * hh)
        return (N, -1, H, W), (n, slice(None), slice(2 * yr, 2 * yr + 2), slice(4 * q, 4 * q + 4))
    if launcher == 'act_pool':
        planes, H, W = shape
        w4, h2 = W // 4, H // 2
        q, pr = idx % w4, idx // w4
        return (planes, H, W), (pr // h2, slice(2 * (pr % h2), 2 * (pr % h2) + 2), slice(4 * q, 4 * q + 4))
    if launcher == 'upsample_pairs':
        planes, H, W = shape
        qw = 2 * W // 4
        r, q = idx // qw, idx % qw
        return (planes, 2 * H, 2 * W), (slice(None), slice(2 * r, 2 * r + 2), slice(4 * q, 4 * q + 4))
    if launcher == 'window_scale_scalar':
        nw, B, C, HW = shape
        return (nw * B * C, HW), (idx, slice(None))
    if launcher == 'bias_act_scalar':
        return (-1,), (slice(idx, idx + 1),)
    # one 16-byte store per item, items in the order of the (contiguous) output
    return (-1,), (slice(4 * idx, 4 * idx + 4),)


def wrw_segments(H, W):
    """thin_wrw's cut of a plane -> (nsub, rs, rows of the last non-empty segment, items a lane walks at most)."""
    qw = W // 4
    nsub = max(1, WRW_LANES // qw)
    rs = -(-H // nsub)
    used = -(-H // rs)
    return nsub, rs, H - (used - 1) * rs, -(-(qw * nsub) // THREADS)


def wrw_rows_per_segment(H, W):
    return wrw_segments(H, W)[1]


def wrw_segment_rows(H, W):
    """[(first row, last row)] of the non-empty segments."""
    nsub, rs, _, _ = wrw_segments(H, W)
    return [(y0, min(H, y0 + rs) - 1) for y0 in range(0, H, rs)]


def cin1_channel_groups(launcher, shape):
    """(gridDim.y, channels per group, channels of the last group that has any; groups left empty)."""
    Co = shape[1]
    groups = CGROUPS if work(launcher, shape) < CGROUP_MAX_WORK and Co >= CGROUP_MIN_CO else 1
    cg = -(-Co // groups)
    used = -(-Co // cg)
    return groups, cg, Co - (used - 1) * cg, groups - used


def dpp_own_loads(shape):
    """conv_cout1_3x3: number of work items that are lane 0 of a wave with a left neighbour in their row, or lane 63 with a
    right one -- the lanes that load an edge column themselves instead of taking it from the next lane."""
    N, Ci, H, W = shape
    qw = W // 4
    total = N * H * qw
    left = sum(1 for i in range(0, total, WAVE) if i % qw > 0)
    right = sum(1 for i in range(WAVE - 1, total, WAVE) if i % qw < qw - 1)
    return left, right


def flanks_5x5(W):
    """conv_cout1_5x5: {(has a left flank, has a right flank)} over the quads of a row."""
    return {(4 * q >= 2, 4 * q + 6 <= W) for q in range(W // 4)}


# ---- shapes, each with the condition it is there for ---------------------------------------------------------------------

WRW_SHAPES = [                  # (N, Cb, H, W), each at k in {3, 5}
    (2, 3, 7, 256),             # nsub = 4, rs = 2, the last segment is one row
    (1, 2, 24, 128),            # nsub = 8, rs = 3, exact
    (2, 1, 23, 128),            # rs = 3, the last segment is two rows
    (1, 2, 5, 16),              # nsub = 64: more segments than rows, rs = 1
    (1, 1, 3, 1028),            # 257 quads per row: two items for lane 0
    (3, 5, 6, 36),              # 9 quads: nsub = 28, the items do not fill the block
]
WRW_OUTPUTS = ['both', 'dw', 'db']

CIN1_CO = [1, 5, 16, 17, 21, 64]        # one group (< 16), four exact groups, ragged groups (cg = 5 and 6), production
CIN1_PLANES = [(2, 6, 4), (3, 10, 36), (1, 16, 260)]    # (N, H, W): one quad per row; 9 quads; 65 quads (neither divides 64)
CIN1_SHAPES = [(N, Co, H, W) for (N, H, W) in CIN1_PLANES for Co in CIN1_CO]
# the pooled output as a window of a larger plane: (pool_oy, pool_ox, extra rows, extra columns); None: plain H/2 x W/2
POOL_WINDOWS = [None, (0, 0, 0, 0), (2, 4, 1, 2), (1, 3, 2, 4), (3, 2, 0, 3), (1, 1, 1, 0)]     # even / odd origins, odd pool_w

COUT1_CI = [1, 3, 4, 5, 17, 64]         # below, at and above the unroll of 4 (3x3) and 2 (5x5); production
COUT1_W = [4, 8, 36, 256, 260]          # one quad (no neighbour, no flank); two; 9 and 65 (lanes 0 / 63 load their own); 64
COUT1_H = [1, 2, 5]                     # every row clamped; one clamped row each; interior rows
COUT1_N = 2
COUT1_SHAPES = [(COUT1_N, Ci, H, W) for Ci in COUT1_CI for H in COUT1_H for W in COUT1_W]

# one shape per launcher whose work is just past cap x 256 (a second pass of a few thousand items), narrow dimension at 1-2
STRIDED = {
    'cin1': (2, 2, 1026, 4096, 5),              # 2,101,248 items against 2,097,152
    'cin1_pool': (2, 1, 2052, 4096, 3),         # 2,101,248
    'cout1_3x3': (2, 2, 1026, 4096),            # 2,101,248
    'cout1_5x5': (2, 2, 1026, 4096),
    'bias_act_vec4': (2, 2, 4198400),           # 4,198,400 quads against 4,194,304
    'bias_act_scalar': (1, 2, 2099201),         # 4,198,402 elements, HW % 4 = 1
    'unpool': (2, 1025, 2048),                  # 2 x 2050 x 1024 = 4,198,400
    'convlstm': (2, 1, 8396800),                # 4,198,400
    'act_pool': (2, 2050, 8192),                # 2 x 1025 x 2048 = 4,198,400
    'shift_stack': (1, 1, 2046, 2048, 5),       # 4 x 2048 x 513 = 4,202,496
    'window_scale': (2, 1, 2, 4198400),         # 4,198,400
    'window_scale_scalar': (4, 2050, 2, 6),     # 16,400 planes against 16,384
    'upsample_pairs': (2, 192, 192),            # 18,432 items per plane against 64 x 256 = 16,384
}

GATE_HW = [4, 60, 256]
GATE_F = [1, 16]
GATE_FORGET_BIAS = [0.0, 1.0, 2.5]
GATE_PATHS = ['both', 'h_only', 'c_only']
GATE_N = 3

ACT_POOL_SHAPES = [(3, 2, 4), (2, 4, 8), (5, 6, 36), (2, 12, 260)]      # (planes, H, W): one item per plane; ...; 65 quads
BIAS_ACT_SHAPES = [(2, 3, 4), (1, 5, 6), (3, 2, 1), (2, 7, 60), (1, 3, 1028), (2, 3, 13)]      # (N, C, HW): vec4 and scalar
UNPOOL_SHAPES = [(1, 1, 2), (3, 1, 4), (5, 3, 6), (2, 7, 130)]          # (planes, h, w)
SHIFT_STACK_SHAPES = [(1, 1, 1, 4, 5), (2, 3, 5, 8, 5), (1, 2, 6, 36, 7), (2, 1, 3, 4, 7)]     # (N, C, H, W, k)
WINDOW_SCALE_SHAPES = [(3, 2, 5, 4), (2, 1, 3, 60), (13, 2, 4, 6), (2, 3, 7, 1), (1, 1, 2, 130)]     # (nw, B, C, HW)


# ---- data --------------------------------------------------------------------------------------------------------------

def _ri(g, lo, hi, *s):
    return torch.randint(lo, hi + 1, s, generator=g).float()


def _nonzero(t):
    """Zeros become +1 / -1 alternately: every weight counts, so a dropped or misplaced term always moves the sum."""
    flat = t.reshape(-1)
    alt = torch.ones_like(flat)
    alt[1::2] = -1
    return torch.where(flat == 0, alt, flat).view(t.shape)


def seam_items(launcher, shape):
    """Work items whose pixels get outliers: lanes 0 and 63 of the first ten waves, and, where the launch strides, the last item
    of the first pass, the first of the second (and that wave's lane 63) and the last item of all."""
    total = work(launcher, shape)
    items = [i for i in range(min(total, 10 * WAVE)) if i % WAVE in (0, WAVE - 1)]
    if strides(launcher, shape):
        first = pass_items(launcher)
        items += [first - 1, first, first + WAVE - 1, first + WAVE, total - 1]
    return sorted(set(i for i in items if 0 <= i < total))


def conv_outlier_sites(launcher, shape):
    """[(n, channel, row, col)] in x for the convolutions: image corners of the first and last image, both ends of a middle row,
    and both outer columns of every quad of seam_items (for the pooled form: its upper row at lane 0, its lower at lane 63).
    One channel per site, cycling."""
    N, C, H, W = shape[:4]
    Ci = 1 if launcher in ('cin1', 'cin1_pool') else C
    qw = W // 4
    where = []
    for n in sorted({0, N - 1}):
        where += [(n, r, c) for r in sorted({0, H // 2, H - 1}) for c in sorted({0, W - 1})]
    for i in seam_items(launcher, shape):
        q = i % qw
        if launcher == 'cin1_pool':
            hh = H // 2
            row, n = 2 * (i // qw % hh) + (1 if i % WAVE == WAVE - 1 else 0), i // (qw * hh)
        else:
            row, n = i // qw % H, i // (qw * H)
        where += [(n, row, 4 * q), (n, row, 4 * q + 3)]
    where = list(dict.fromkeys(where))
    return [(n, k % Ci, r, c) for k, (n, r, c) in enumerate(where)]


def conv_int_case(launcher, shape, seed, outliers=True):
    """(x, w, b) of a thin convolution: x [N, Ci, H, W] in [-4, 4], w [Co, Ci, k, k] in [-3, 3] without zeros, b [Co] in
    [-8, 8]; Ci = 1 for cin1 / cin1_pool (shape (N, Co, H, W, k)), Co = 1 for cout1_3x3 / cout1_5x5 (shape (N, Ci, H, W))."""
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = shape[:4]
    if launcher in ('cin1', 'cin1_pool'):
        Ci, Co, k = 1, C, shape[4]
    else:
        Ci, Co, k = C, 1, 3 if launcher == 'cout1_3x3' else 5
    x = _ri(g, -4, 4, N, Ci, H, W)
    w = _nonzero(_ri(g, -3, 3, Co, Ci, k, k))
    b = _ri(g, -8, 8, Co)
    if outliers:
        for j, (n, c, r, col) in enumerate(conv_outlier_sites(launcher, shape)):
            x[n, c, r, col] = OUTLIER if j % 2 == 0 else -OUTLIER
    return x, w, b


def conv_float_case(shape, seed):
    """tests/test_gpu_thin_conv.py's data for the one-output-channel 3x3 layer: x N(0, 1), w N(0, 0.1), b N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    N, Ci, H, W = shape
    return torch.randn(N, Ci, H, W, generator=g), torch.randn(1, Ci, 3, 3, generator=g) * 0.1, torch.randn(1, generator=g)


def wrw_outlier_sites(shape):
    """([(n, cb, row, col)] in big, [(n, row, col)] in thin).  big: the first and last row of every row segment at columns 0, 3,
    W - 4 and W - 1 (the outer columns of a row's first and last quad; at W = 256 a row is one wave: lanes 0 and 63), and at
    W > 1024 the quad that is lane 0's second item.  thin: the image corners, and the last row of every segment but the last
    with the row after it (the rows two segments both read) at columns 1 and W - 2."""
    N, Cb, H, W = shape
    segs = wrw_segment_rows(H, W)
    cols = sorted({0, 3, W - 4, W - 1} | ({4 * THREADS, 4 * THREADS + 3} if W > 4 * THREADS else set()))
    rows = sorted({r for seg in segs for r in seg})
    big = [(k % N, k % Cb, r, c) for k, (r, c) in enumerate((r, c) for r in rows for c in cols)]
    spots = [(r, c) for r in (0, H - 1) for c in (0, W - 1)]
    spots += [(r, c) for (_, last) in segs[:-1] for r in (last, last + 1) for c in (1, W - 2)]
    spots = list(dict.fromkeys(spots))
    thin = [(k % N, r, c) for k, (r, c) in enumerate(spots)]
    return big, thin


def wrw_int_case(shape, seed, outliers=True):
    """(big [N, Cb, H, W], thin [N, 1, H, W]): integers in [-4, 4] plus the outliers."""
    g = torch.Generator().manual_seed(seed)
    N, Cb, H, W = shape
    big, thin = _ri(g, -4, 4, N, Cb, H, W), _ri(g, -4, 4, N, 1, H, W)
    if outliers:
        bs, ts = wrw_outlier_sites(shape)
        for j, (n, cb, r, c) in enumerate(bs):
            big[n, cb, r, c] = OUTLIER if j % 2 == 0 else -OUTLIER
        for j, (n, r, c) in enumerate(ts):
            thin[n, 0, r, c] = -OUTLIER if j % 2 == 0 else OUTLIER
    return big, thin


def quantised(g, step, lo, hi, *s):
    """Multiples of `step` (a power of two) in [lo, hi] * step."""
    return _ri(g, lo, hi, *s) * step


# ---- plain references ----------------------------------------------------------------------------------------------------

def conv_shifts64(x, w, b):
    """'Same' zero-padded stride-1 convolution in fp64 as a sum of shifted copies, on whatever device x is: the reference of
    the strided cases (F.conv2d in fp64 unfolds the whole image: k * k times its memory)."""
    N, Ci, H, W = x.shape
    Co, _, k, _ = w.shape
    R = k // 2
    xp = F.pad(x.double(), (R, R, R, R))
    wl = w.tolist()
    out = torch.zeros(N, Co, H, W, dtype=torch.float64, device=x.device)
    if b is not None:
        out += b.double().view(1, Co, 1, 1)
    for co in range(Co):
        for ci in range(Ci):
            for r in range(k):
                for c in range(k):
                    out[:, co].add_(xp[:, ci, r:r + H, c:c + W], alpha=wl[co][ci][r][c])
    return out


def wrw_ref64(big, thin, k):
    """(dw [Cb, k, k], db [Cb]) in fp64: dw[cb][a][b] = sum over n, y, x of big[n, cb, y, x] * thin[n, 0, y + a - k/2, x + b - k/2]."""
    N, Cb, H, W = big.shape
    R = k // 2
    tp = F.pad(thin.double(), (R, R, R, R))
    bd = big.double()
    dw = torch.stack([torch.stack([(bd * tp[:, :, a:a + H, b:b + W]).sum(dim=(0, 2, 3)) for b in range(k)], 1) for a in range(k)], 1)
    return dw, bd.sum(dim=(0, 2, 3))


def act_pool_backward_ref(y, gy, gyp, relu):
    """The gradient of z for y = relu(z) or z [planes, H, W] and yp = maxpool2x2(y), from gy and gyp (either may be None): gyp
    goes to the FIRST maximum of each window in row-major order, is added to gy, and the sum is masked by y > 0 (relu)."""
    P, H, W = y.shape
    win = y.view(P, H // 2, 2, W // 2, 2).permute(0, 1, 3, 2, 4).reshape(P, H // 2, W // 2, 4)      # p00, p01, p10, p11
    is_max = win == win.max(dim=-1, keepdim=True).values
    first = is_max & (is_max.int().cumsum(-1) == 1)
    out = torch.zeros_like(y) if gy is None else gy.clone()
    if gyp is not None:
        scat = torch.where(first, gyp.unsqueeze(-1), torch.zeros((), dtype=y.dtype, device=y.device))
        out = out + scat.view(P, H // 2, W // 2, 2, 2).permute(0, 1, 3, 2, 4).reshape(P, H, W)
    return torch.where(y > 0, out, torch.zeros((), dtype=y.dtype, device=y.device)) if relu else out


def shift_stack_ref(x, k):
    """out[n][(a*S + b)*C + c][u][v] = x[n][c][u - 1 + oa][v - 2 + ob] (0 outside), (oa, ob) = (3a - k/2 + 1, 3b - k/2 + 1)."""
    N, C, H, W = x.shape
    S = {5: 2, 7: 3}[k]
    P = 8
    xp = F.pad(x, (P, P, P, P))
    planes = []
    for a in range(S):
        for b in range(S):
            oa, ob = 3 * a - k // 2 + 1, 3 * b - k // 2 + 1
            planes.append(xp[:, :, P - 1 + oa:P - 1 + oa + H + 2, P - 2 + ob:P - 2 + ob + W + 4])
    return torch.cat(planes, 1).contiguous()
