"""Conditions of the case generators in tests/thin_cases.py, without a GPU.

tests/test_gpu_thin_kernels.py compares integer cases with torch.equal.  That is sound only if every partial sum is an integer
below 2^24: a cap, asserted here per case on the ABSOLUTE values of the operands, which bounds every partial sum of any order
and any sign pattern.  Each shape is also held to the condition its comment in thin_cases.py claims (rows per thin_wrw
segment, channel groups, passes of a grid-stride loop, which lanes hold outliers), and the launch constants thin_cases.py
restates are read back from the sources."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import thin_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'video-frame-inpainting_amd', 'csrc')

CONV_LAUNCHERS = ['cin1', 'cin1_pool', 'cout1_3x3', 'cout1_5x5']


def _conv_cases(launcher):
    """Every shape the GPU module runs `launcher` at, the strided one last."""
    if launcher in ('cin1', 'cin1_pool'):
        return [s + (k,) for s in tc.CIN1_SHAPES for k in (3, 5)] + [tc.STRIDED[launcher]]
    return tc.COUT1_SHAPES + [tc.STRIDED[launcher]]


def _abs_cap(x, w, b):
    """The sum of the absolute terms of every output.  fp32 is enough to tell: sums of non-negative integers are exact below
    2^24, and one that reaches 2^24 cannot round back below it."""
    return F.conv2d(x.abs(), w.abs(), b.abs(), padding=w.shape[-1] // 2).double()


@pytest.mark.parametrize('launcher', CONV_LAUNCHERS)
def test_convolution_cases_stay_below_2_to_24(launcher):
    for shape in _conv_cases(launcher):
        _below_cap(launcher, shape)


def _below_cap(launcher, shape):
    x, w, b = tc.conv_int_case(launcher, shape, seed=1)
    for t in (x, w, b):
        assert bool((t == t.round()).all())
    assert bool((w != 0).all()) and float(w.abs().max()) <= 3 and float(b.abs().max()) <= 8
    cap = _abs_cap(x, w, b)
    assert float(cap.max()) < tc.CAP, float(cap.max())
    if x.numel() <= 1 << 20:        # the signed case itself: fp32 equals fp64, integers throughout
        r32 = F.conv2d(x, w, b, padding=w.shape[-1] // 2)
        r64 = F.conv2d(x.double(), w.double(), b.double(), padding=w.shape[-1] // 2)
        assert torch.equal(r32.double(), r64) and torch.equal(r64, r64.round()) and bool((r64.abs() <= cap).all())
        assert torch.equal(tc.conv_shifts64(x, w, b), r64)          # the strided cases' reference is the same function


@pytest.mark.parametrize('launcher', CONV_LAUNCHERS)
def test_convolution_outliers_sit_where_the_kernels_change_hands(launcher):
    for shape in _conv_cases(launcher):
        _outliers_on_the_seams(launcher, shape)


def _outliers_on_the_seams(launcher, shape):
    N, C, H, W = shape[:4]
    x, w, b = tc.conv_int_case(launcher, shape, seed=2)
    plain = tc.conv_int_case(launcher, shape, seed=2, outliers=False)
    assert float(plain[0].abs().max()) <= 4 and torch.equal(plain[1], w) and torch.equal(plain[2], b)
    sites = tc.conv_outlier_sites(launcher, shape)
    assert len({(n, r, c) for n, _, r, c in sites}) == len(sites)
    assert int((x.abs() == tc.OUTLIER).sum()) == len(sites)
    assert all(abs(float(x[s])) == tc.OUTLIER for s in sites)
    where = {(n, r, c) for n, _, r, c in sites}
    assert where >= {(n, r, c) for n in (0, N - 1) for r in (0, H - 1) for c in (0, W - 1)}      # corners, row ends
    assert {ch for _, ch, _, _ in sites} == set(range(min(x.shape[1], len(sites))))              # the channels cycle
    # lanes 0 and 63 of the first waves: both outer columns of their quads
    total, qw = tc.work(launcher, shape), W // 4
    items = tc.seam_items(launcher, shape)
    assert all(i % tc.WAVE in (0, tc.WAVE - 1) or tc.strides(launcher, shape) for i in items)
    assert set(items) >= {i for i in (0, 63, 64, 127) if i < total}
    rows = (H // 2) if launcher == 'cin1_pool' else H
    for i in items:
        q, n = i % qw, i // (qw * rows)
        r = i // qw % rows
        r = 2 * r + (1 if i % tc.WAVE == tc.WAVE - 1 else 0) if launcher == 'cin1_pool' else r
        assert (n, r, 4 * q) in where and (n, r, 4 * q + 3) in where
        # the item that owns the site writes where item_slices says
        view, index = tc.item_slices(launcher, shape, i)
        assert index[0] == n and index[-1] == slice(4 * q, 4 * q + 4)
    again = tc.conv_int_case(launcher, shape, seed=2)
    assert all(torch.equal(a, b_) for a, b_ in zip((x, w, b), again))


@pytest.mark.parametrize('k', [3, 5])
@pytest.mark.parametrize('shape', tc.WRW_SHAPES, ids=tc.shape_id)
def test_weight_gradient_cases_stay_below_2_to_24(shape, k):
    big, thin = tc.wrw_int_case(shape, seed=1)
    assert bool((big == big.round()).all()) and bool((thin == thin.round()).all())
    cap_w, cap_b = tc.wrw_ref64(big.abs(), thin.abs(), k)
    assert float(cap_w.max()) < tc.CAP and float(cap_b.max()) < tc.CAP, (float(cap_w.max()), float(cap_b.max()))
    dw, db = tc.wrw_ref64(big, thin, k)
    assert torch.equal(dw, dw.round()) and bool((dw.abs() <= cap_w).all()) and bool((db.abs() <= cap_b).all())
    # the sum of shifted products is the weight gradient of the convolution: fp64 autograd of F.conv2d, both roles
    N, Cb, H, W = shape
    w = torch.zeros(Cb, 1, k, k, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(Cb, dtype=torch.float64, requires_grad=True)
    gw, gb = torch.autograd.grad(F.conv2d(thin.double(), w, bias, padding=k // 2), (w, bias), big.double())
    assert torch.equal(gw[:, 0], dw) and torch.equal(gb, db)
    w1 = torch.zeros(1, Cb, k, k, dtype=torch.float64, requires_grad=True)
    gw1, = torch.autograd.grad(F.conv2d(big.double(), w1, None, padding=k // 2), (w1,), thin.double())
    assert torch.equal(gw1[0].flip(-1, -2), dw)             # one output channel: big = x, thin = dL/dy, taps flipped


@pytest.mark.parametrize('shape', tc.WRW_SHAPES, ids=tc.shape_id)
def test_weight_gradient_outliers_sit_on_the_segment_seams(shape):
    N, Cb, H, W = shape
    big, thin = tc.wrw_int_case(shape, seed=2)
    plain = tc.wrw_int_case(shape, seed=2, outliers=False)
    assert float(plain[0].abs().max()) <= 4 and float(plain[1].abs().max()) <= 4
    bs, ts = tc.wrw_outlier_sites(shape)
    assert int((big.abs() == tc.OUTLIER).sum()) == len(bs) and int((thin.abs() == tc.OUTLIER).sum()) == len(ts)
    segs = tc.wrw_segment_rows(H, W)
    assert segs[0][0] == 0 and segs[-1][1] == H - 1 and all(a[1] + 1 == b[0] for a, b in zip(segs, segs[1:]))
    rs = tc.wrw_rows_per_segment(H, W)
    assert all(last - first + 1 == rs for first, last in segs[:-1])
    big_rows, big_cols = {r for _, _, r, _ in bs}, {c for _, _, _, c in bs}
    assert big_rows == {r for seg in segs for r in seg} and big_cols >= {0, 3, W - 4, W - 1}
    thin_at = {(r, c) for _, r, c in ts}
    assert thin_at >= {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
    for (_, last), (first, _) in zip(segs, segs[1:]):
        assert {(last, 1), (first, 1), (last, W - 2), (first, W - 2)} <= thin_at


def test_weight_gradient_shapes_reach_what_they_are_listed_for():
    seg = {s: tc.wrw_segments(s[2], s[3]) for s in tc.WRW_SHAPES}
    assert seg[(2, 3, 7, 256)] == (4, 2, 1, 1)              # rs = 2, the last segment one row
    assert seg[(1, 2, 24, 128)] == (8, 3, 3, 1)             # rs = 3, exact
    assert seg[(2, 1, 23, 128)] == (8, 3, 2, 1)             # ragged
    assert seg[(1, 2, 5, 16)] == (64, 1, 1, 1) and 64 > 5   # more segments than rows
    assert seg[(1, 1, 3, 1028)] == (1, 3, 3, 2)             # two items for lane 0: the window restarts inside one lane
    assert seg[(3, 5, 6, 36)] == (28, 1, 1, 1) and 9 * 28 < tc.THREADS
    # what tests/test_gpu_thin_conv.py runs: one row per lane, no carry
    assert tc.wrw_rows_per_segment(24, 40) == 1 and tc.wrw_rows_per_segment(20, 36) == 1
    assert any(tc.wrw_rows_per_segment(s[2], s[3]) > 1 and len(tc.wrw_segment_rows(s[2], s[3])) > 1 for s in tc.WRW_SHAPES)


def test_channel_groups_and_windows():
    groups = {Co: tc.cin1_channel_groups('cin1', (3, Co, 10, 36, 3)) for Co in tc.CIN1_CO}
    assert groups == {1: (1, 1, 1, 0), 5: (1, 5, 5, 0), 16: (4, 4, 4, 0), 17: (4, 5, 2, 0), 21: (4, 6, 3, 0), 64: (4, 16, 16, 0)}
    assert all(tc.cin1_channel_groups('cin1_pool', s + (5,))[0] == (4 if s[1] >= 16 else 1) for s in tc.CIN1_SHAPES)
    # 17 and 21 are the two ways a floor instead of a ceiling loses channels: 4 * (17 // 4) = 16, 4 * (21 // 4) = 20
    assert 4 * (17 // 4) < 17 and 4 * (21 // 4) < 21
    # the strided shapes are past the split's work limit: one group whatever Co
    assert tc.cin1_channel_groups('cin1', (2, 64, 1026, 4096, 5))[0] == 1
    assert [W // 4 for _, _, W in tc.CIN1_PLANES] == [1, 9, 65] and all(H % 2 == 0 for _, H, _ in tc.CIN1_PLANES)
    wins = [w for w in tc.POOL_WINDOWS if w]
    assert {(oy % 2, ox % 2) for oy, ox, _, _ in wins} == {(0, 0), (1, 1), (1, 0)} and None in tc.POOL_WINDOWS
    for N, H, W in tc.CIN1_PLANES:          # odd pool_w with an even origin, an odd origin, and the plain aligned pair store
        odd = {((ox | (W // 2 + ox + ew)) & 1) for _, ox, _, ew in wins}
        assert odd == {0, 1}
        assert any(ox % 2 == 0 and (W // 2 + ox + ew) % 2 == 1 for _, ox, _, ew in wins)


def test_one_output_channel_shapes_reach_what_they_are_listed_for():
    assert tc.COUT1_CI == [1, 3, 4, 5, 17, 64] and tc.COUT1_W == [4, 8, 36, 256, 260] and tc.COUT1_H == [1, 2, 5]
    own = {W: tc.dpp_own_loads((tc.COUT1_N, 1, 5, W)) for W in tc.COUT1_W}
    assert own[4] == (0, 0) and own[8] == (0, 0) and own[256] == (0, 0)         # quads divide 64: every neighbour is a lane
    assert min(own[36]) > 0 and min(own[260]) > 0                               # lanes 0 and 63 load their own
    assert tc.dpp_own_loads((5, 64, 20, 36))[0] > 0                             # (the one shape the older test has)
    assert tc.flanks_5x5(4) == {(False, False)}                                 # no flank at all
    assert tc.flanks_5x5(8) == {(False, True), (True, False)}
    assert tc.flanks_5x5(36) == {(False, True), (True, True), (True, False)}
    # a row's second-to-last quad has a right flank: what `x0 + 8 < W` would take away, from W = 8 on
    assert all((4 * (W // 4 - 2) + 6 <= W) and not (4 * (W // 4 - 2) + 8 < W) for W in tc.COUT1_W if W >= 8)


def test_strided_shapes_run_the_loop_exactly_twice():
    for launcher, shape in tc.STRIDED.items():
        assert tc.passes(launcher, shape) == 2, launcher
        first, last = tc.second_pass(launcher, shape)
        assert first == tc.pass_items(launcher) and 0 < last - first + 1 <= 8192, (launcher, last - first + 1)
    assert set(tc.STRIDED) == set(tc.BLOCK_CAPS)
    # no other shape of the lists strides: the small cases pin values, these pin the loop
    small = ([('cin1', s + (5,)) for s in tc.CIN1_SHAPES] + [('cin1_pool', s + (5,)) for s in tc.CIN1_SHAPES]
             + [('cout1_3x3', s) for s in tc.COUT1_SHAPES] + [('act_pool', s) for s in tc.ACT_POOL_SHAPES]
             + [('unpool', s) for s in tc.UNPOOL_SHAPES] + [('shift_stack', s) for s in tc.SHIFT_STACK_SHAPES]
             + [('window_scale_scalar', s) for s in tc.WINDOW_SCALE_SHAPES]
             + [('convlstm', (tc.GATE_N, f, hw)) for f in tc.GATE_F for hw in tc.GATE_HW])
    assert not any(tc.strides(l, s) for l, s in small)
    # production: act_pool2x2 on [32, 64, 128, 128] is exactly the cap, the discriminator's last layer is past it
    assert tc.work('act_pool', (32 * 64, 128, 128)) == tc.pass_items('act_pool') == 4194304
    assert tc.work('window_scale_scalar', (13, 32, 64, 130)) == 26624 > tc.pass_items('window_scale_scalar')
    assert tc.work('upsample_pairs', (2, 192, 192)) == 18432 > 64 * 256
    assert tc.STRIDED['bias_act_scalar'][2] % 4 == 1 and tc.STRIDED['bias_act_vec4'][2] % 4 == 0
    # item_slices on the second pass: inside the output, the last item ends it
    for launcher, shape in tc.STRIDED.items():
        first, last = tc.second_pass(launcher, shape)
        view, index = tc.item_slices(launcher, shape, last)
        if view == (-1,):
            per = 1 if launcher == 'bias_act_scalar' else 4
            assert index[0].stop == per * tc.work(launcher, shape)


def test_pointwise_shape_lists():
    assert {hw % 4 for _, _, hw in tc.BIAS_ACT_SHAPES} >= {0, 1, 2} and any(hw == 1 for _, _, hw in tc.BIAS_ACT_SHAPES)
    assert any(W == 4 for _, _, W in tc.ACT_POOL_SHAPES) and any(H == 2 for _, H, _ in tc.ACT_POOL_SHAPES)
    assert all(H % 2 == 0 and W % 4 == 0 for _, H, W in tc.ACT_POOL_SHAPES)
    assert all(w % 2 == 0 for _, _, w in tc.UNPOOL_SHAPES) and any(w % 4 == 2 for _, _, w in tc.UNPOOL_SHAPES)
    assert {k for *_, k in tc.SHIFT_STACK_SHAPES} == {5, 7} and all(W % 4 == 0 for _, _, _, W, _ in tc.SHIFT_STACK_SHAPES)
    assert {hw % 4 == 0 for *_, hw in tc.WINDOW_SCALE_SHAPES} == {True, False}
    assert tc.GATE_HW == [4, 60, 256] and tc.GATE_F == [1, 16] and tc.GATE_FORGET_BIAS == [0.0, 1.0, 2.5]
    assert tc.GATE_PATHS == ['both', 'h_only', 'c_only'] and all(hw % 4 == 0 for hw in tc.GATE_HW)


def test_plain_references_agree_with_aten_on_the_cpu():
    g = torch.Generator().manual_seed(5)
    # first-maximum scatter against max_pool2d's own backward, on data full of ties
    z = (torch.randint(-3, 4, (4, 6, 8), generator=g).float() * 0.5).requires_grad_(True)
    for relu in (True, False):
        y = torch.relu(z) if relu else z
        yp = F.max_pool2d(y.unsqueeze(0), 2)[0]
        gy, gyp = torch.randn(y.shape, generator=g), torch.randn(yp.shape, generator=g)
        for use_y, use_p in ((True, True), (False, True), (True, False)):
            loss = ((y * gy).sum() if use_y else 0) + ((yp * gyp).sum() if use_p else 0)
            want, = torch.autograd.grad(loss, z, retain_graph=True)
            got = tc.act_pool_backward_ref(y.detach(), gy if use_y else None, gyp if use_p else None, relu)
            assert torch.equal(got, want)
    ties = tc.act_pool_backward_ref(torch.ones(1, 2, 4), None, torch.tensor([[[2.0, 3.0]]]), False)
    assert torch.equal(ties, torch.tensor([[[2.0, 0, 3.0, 0], [0, 0, 0, 0]]]))
    # the shift stack: a 3x3 convolution over it with the k x k filter cut into blocks is the k x k convolution
    for k in (5, 7):
        S = {5: 2, 7: 3}[k]
        x = torch.randint(-4, 5, (2, 3, 5, 8), generator=g).double()
        w = torch.randint(-3, 4, (2, 3, k, k), generator=g).double()
        stack = tc.shift_stack_ref(x, k)
        assert stack.shape == (2, S * S * 3, 5 + 2, 8 + 4)
        wp = F.pad(w, (0, 3 * S - k, 0, 3 * S - k))
        w3 = torch.cat([wp[:, :, 3 * a:3 * a + 3, 3 * b:3 * b + 3] for a in range(S) for b in range(S)], 1)
        got = F.conv2d(stack, w3)[:, :, :, 1:-1]          # valid 3x3 over the haloed plane whose origin is (1, 2)
        assert torch.equal(got, F.conv2d(x, w, padding=k // 2))


def test_launch_constants_match_the_sources():
    capi = open(os.path.join(CSRC, 'capi_pointwise.inc')).read()          # the launchers of these kernels
    helpers = open(os.path.join(CSRC, 'sepconv_capi.hip')).read()
    thin = open(os.path.join(CSRC, 'thin_conv.hip.inc')).read()
    bact = open(os.path.join(CSRC, 'bias_act.hip.inc')).read()
    snorm = open(os.path.join(CSRC, 'spectral_norm.hip.inc')).read()
    ups = open(os.path.join(CSRC, 'upsample.hip.inc')).read()

    def body(name):
        start = capi.index('\nint %s(' % name)
        return capi[start:capi.index('\n}\n', start)]

    # grid_for(work, cap): workgroups of 256 threads over the work items, at most cap
    assert re.search(r'int grid_for\(long long work, int cap\) \{\s+const long long blocks = \(work \+ 255\) / 256;\s+'
                     r'return \(int\)\(blocks < cap \? blocks : cap\);\s+\}', helpers)

    def cap_of(name, count='work'):
        m = re.findall(r'const int blocks = grid_for\(%s, (\d+)\);' % count, body(name))
        assert len(m) == 1, name
        assert 'dim3(256)' in body(name)
        return int(m[0])

    caps = tc.BLOCK_CAPS
    assert cap_of('tai_conv_cin1_forward') == caps['cin1'] and cap_of('tai_conv_cin1_forward_maxpool_window') == caps['cin1_pool']
    assert cap_of('tai_conv_cout1_3x3_forward') == caps['cout1_3x3'] and cap_of('tai_conv_cout1_5x5_forward') == caps['cout1_5x5']
    assert cap_of('tai_bias_act_inplace') == caps['bias_act_vec4'] == caps['bias_act_scalar']
    assert cap_of('tai_unpool2x_add') == caps['unpool'] and cap_of('tai_conv_shift_stack') == caps['shift_stack']
    assert cap_of('tai_convlstm_gates_forward') == cap_of('tai_convlstm_gates_backward') == caps['convlstm']
    assert cap_of('tai_act_maxpool2x2_forward') == cap_of('tai_act_maxpool2x2_backward') == caps['act_pool']
    assert cap_of('tai_window_scale_bias_lrelu', 'n4') == cap_of('tai_window_scale_lrelu_backward', 'n4') == caps['window_scale']
    for name in ('tai_window_scale_bias_lrelu_scalar', 'tai_window_scale_lrelu_backward_scalar'):
        assert 'const int blocks = planes < %d ? planes : %d;' % ((caps['window_scale_scalar'],) * 2) in body(name)
    up = body('tai_upsample_bilinear2x_forward')
    assert 'const int per_plane = H * (2 * W / 4);' in up
    assert 'const int bx = grid_for(per_plane, %d);' % tc.UPS_XBLOCKS in up
    assert 'if ((2 * W) % 4 == 0 && H >= 2 && W >= 2 &&' in up
    assert 'for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < per_plane; t += gridDim.x * blockDim.x) {' in ups
    # the work counts
    assert 'const long long work = (long long)N * H * (W / 4);' in body('tai_conv_cin1_forward')
    assert 'const long long work = (long long)N * (H / 2) * (W / 4);' in body('tai_conv_cin1_forward_maxpool_window')
    assert 'const long long work = planes * (H / 2) * (W / 4);' in body('tai_act_maxpool2x2_forward')
    assert 'const long long work = planes * 2 * h * (2 * w / 4);' in body('tai_unpool2x_add')
    assert 'const long long work = (long long)N * F * (HW / 4);' in body('tai_convlstm_gates_forward')
    assert 'const long long work = (long long)N * S * S * C * (H + 2) * ((W + 4) / 4);' in body('tai_conv_shift_stack')
    assert 'const bool vec = (HW % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);' in body('tai_bias_act_inplace')
    assert 'const long long work = vec ? n / 4 : n;' in body('tai_bias_act_inplace')
    # the channel split, in both launchers and both kernels
    rule = 'const int cgroups = (work < 4 * 262144 && Co >= %d) ? %d : 1;' % (tc.CGROUP_MIN_CO, tc.CGROUPS)
    assert capi.count(rule) == 2 and tc.CGROUP_MAX_WORK == 4 * 262144
    assert thin.count('const int cg = (Co + gridDim.y - 1) / gridDim.y, co_end = min(Co, (int)(blockIdx.y + 1) * cg);') == 2
    # thin_wrw's segments
    assert 'const int nsub = max(1, %d / qw), rs = (H + nsub - 1) / nsub;' % tc.WRW_LANES in thin
    assert 'for (int item = threadIdx.x; item < qw * nsub; item += %d) {' % tc.THREADS in thin
    assert 'const int q = item % qw, sub = item / qw;' in thin and 'y0 = sub * rs, y1 = min(H, y0 + rs);' in thin
    # every kernel here is a 256-thread kernel whose loop strides by the whole grid
    assert thin.count('__launch_bounds__(256)') == 7 and bact.count('__launch_bounds__(256)') == 7
    assert thin.count('idx += (long long)gridDim.x * blockDim.x') == 5
    assert bact.count('+= (long long)gridDim.x * blockDim.x') == 7
    assert snorm.count('i += (long long)gridDim.x * 256') == 2 and snorm.count('for (int p = blockIdx.x; p < planes; p += gridDim.x) {') == 2
    assert 'const bool own_l = hasl && lane == 0, own_r = hasr && lane == 63;' in thin and tc.WAVE == 64
    assert 'const bool hasl = x0 >= 2, hasr = x0 + 6 <= W;' in thin
