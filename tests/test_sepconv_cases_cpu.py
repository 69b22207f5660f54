"""Conditions of the case generators in tests/sepconv_cases.py, without a GPU.

The GPU module compares integer-exact cases with torch.equal.  That is sound only if every partial sum of every gradient is
an integer below 2^24 -- a cap, asserted here per shape on the ABSOLUTE values of the operands (which bounds every partial sum
of any summation order and any sign pattern), together with "the fp32 oracle equals the fp64 oracle bit for bit".  The same for the
forward's cases (tests/test_gpu_sepconv_forward.py), whose persistent-kernel shapes depend on the device's CU count: checked here
for the MI355X's 256, together with the route predicates that say which kernel each of those shapes reaches."""
import os
import re

import numpy as np
import pytest

import sepconv_cases as sc
from oracle import sepconv_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'video-frame-inpainting_amd', 'csrc')


def _np(ts):
    return [t.numpy() for t in ts]


@pytest.mark.parametrize('shape', sorted(set(sc.ALL_SHAPES)), ids=sc.shape_id)
def test_integer_cases_stay_below_2_to_24_and_fp32_equals_fp64(shape):
    B, C, H, W, ks = shape
    inp, v, h, gO = sc.int_case(B, C, H, W, ks, seed=1)
    for t in (inp, v, h, gO):
        assert bool((t == t.round()).all())
    a_inp, a_v, a_h, a_gO = _np(t.abs() for t in (inp, v, h, gO))
    cap32 = so.backward(a_gO, a_inp, a_v, a_h, ks)
    cap64 = so.backward(a_gO, a_inp, a_v, a_h, ks, f64=True)
    for g32, g64 in zip(cap32, cap64):
        assert float(g32.max()) < sc.CAP and float(g64.max()) < sc.CAP
        assert np.array_equal(g32, g64)
    # the signed case itself: exact in fp32, integers throughout
    inp, v, h, gO = _np((inp, v, h, gO))
    for g32, g64, bound in zip(so.backward(gO, inp, v, h, ks), so.backward(gO, inp, v, h, ks, f64=True), cap64):
        assert np.array_equal(g32, g64)
        assert np.array_equal(g64, np.round(g64))
        assert bool((np.abs(g64) <= bound).all())


@pytest.mark.parametrize('shape', sorted(set(sc.ALL_SHAPES)), ids=sc.shape_id)
def test_integer_case_ranges_and_outlier_sites(shape):
    B, C, H, W, ks = shape
    inp, v, h, gO = sc.int_case(B, C, H, W, ks, seed=2)
    plain = sc.int_case(B, C, H, W, ks, seed=2, outliers=False)
    assert float(plain[0].abs().max()) <= 4 and float(plain[3].abs().max()) <= 3
    assert float(v.abs().max()) <= 2 and float(h.abs().max()) <= 2
    g_sites, i_sites = sc.outlier_sites(B, C, H, W, ks)
    Hp, Wp = H + ks - 1, W + ks - 1
    assert {(r, c) for _, _, r, c in g_sites} >= {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
    assert {(r, c) for _, _, r, c in i_sites} >= {(0, 0), (Hp - 1, Wp - 1), (0, Wp - 1), (Hp - 1, 0)}
    if H > 8:
        assert {7, 8} <= {r for _, _, r, _ in g_sites}
    if H > 10:
        assert {9, 10} <= {r for _, _, r, _ in g_sites}
    if W > 128:
        assert {127, 128} <= {c for _, _, _, c in g_sites}
    for b, c, r, col in g_sites:
        assert abs(float(gO[b, c, r, col])) == sc.OUTLIER
        assert bool((v[b, :, r, col] != 0).all()) and bool((h[b, :, r, col] != 0).all())
    for b, c, r, col in i_sites:
        assert abs(float(inp[b, c, r, col])) == sc.OUTLIER
    assert int((gO.abs() == sc.OUTLIER).sum()) == len(g_sites) and int((inp.abs() == sc.OUTLIER).sum()) == len(i_sites)
    # and the generator is a function of its seed
    again = sc.int_case(B, C, H, W, ks, seed=2)
    assert all(bool((a == b).all()) for a, b in zip((inp, v, h, gO), again))


def test_tiling_constants_match_the_kernels():
    bwd = open(os.path.join(CSRC, 'sepconv_bwd.hip.inc')).read()
    fwd = open(os.path.join(CSRC, 'sepconv_fwd.hip.inc')).read()
    assert re.search(r'constexpr int TILE_W = (\d+);', fwd).group(1) == str(sc.TILE_W)
    gi2 = bwd[bwd.index('namespace gi2 {'):bwd.index('}  // namespace gi2')]
    const = lambda name: int(re.search(r'\b%s = (\d+)\b' % name, gi2).group(1))
    assert const('KS') == 51 and const('R') == sc.GI_R
    assert 'AROWS = R + KS - 1;' in gi2 and 'SLAB = AROWS * SPITCH;' in gi2
    assert (sc.GI_R + 51 - 1) * const('SPITCH') == sc.GI_SLAB == 10800
    assert 'constexpr int KS = 51, THREADS = 512, TILE_H = %d;' % sc.GV_TILE_H in bwd       # sepconv_grad_vh_ab
    assert 'ROWS_PER_WAVE = 2 / SPLIT;' in fwd and 'WAVES = SPLIT == 1 ? 4 : 8;' in fwd      # Cfg<KS, 1>::TILE_H = 2 * 4
    capi = open(os.path.join(CSRC, 'capi_sepconv.inc')).read()
    assert 'const bool tileable = (ks == 51) && (W % 4 == 0) && (C == 1 || C == 3);' in capi


def test_every_shape_reaches_the_branch_it_is_listed_for():
    assert all(sc.tileable(C, W, ks) for _, C, _, W, ks in sc.TILEABLE_SHAPES)
    assert not any(sc.tileable(C, W, ks) for _, C, _, W, ks in sc.GENERIC_SHAPES)
    assert all(C == 1 for _, C, _, _, _ in sc.AB_SHAPES) and all(C == 3 for _, C, _, _, _ in sc.C3_SHAPES)
    th, tw = sc.GV_TILE_H, sc.TILE_W
    ab = {s[2:4] for s in sc.AB_SHAPES}
    assert any(H % th == 0 and W % tw == 0 for H, W in ab)                              # exact tiles
    assert any(H < th and W < tw for H, W in ab)                                        # one tile, ragged both ways
    assert any(H % th == 1 and W % tw == 4 for H, W in ab)                              # a one-row tile, a one-quad tile
    assert any(H > 2 * th and W > 2 * tw and H % th and W % tw for H, W in ab)          # 3 x 3 tiles, ragged
    assert {H % sc.GI_R for H, _ in ab} >= {0, 1} and any(H > 2 * sc.GI_R for H, _ in ab)
    assert all(W > tw and W % tw == 4 and H % th for _, _, H, W, _ in sc.C3_SHAPES)
    # the slab boundary: one fit and one no-fit per channel count, each as close to the boundary as W % 4 == 0 allows
    fit = {s: sc.slabs_fit(*s) for s in sc.SLAB_SHAPES}
    assert [fit[s] for s in sc.SLAB_SHAPES] == [True, False, True, False, False]
    for (B, C, H, W, ks), ok in list(fit.items())[:4]:
        assert sc.slabs_fit(B, C, H, W + 4, ks) if not ok else not sc.slabs_fit(B, C, H, W - 4, ks)
    assert sc.slab_floats(1, 1, 2, 108) == 10800 <= 51 * 2 * 108 == 11016 and 51 * 2 * 104 == 10608
    assert sc.slab_floats(1, 3, 5, 128) == 32400 <= 51 * 5 * 128 == 32640 and 51 * 5 * 124 == 31620
    assert sc.slab_floats(1, 3, 11, 132) == 4 * 32400
    assert all(sc.slabs_fit(*s) for s in sc.REPEAT_SHAPES + sc.AB_SHAPES)
    assert not sc.slabs_fit(1, 3, 9, 132, 51) and sc.slabs_fit(1, 1, 9, 132, 51)       # 64,800 slab floats against 60,588
    # the generic routes: the gather's channel split, W % 4 != 0, other filter sizes
    gen = sc.GENERIC_SHAPES
    assert {C for _, C, _, _, ks in gen if ks == 51 and C > 3} == {4, 5}                  # 3 + 1 and 3 + 1 + 1
    assert any(W % 4 and ks == 51 and C == 1 for _, C, _, W, ks in gen) and {ks for *_, ks in gen} == {51, 7, 1}
    every = set(sc.ALL_SHAPES)
    assert set(sc.SUBSET_SHAPES) <= every and set(sc.BAND_SHAPES) <= every and set(sc.REPEAT_SHAPES) <= every
    assert len(set(sc.SUBSETS)) == 7 and (False, False, False) not in sc.SUBSETS


# ---- the forward's cases ------------------------------------------------------------------------------------------------

CUS = 256               # compute units of an MI355X: the device the derived batch sizes are checked for here
FWD_SHAPES = sorted(set(sc.fwd_all_shapes(CUS)))


@pytest.mark.parametrize('shape', FWD_SHAPES, ids=sc.shape_id)
def test_forward_integer_cases_stay_below_2_to_24_and_fp32_equals_fp64(shape):
    """The sum of the absolute terms of an output pixel bounds every partial sum of every order: rows first (type A: h folded
    into a row sum, rows folded with v) or 51 accumulators folded with h last (type B)."""
    B, C, H, W, ks = shape
    inp, v, h = sc.fwd_int_case(B, C, H, W, ks, seed=1)
    for t in (inp, v, h):
        assert bool((t == t.round()).all())
    cap = so.forward(*_np(t.abs() for t in (inp, v, h)), ks, f64=True)
    assert float(cap.max()) < sc.CAP, float(cap.max())
    o32, o64 = so.forward(*_np((inp, v, h)), ks), so.forward(*_np((inp, v, h)), ks, f64=True)
    assert np.array_equal(o32, o64)
    assert np.array_equal(o64, np.round(o64)) and bool((np.abs(o64) <= cap).all())


@pytest.mark.parametrize('shape', FWD_SHAPES, ids=sc.shape_id)
def test_forward_integer_case_ranges_and_outlier_sites(shape):
    B, C, H, W, ks = shape
    inp, v, h = sc.fwd_int_case(B, C, H, W, ks, seed=2)
    assert float(inp[inp.abs() != sc.OUTLIER].abs().max()) <= 4 and float(v.abs().max()) <= 2 and float(h.abs().max()) <= 2
    sites = sc.fwd_outlier_sites(B, C, H, W, ks)
    Hp, Wp = H + ks - 1, W + ks - 1
    rows, cols = {r for _, _, r, _ in sites}, {c for _, _, _, c in sites}
    assert {(r, c) for _, _, r, c in sites} >= {(0, 0), (0, Wp - 1), (Hp - 1, 0), (Hp - 1, Wp - 1)}
    assert rows >= {0, H - 1, Hp - 2, Hp - 1} and cols >= {0, W - 1, Wp - 2, Wp - 1}      # the two edge floats of the last column tile
    if Hp > sc.PATCH_ROWS:
        assert {15, 16, 65, 66} <= rows                                                 # the row-tile seam, the last patch row
    if Wp > 178:
        assert {127, 128, 177, 178} <= cols                                             # the column-tile seam, the last patch column
    assert len(set(sites)) == len(sites) and all(0 <= b < B and 0 <= c < C for b, c, _, _ in sites)
    for site in sites:
        b, c, r, col = site
        assert abs(float(inp[b, c, r, col])) == sc.OUTLIER
        # it is read, and by pixels whose taps -- all of them, so the two that multiply it too -- are never zero
        ys, xs = sc.fwd_readers(site, H, W, ks)
        assert v[b, :, ys, xs].numel() > 0 and bool((v[b, :, ys, xs] != 0).all()) and bool((h[b, :, ys, xs] != 0).all())
        y, x = ys.start, xs.start
        assert 0 <= r - y < ks and 0 <= col - x < ks and y < H and x < W
    assert int((inp.abs() == sc.OUTLIER).sum()) == len(sites)
    again = sc.fwd_int_case(B, C, H, W, ks, seed=2)
    assert all(bool((a == b).all()) for a, b in zip((inp, v, h), again))


def test_forward_shapes_reach_the_route_they_are_listed_for():
    # the persistent planes with their derived batch: persistent on the automatic route, three tiles for some workgroup
    assert sc.PERSISTENT_ROUNDS == 3
    for plane in sc.FWD_PERSISTENT_PLANES:
        B, C, H, W, ks = sc.fwd_persistent_shape(plane, CUS)
        assert C == 1 and ks == 51 and sc.fwd_tileable(W, ks)
        assert sc.fwd_persistent_runs(B, H, W, CUS) and sc.fwd_persistent_runs(B, H, W, CUS, forced=True)
        most, fewest = sc.fwd_rounds(B, H, W, CUS)
        assert most == 3 and fewest >= 2                       # both patch buffers are staged a second time, by every workgroup
        assert not any(sc.fwd_tiles(b, H, W) % 8 == 0 and sc.fwd_rounds(b, H, W, CUS)[0] >= 3 for b in range(1, B))
        fb = sc.fwd_fallback_shapes(plane, CUS)
        Br, Bf = fb['ragged'][0], fb['few'][0]
        assert sc.fwd_tiles(Br, H, W) % 8 != 0 and sc.fwd_tiles(Br, H, W) > CUS
        assert not sc.fwd_persistent_runs(Br, H, W, CUS) and not sc.fwd_persistent_runs(Br, H, W, CUS, forced=True)
        assert sc.fwd_tiles(Bf, H, W) % 8 == 0 and sc.fwd_tiles(Bf, H, W) <= CUS
        assert not sc.fwd_persistent_runs(Bf, H, W, CUS) and sc.fwd_persistent_runs(Bf, H, W, CUS, forced=True)
        assert sc.fwd_rounds(Bf, H, W, CUS) == (1, 1)
    assert [sc.fwd_persistent_shape(p, CUS)[0] for p in sc.FWD_PERSISTENT_PLANES] == [130, 64, 130, 260]
    planes = dict((p, (p[1] % sc.TILE_W, p[0] % sc.FWD_TILE_H)) for p in sc.FWD_PERSISTENT_PLANES)
    assert planes == {(20, 132): (4, 4), (40, 320): (64, 8), (26, 208): (80, 10), (17, 128): (0, 1)}
    # the shapes tests/test_gpu_sepconv.py asks variant 20 for have 12, 2, 3 and 2 tiles: none a multiple of 8, so none of them
    # runs the persistent kernel even when it is asked for by number -- which is why the planes above exist
    assert [sc.fwd_tiles(*s) for s in sc.MIXED_WAVE_SHAPES] == [12, 2, 3, 2]
    assert not any(sc.fwd_persistent_runs(B, H, W, CUS, forced=True) for B, H, W in sc.MIXED_WAVE_SHAPES)
    # the colour and the small shapes
    c3 = sc.FWD_C3_SHAPES
    assert all(sc.fwd_tileable(W, ks) for _, _, _, W, ks in c3)
    assert {C for _, C, _, _, _ in c3} == {2, 3, 4, 5, 6, 7}
    assert any(C == 3 and W > 2 * sc.TILE_W and H > 2 * sc.FWD_TILE_H and B > 1 for B, C, H, W, _ in c3)      # 3 x 3 tiles
    assert any(C == 3 and W > sc.TILE_W and W % sc.TILE_W == 4 and H % sc.FWD_TILE_H == 1 for _, C, H, W, _ in c3)
    assert any(C == 3 and W == 320 for _, C, _, W, _ in c3)
    small = sc.FWD_SMALL_SHAPES
    assert [sc.fwd_tileable(W, ks) for _, _, _, W, ks in small] == [True, True, True, False, False, False]
    assert any(H % sc.FWD_TILE_H_SMALL == 1 and H > sc.FWD_TILE_H_SMALL and W > sc.TILE_W for _, _, H, W, _ in small)
    assert any(H == 1 and W == 4 for _, _, H, W, _ in small) and {ks for *_, ks in small} == {51, 7, 1}
    assert sc.FWD_VARIANTS == tuple(range(28)) and sc.FWD_PERSISTENT_VARIANTS == tuple(range(20, 28))


def test_forward_constants_and_route_conditions_match_the_sources():
    fwd = open(os.path.join(CSRC, 'sepconv_fwd.hip.inc')).read()
    # the launchers: every host file of the translation unit, so that "no second copy" means none anywhere
    capi = ''.join(open(os.path.join(CSRC, f)).read() for f in ['sepconv_capi.hip'] + sorted(f for f in os.listdir(CSRC) if f.startswith('capi_')))
    assert 'int persistent_policy(' in open(os.path.join(CSRC, 'capi_sepconv.inc')).read()
    # the persistent kernel and the kernels it shares its row loops with
    pers = fwd[fwd.index('void sepconv_forward_persistent('):fwd.index('// ---- multi-channel frames (RGB)')]
    m = re.search(r'constexpr int KS = (\d+), WAVES = (\d+), TILE_H = (\d+);\s+constexpr int PR = TILE_H \+ KS - 1, PITCH = (\d+);', pers)
    assert [int(x) for x in m.groups()] == [51, 8, sc.FWD_TILE_H, sc.PATCH_PITCH]
    assert sc.PATCH_ROWS == sc.FWD_TILE_H + 51 - 1
    assert 'constexpr int TILE_H = 2 * WAVES;' in fwd and sc.FWD_TILE_H_SMALL == 2 * 4 and sc.FWD_TILE_H == 2 * 8
    dma = fwd[fwd.index('float2 stage_patch_dma('):fwd.index('// ---- type A + type B waves in one workgroup')]
    assert int(re.search(r'constexpr int CH = (\d+), SLOTS = PR \* CH', dma).group(1)) == sc.PATCH_CHUNKS
    assert sc.PATCH_CHUNKS * 4 == sc.PATCH_PITCH and 'edge_lds = lds_base + (unsigned)((er * %d + ec) * sizeof(float));' % sc.PATCH_PITCH in dma
    assert 'const int qmax = min((Wp - x0 - 4) >> 2, CH - 1);' in dma and 'ec = 4 * (qmax + 1);' in dma
    # the walk fwd_rounds restates
    assert 'const int per_xcd = ntiles >> 3, slots = gridDim.x >> 3;' in pers
    assert 'for (int r = 0; slot + r * slots < per_xcd; ++r) {' in pers and 'const int buf = r & 1;' in pers
    # the decision fwd_persistent_runs restates: one function in the launcher
    pol = capi[capi.index('int persistent_policy('):capi.index('template <int DBG = 0>\nint launch_persistent(')]
    assert 'tiles_x = (W + fwd::TILE_W - 1) / fwd::TILE_W, tiles_y = (H + %d) / %d;' % (sc.FWD_TILE_H - 1, sc.FWD_TILE_H) in pol
    assert 'const int ntiles = B * tiles_x * tiles_y;' in pol and 'const int grid = cus > 0 ? (cus / 8) * 8 : 0;' in pol
    cond = re.search(r'if \((C != 1 \|\| .*?)\)\n\s+return 0;', pol, re.S).group(1)
    assert [c.strip() for c in cond.split('||')] == ['C != 1', 'grid < 8', 'ntiles % 8 != 0', '(!force && ntiles <= grid)',
                                                     '(long long)B * 51 * H * W * 4 > 0xffffffffLL']
    assert 0xffffffff == 2 ** 32 - 1
    assert capi.count('ntiles % 8 != 0') == 1 and capi.count('ntiles <= grid') == 1        # no second copy of the conditions
    assert 'if (grid > ntiles) grid = ntiles;' in capi
    # both users go through forward_route
    assert len(re.findall(r'\bpersistent_policy\(', capi)) == 3          # its definition, forward_route, the stamped tools launch
    assert len(re.findall(r'\bforward_route\(B, C, H, W, ks, ', capi)) == 2
    assert 'const bool tileable = (ks == 51) && (W % 4 == 0);' in capi[capi.index('int forward_route('):capi.index('int fwd_asm_channel_loop')]
