"""Conditions of the case generators in tests/sepconv_cases.py, without a GPU.

The GPU module compares integer-exact cases with torch.equal.  That is sound only if every partial sum of every gradient is
an integer below 2^24 -- a cap, asserted here per shape on the ABSOLUTE values of the operands (which bounds every partial sum
of any summation order and any sign pattern), together with "the fp32 oracle equals the fp64 oracle bit for bit"."""
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
    capi = open(os.path.join(CSRC, 'sepconv_capi.hip')).read()
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
