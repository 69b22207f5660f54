"""Conditions of the case generator in tests/wino_cases.py, without a GPU.

tests/test_gpu_wino_kernels.py claims, per case, which Winograd kernel instance and which branches inside it a launch takes, compares
the integer cases with torch.equal and the F(4x4, 3x3) cases under a bound taken against the tile's magnitude.  Here:
  * the Python restatements of the launchers' plans equal the library's own answers -- tai_conv3x3_wino_forward_plan,
    tai_conv3x3_wino_wrw_plan (the functions the launchers call) and tai_conv3x3_wino43_splits -- on every case and on sweeps of 2,000
    shapes each, refusals included, and their constants are read back from the sources;
  * every flag a case claims holds, and the cases together reach every kernel instance the launchers can select and every flag
    (wino_cases.IMPOSSIBLE lists what no case can reach, with the enumeration that proves it);
  * every integer case keeps every stage of the F(2x2, 3x3) algorithm on absolute values below 2^24 quanta, its float64 reference is
    made of integers (quarters never occur: the weight gradient is an integer too), and the outliers sit where outlier_sites says;
  * on the F(4x4, 3x3) float cases an fp32 emulation of the algorithm passes the tile-magnitude bound and each injected defect fails it;
  * the queries refuse what the launchers refuse for the same arguments, with the same words (in a child process that sees no device:
    an accepted launcher call fails at its launch there instead of running on dummy pointers)."""
import ctypes
import json
import os
import random
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wino_cases as wc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'video-frame-inpainting_amd', 'csrc')
EINVAL = -1
NO_DEVICE = {'HIP_VISIBLE_DEVICES': '-1', 'ROCR_VISIBLE_DEVICES': '-1'}
UNTOUCHED = -7


def _lib():
    from video_frame_inpainting_amd import _native
    return _native.lib()


def lib_fwd_plan(L, N, C, K, H, W, nparts=1, shift_k=0, act=0, has_pool=False, has_addx=False, has_y2=False, window=None, U=None):
    out = (ctypes.c_int * 9)(*([UNTOUCHED] * 9))
    rc = L.tai_conv3x3_wino_forward_plan(nparts, shift_k, int(has_pool), int(has_addx), int(has_y2), N, C, K, H, W, *(window or (0, 0, 0, 0)), act, U, out)
    return rc, list(out)


def lib_wrw_plan(L, N, C, K, H, W, window=None, tile=4, paired=True):
    out = (ctypes.c_int * 8)(*([UNTOUCHED] * 8))
    L.tai_conv3x3_wino_wrw_set_tile(tile)
    L.tai_conv3x3_wino_wrw_set_paired(int(paired))
    try:
        rc = L.tai_conv3x3_wino_wrw_plan(N, C, K, H, W, *(window or (0, 0, 0, 0)), out)
    finally:
        L.tai_conv3x3_wino_wrw_set_tile(4)
        L.tai_conv3x3_wino_wrw_set_paired(1)
    return rc, list(out)


def _same_fwd(L, args, tall_on=True):
    N, C, K, H, W, nparts, shift_k, act, hp, ha, hy, window = args
    want = wc.fwd22_plan(N, C, K, H, W, nparts, shift_k, act, hp, ha, hy, window, False, tall_on)
    rc, out = lib_fwd_plan(L, N, C, K, H, W, nparts, shift_k, act, hp, ha, hy, window)
    if want is None:
        assert rc == EINVAL and out == [UNTOUCHED] * 9 and L.tai_sepconv_last_error(), (args, rc, out)
    else:
        assert rc == want['grid'] and out == [want[f] for f in wc.FWD_FIELDS], (args, want, rc, out, L.tai_sepconv_last_error())
    return want


def _same_wrw(L, N, C, K, H, W, window, tile, paired):
    want = wc.wrw_plan(N, C, K, H, W, window, tile, paired)
    rc, out = lib_wrw_plan(L, N, C, K, H, W, window, tile, paired)
    if want is None:
        assert rc == EINVAL and out == [UNTOUCHED] * 8 and L.tai_sepconv_last_error(), ((N, C, K, H, W, window, tile, paired), rc, out)
    else:
        assert rc == want['kblocks'] * want['cblocks'] * want['splits'] and out == [want[f] for f in wc.WRW_FIELDS], \
            ((N, C, K, H, W, window, tile, paired), want, rc, out)
    return want


def test_python_plans_equal_the_library_on_every_case():
    L = _lib()
    for c in wc.FWD22_CASES:            # (the split-arithmetic plans need a registered weight buffer: asserted per case on the GPU)
        p = _same_fwd(L, wc._fwd22_args(c)[:-1])
        assert p is not None, wc.fcase_id(c)
    for c in wc.WRW_CASES:
        p = _same_wrw(L, c.N, c.C, c.K, c.H, c.W, c.window, c.tile, c.paired)
        assert p is not None and p['tile'] == c.tile, wc.gcase_id(c)
    for c in wc.W43_CASES:
        if c.form == 'ws':
            cps = ctypes.c_int(UNTOUCHED)
            assert (L.tai_conv3x3_wino43_splits(c.N, c.C, c.K, c.H, c.W, c.nparts, ctypes.byref(cps)), cps.value) == \
                wc.w43_splits(c.N, c.C, c.K, c.H, c.W, c.nparts), wc.hcase_id(c)


def test_python_plans_equal_the_library_on_sweeps():
    """2,000 shapes each: the forward (parts, displaced reads, epilogues, windows, both tall settings; about a third are refusals), the
    weight gradient (both tiles, windows) and the split count of the F(4x4, 3x3) forward."""
    L = _lib()
    rnd = random.Random(0)
    seen = set()
    for _ in range(2000):
        N, H, W = rnd.randint(1, 40), rnd.randint(1, 40), rnd.randint(1, 40)
        if rnd.random() < 0.6:
            H, W = H + H % 2, W + W % 2
        nparts = rnd.choice((1, 1, 1, 2, 3, 4, 5))
        shift_k = rnd.choice((0, 0, 0, 3, 4, 5, 6, 7, 8, 9, 10)) if nparts == 1 else rnd.choice((0, 0, 0, 5))
        S = (shift_k + 2) // 3 if shift_k else 1
        C = rnd.choice((1, 3, 8, 12, 16, 24, 51, 64)) * (nparts if rnd.random() < 0.8 else 1) * (S * S if rnd.random() < 0.9 else 1)
        K = rnd.choice((1, 3, 51, 64, 70, 128, 130, 192, 256))
        act = rnd.choice((0, 1, 1, 2, 3)) if not shift_k else rnd.choice((1, 1, 1, 0))
        epi = rnd.choice(('plain', 'plain', 'pool', 'unpool', 'unpool_sum', 'y2_alone'))
        if epi.startswith('unpool') and rnd.random() < 0.8:
            act = 0
        window = None
        if shift_k and rnd.random() < 0.9:
            window = wc.halo_geometry(H, W, shift_k)[3:] + (1, 2)
            if rnd.random() < 0.15:
                window = (window[0] - rnd.randint(0, 1), window[1] - rnd.randint(0, 2), rnd.randint(0, 1), rnd.choice((0, 2)))
        elif rnd.random() < 0.3:
            oy, ox = rnd.randint(0, 3), rnd.randint(0, 4)
            window = (H + oy + rnd.randint(-1, 2), W + ox + rnd.randint(-1, 3), oy, ox)
        tall_on = rnd.random() < 0.8
        L.tai_conv3x3_wino_set_tall(int(tall_on))
        try:
            p = _same_fwd(L, (N, C, K, H, W, nparts, shift_k, act, epi == 'pool', epi in ('unpool', 'unpool_sum'), epi in ('unpool', 'y2_alone'), window),
                          tall_on)
        finally:
            L.tai_conv3x3_wino_set_tall(1)
        seen.add('refused' if p is None else ('fwd', p['tall'], p['parts'], p['epi']))
    assert 'refused' in seen and {('fwd', t, q, e) for t in (0, 1) for q in (0, 1) for e in (0, 1, 2, 3)} | {('fwd', t, 2, 0) for t in (0, 1)} <= seen
    seen = set()
    for _ in range(2000):
        N, C, K = rnd.randint(0, 48), rnd.choice((1, 8, 32, 33, 64, 70, 200)), rnd.choice((1, 8, 64, 65, 130, 200))
        H, W = rnd.choice((1, 2, 4, 5, 6, 8, 12, 32, 64)), rnd.choice((1, 4, 10, 12, 16, 20, 32, 48, 64, 128))
        window = None
        if rnd.random() < 0.3:
            oy, ox = rnd.randint(-1, 3), rnd.randint(-1, 4)
            window = (H + oy + rnd.randint(-1, 2), W + ox + rnd.randint(-1, 3), oy, ox)
            if window[0] <= 0:
                window = None
        tile, paired = rnd.choice((2, 4, 4)), rnd.random() < 0.7
        p = _same_wrw(L, N, C, K, H, W, window, tile, paired)
        seen.add('refused' if p is None else (p['tile'], p['paired'], p['ragged'], p['splits'] > 1, p['nchunks'] % p['chunks_per_split'] != 0))
    assert 'refused' in seen and {t[:3] for t in seen if t != 'refused'} == {(4, 0, 0), (2, 1, 0), (2, 0, 0), (2, 0, 1)}
    assert any(t != 'refused' and t[0] == tile and t[3] and t[4] for t in seen for tile in (2, 4))
    seen = set()
    for _ in range(2000):
        nparts = rnd.choice((1, 1, 2, 3, 4))
        N, C, K = rnd.randint(1, 16), rnd.choice((4, 51, 64, 70, 74, 128, 256, 512)) * rnd.choice((1, nparts)), rnd.choice((5, 64, 70, 128, 256))
        H, W = rnd.choice((4, 8, 12, 16, 32, 6)), rnd.choice((4, 8, 12, 16, 32))
        cps = ctypes.c_int(UNTOUCHED)
        got = (L.tai_conv3x3_wino43_splits(N, C, K, H, W, nparts, ctypes.byref(cps)), cps.value)
        assert got == wc.w43_splits(N, C, K, H, W, nparts), ((N, C, K, H, W, nparts), got)
        seen.add((got[0] > 1, nparts > 1))
    assert seen == {(a, b) for a in (False, True) for b in (False, True)}


def test_every_claimed_flag_holds():
    for c in wc.FWD22_CASES:
        f = wc.fwd22_flags(c)
        assert set(c.claims) <= set(wc.FWD22_FLAGS) and all(f[n] for n in c.claims), (wc.fcase_id(c), [n for n in c.claims if not f[n]])
        assert (c.act == 'tanh') <= (c.data == 'float')             # integers saturate tanh: it runs float data
        assert c.N * c.K * c.H * c.W <= 1 << 21
    for c in wc.WRW_CASES:
        f = wc.wrw_flags(c)
        assert set(c.claims) <= set(wc.WRW_FLAGS) and all(f[n] for n in c.claims), (wc.gcase_id(c), [n for n in c.claims if not f[n]])
        assert f['tile'] == c.tile and c.N * c.K * c.H * c.W <= 1 << 21 and c.N * c.C * c.H * c.W <= 1 << 21
    for c in wc.W43_CASES:
        f = wc.w43_flags(c)
        assert set(c.claims) <= set(wc.W43_FLAGS) and all(f[n] for n in c.claims), (wc.hcase_id(c), [n for n in c.claims if not f[n]])
        assert c.N * c.K * c.H * c.W <= 1 << 21 and (f['splits'] > 1) == (c.form == 'ws')
    for cases, ident in ((wc.FWD22_CASES, wc.fcase_id), (wc.WRW_CASES, wc.gcase_id), (wc.W43_CASES, wc.hcase_id)):
        assert len({ident(c) for c in cases}) == len(cases)


def test_the_cases_cover_every_instance_and_every_flag():
    # ---- F(2x2, 3x3) forward and its split arithmetic
    flags = [(c, wc.fwd22_flags(c)) for c in wc.FWD22_CASES]
    fp32, split = wc.fwd22_all_instances()
    got = {wc.fwd22_instance(f) for _, f in flags}
    assert got == fp32 | split, sorted((fp32 | split) - got) + sorted(got - (fp32 | split))
    assert len(fp32) == 34 and len(split) == 20
    # (the exact comparison reaches every instance but the tanh ones)
    assert {wc.fwd22_instance(f) for c, f in flags if c.data == 'int'} == {i for i in fp32 | split if not (i[1] == 2 and (i[0] == 'fp32' or i[3] == 0))}
    for name in wc.FWD22_FLAGS:
        hit = [c for c, f in flags if f[name]]
        assert hit and (any(name in c.claims for c in hit) or name in ('ragged_k', 'multi_kblock', 'partial_last_block', 'block_straddles_images')), name
    for tall in (0, 1):                 # both workgroup shapes meet the seams
        for name in ('ragged_c', 'ragged_k', 'multi_kblock', 'block_straddles_images', 'partial_last_block', 'odd_h', 'odd_w', 'xcd_block', 'no_xcd_block'):
            assert any(f[name] and f['tall'] == tall and not f['split'] for _, f in flags), (tall, name)
        assert {f['shift_k'] for _, f in flags if f['tall'] == tall and f['parts'] == 2} == {4, 5, 6, 7, 8, 9}
        assert {f['nparts'] for _, f in flags if f['tall'] == tall and f['parts'] == 1} == {2, 3, 4}
    assert any(f['tall'] and c.K == 70 for c, f in flags)             # K = 70 pads to 128: the tall workgroups, not two ragged 64-blocks
    assert any(f['window_origin'] and c.window[2] % 2 == 1 for c, f in flags) and any(f['window_origin'] and c.window[2] % 2 == 0 for c, f in flags)
    assert any(f['split'] and c.epi == 'pool' for c, f in flags)
    # ---- weight gradient
    gflags = [(c, wc.wrw_flags(c)) for c in wc.WRW_CASES]
    for tile in (2, 4):
        for name in wc.WRW_FLAGS:
            hit = [c for c, f in gflags if f[name] and c.tile == tile]
            assert bool(hit) != ((('wrw%d' % tile), name) in wc.IMPOSSIBLE), (tile, name)
            assert not hit or any(name in c.claims for c in hit) or name in ('bias', 'ragged_k', 'ragged_c', 'one_chunk_per_split', 'one_block'), (tile, name)
    assert {c.window[2:] for c in wc.WRW_CASES if c.tile == 4 and c.window} == {(1, 2), (3, 4)}
    # ---- F(4x4, 3x3) forward
    hflags = [(c, wc.w43_flags(c)) for c in wc.W43_CASES]
    assert {(c.form, f['instance']) for c, f in hflags if c.form != 'blocks'} == {(form, i) for form in ('plain', 'ws') for i in range(7)}
    assert {(c.shift_k, f['instance']) for c, f in hflags if c.form == 'blocks'} == {(k, i) for k in (5, 7, 9) for i in range(4)}
    assert {f['placement'] for _, f in hflags} == {'order', 'one_kblock_per_xcd', 'kblocks_over_xcds', 'fallback'}
    on = {(c.N, c.C, c.K, c.H, c.W): f['placement'] for c, f in hflags if c.placement and c.form == 'plain'}
    off = {(c.N, c.C, c.K, c.H, c.W) for c, f in hflags if not c.placement}
    assert {on[s] for s in off} == {'one_kblock_per_xcd', 'kblocks_over_xcds', 'fallback'}        # each branch also under set_placement(0)
    for name in wc.W43_FLAGS:
        hit = [c for c, f in hflags if f[name]]
        assert hit and any(name in c.claims for c in hit), name
    assert any(f['ragged_c'] and c.nparts == 1 for c, f in hflags) and {c.nparts for c in wc.W43_CASES} >= {1, 2, 4}


def test_what_no_case_can_reach():
    """wino_cases.IMPOSSIBLE, by enumeration over the plans and from the sources."""
    assert set(wc.IMPOSSIBLE) == {('wrw2', 'xcd_placement'), ('wrw2', 'plain_placement'), ('wrw4', 'paired'), ('wrw4', 'plain'), ('wrw4', 'ragged_odd_h'),
                                  ('wrw4', 'ragged_w')}
    # the placement is an argument of conv3x3_wrw_gen alone: wino::wrw::conv3x3_wrw takes none
    src = open(os.path.join(CSRC, 'wino_wrw.hip.inc')).read()
    assert 'dispatch_order' not in src and 'dispatch_order' in open(os.path.join(CSRC, 'wino43_conv.hip.inc')).read()
    # every plan at tile 4 has H % 4 == 0 and W % 16 == 0 and reports neither pairs nor the ragged form
    L = _lib()
    for H in range(1, 34):
        for W in range(1, 70):
            for window in (None, (H + 2, W + 4, 1, 2)):
                p = _same_wrw(L, 2, 8, 8, H, W, window, 4, True)
                assert p['tile'] == (4 if H % 4 == 0 and W % 16 == 0 else 2)
                assert p['tile'] == 2 or (p['paired'], p['ragged']) == (0, 0)


def _const(src, name, env=None):
    return eval(re.search(r'constexpr int (?:[\w, =]*\b)?%s = ([^;,]+)[;,]' % name, src).group(1), {}, env or {})


def test_constants_are_the_sources():
    conv = open(os.path.join(CSRC, 'wino_conv.hip.inc')).read()
    assert 'constexpr int KC = %d;' % wc.KC in conv and 'constexpr int TM = %d, TN = %d;' % (wc.TM, wc.TN) in conv
    assert 'constexpr int TTM = %d, TTN = %d;' % (wc.TTM, wc.TTN) in conv
    assert 'int xcd_block(int bid, int n) { return (n % 8 == 0) ? (bid % 8) * (n / 8) + bid / 8 : bid; }' in conv
    wrw = open(os.path.join(CSRC, 'wino_wrw.hip.inc')).read()
    assert 'constexpr int CT = %d;' % wc.CT in wrw
    w43 = open(os.path.join(CSRC, 'wino43_conv.hip.inc')).read()
    assert 'constexpr int KC = %d;' % wc.W43_KC in w43 and 'constexpr int TM = %d, TN = %d;' % (wc.W43_TM, wc.W43_TN) in w43
    assert 'constexpr double PT_A = %s, PT_B = %s;' % tuple(float(p) for p in wc.W43_POINTS) in w43
    # the three placement branches, as restated in w43_placement / w43_block_of
    assert 'if (win.dispatch_order) {' in w43 and 'kb = xcd % kblocks;' in w43 and 'tb = (xcd / kblocks) * (tblocks / (8 / kblocks)) + slot;' in w43
    assert '} else if (nblk % 8 == 0 && kblocks <= 8 && 8 % kblocks == 0 && tblocks % (8 / kblocks) == 0) {' in w43
    assert '} else if (nblk % 8 == 0 && kblocks % 8 == 0) {' in w43 and 'kb = xcd * per + slot % per;' in w43
    capi43 = open(os.path.join(CSRC, 'capi_wino43.inc')).read()
    assert 'constexpr int W43_MIN_SPLIT_CHUNKS = %d, W43_MAX_SPLITS = %d;' % (wc.W43_MIN_SPLIT_CHUNKS, wc.W43_MAX_SPLITS) in capi43
    assert 'if (ypool) return act == 0 ? 2 : 3;' in capi43 and 'if (addx) return y2 ? 5 : 6;' in capi43 and 'return act == 2 ? 4 : act;' in capi43
    table = re.search(r'static const W43Kernel plain\[W43_INSTANCES\] = \{([^}]*)\}', capi43).group(1)
    assert [tuple(int(v) for v in m) for m in re.findall(r'conv3x3_gen<(\d), (\d)>', table)] == list(wc.W43_INSTANCES)
    # the queries and the launchers call the same functions, and the queries' order of out[] is FWD_FIELDS / WRW_FIELDS
    capi = open(os.path.join(CSRC, 'capi_wino.inc')).read()
    assert len(re.findall(r'\bwino_forward_plan\(', capi)) == 3 and len(re.findall(r'\bwrw_route\(', capi)) == 3        # definition + two calls
    assert len(re.findall(r'\bwino_ex_arguments\(', capi)) == 3
    order = re.search(r'const int v\[9\] = \{([^}]*)\}', capi).group(1)
    assert [s.strip().replace('(int)', '').replace('p.', '').replace('pmode', 'parts') for s in order.split(',')] == list(wc.FWD_FIELDS)
    order = re.search(r'const int v\[8\] = \{([^}]*)\}', capi).group(1)
    assert [s.strip().replace('r.p.', '').replace('r.', '').replace('pair', 'paired') for s in order.split(',')] == list(wc.WRW_FIELDS)
    for t in range(1, 300):             # w43_block_of is a bijection under every branch
        for kblocks in (1, 2, 3, 4, 8, 16):
            for placement in (0, 1):
                nblk = t * kblocks
                if nblk <= 512:
                    assert sorted(wc.w43_block_of(b, nblk, kblocks, placement) for b in range(nblk)) == [(tb, kb) for tb in range(t) for kb in range(kblocks)]


INT_FWD = [c for c in wc.FWD22_CASES if c.data == 'int']


@pytest.mark.parametrize('c', INT_FWD, ids=wc.fcase_id)
def test_integer_forward_cases_are_exact_in_any_order(c):
    x, w, b, addx = wc.fwd22_data(c)
    plain = wc.fwd22_data(c, outliers=False)[0]
    assert float(plain.abs().max()) <= 4 and set(w.abs().unique().tolist()) <= {4., 8.} and float(b.abs().max()) <= 8
    assert addx is None or float(addx.abs().max()) <= 8
    w3 = wc.block3x3_weight(w) if c.shift_k else w
    src = wc.fwd22_patch_source(c, x)
    stages = wc.wino22_abs_terms(src, w3, b, addx)
    assert all(v == round(v) and v < wc.CAP for v in stages.values()), stages
    ref = wc.conv_reference(x, w, b, c.H, c.W, None if c.shift_k else c.window, c.act, addx)
    for name in ('y', 'pool', 'sum'):
        t = ref.get(name)
        if t is not None:
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= stages['Y'] and torch.equal(t.float().double(), t), name
    assert float(ref['y'].abs().max()) > wc.OUTLIER                 # the outliers reach the output
    # the 3 x 3 convolution the kernel is handed (blocked weight over displaced copies; the window in its frame) is that convolution
    direct = wc.activate(torch.nn.functional.conv2d(src[:, :, :c.H + 2, :c.W + 2].double(), w3.double(), b.double()), c.act)
    assert torch.equal(direct, ref['y'])


@pytest.mark.parametrize('c', wc.WRW_CASES, ids=wc.gcase_id)
def test_integer_weight_gradient_cases_are_exact_in_any_order(c):
    x, dy = wc.wrw_data(c)
    stages = wc.wino22_wrw_abs_terms(x, dy, c.H, c.W, c.window)
    assert all(v == round(v) and v < wc.CAP for v in stages.values()), stages
    dw, db = wc.wrw_reference(x, dy, c.H, c.W, c.window)
    assert torch.equal(dw, dw.round()) and torch.equal(db, db.round()) and float(dw.abs().max()) > wc.OUTLIER
    assert 4 * float(dw.abs().max()) <= stages['dw'] and float(db.abs().max()) <= stages['db']
    # ... and it is autograd's weight gradient of the convolution over the window in its frame
    oy, ox = c.window[2:] if c.window else (0, 0)
    xp = torch.nn.functional.pad(x.double(), (1, 1, 1, 1))[:, :, oy:oy + c.H + 2, ox:ox + c.W + 2]
    w = torch.zeros(c.K, c.C, 3, 3, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(xp, w).backward(dy.double())
    assert torch.equal(w.grad, dw)


def _check_sites(x, sites, N, C, H, W, tile, wtn, nparts, th=None, tw=None):
    assert len({(n, r, col) for n, _, r, col in sites}) == len(sites)
    assert int((x.abs() == wc.OUTLIER).sum()) == len(sites) and all(abs(float(x[s])) == wc.OUTLIER for s in sites)
    assert int((x == wc.OUTLIER).sum()) > 0 and (int((x == -wc.OUTLIER).sum()) > 0 or len(sites) == 1)
    th, tw = th or -(-H // tile), tw or -(-W // tile)
    tiles_hit = {(n * th + r // tile) * tw + col // tile for n, _, r, col in sites}
    total = N * th * tw
    real = lambda t: tile * (t % tw) < W                                 # (a tile of the extended grid past the plane holds no pixel)
    for b in range(1, -(-total // wtn)):                                  # both sides of the first and the last block seam
        if b in (1, -(-total // wtn) - 1):
            assert {t for t in (b * wtn - 1, b * wtn) if real(t)} <= tiles_hit, b
    assert {0, total - 1} & tiles_hit == {t for t in (0, total - 1) if real(t)}
    where = {(n, r, col) for n, _, r, col in sites}
    assert {(n, r, col) for n in (0, N - 1) for r in (0, H - 1) for col in (0, W - 1)} <= where              # plane corners
    chans = wc.seam_channels(C, nparts)
    used = {ch for _, ch, _, _ in sites}
    assert used <= set(chans) and (used == set(chans) or len(sites) < len(chans))


@pytest.mark.parametrize('c', INT_FWD, ids=wc.fcase_id)
def test_forward_outliers_sit_on_the_seams(c):
    x = wc.fwd22_data(c)[0]
    oy, ox = (c.window[2], c.window[3]) if c.window else (0, 0)
    inner = x[:, :, oy:oy + c.H, ox:ox + c.W]
    assert int((x.abs() == wc.OUTLIER).sum()) == int((inner.abs() == wc.OUTLIER).sum())
    f = wc.fwd22_flags(c)
    _check_sites(inner, wc.fwd22_sites(c), c.N, c.C, c.H, c.W, 2, wc.TTN if f['tall'] else wc.TN, c.nparts)


@pytest.mark.parametrize('c', wc.WRW_CASES, ids=wc.gcase_id)
def test_weight_gradient_outliers_sit_on_the_seams_and_split_boundaries(c):
    x = wc.wrw_data(c)[0]
    oy, ox = (c.window[2], c.window[3]) if c.window else (0, 0)
    inner = x[:, :, oy:oy + c.H, ox:ox + c.W]
    p = wc.wrw_plan(c.N, c.C, c.K, c.H, c.W, c.window, c.tile, c.paired)
    per_chunk = 4 if c.tile == 4 else wc.CT
    tw = c.W // 4 if c.tile == 4 else -(-c.W // 16) * 16 // 2
    _check_sites(inner, wc.wrw_sites(c), c.N, c.C, c.H, c.W, c.tile, per_chunk * p['chunks_per_split'], 1, tw=tw)


FLOAT43 = sorted({(c.N, c.C, c.K, c.H, c.W, c.nparts) for c in wc.W43_CASES if c.form != 'blocks'})


@pytest.mark.parametrize('shape', FLOAT43, ids=lambda s: 'x'.join(str(v) for v in s))
def test_the_tile_bound_passes_the_algorithm_and_fails_every_defect(shape):
    """wino43_emulated (fp32) against float64 under TOL43 of 1 + the tile's largest magnitude sum: clean passes, every defect that the
    shape can show fails it by two orders of magnitude at the least.  Every shape of the plain and split-over-channels cases; the six
    displaced-read (blocks) cases are left out: wino43_emulated is the 3 x 3 algorithm on a zero-padded tensor, and a k x k filter cut
    into 3 x 3 blocks over displaced windows of a halo-carrying plane is the same algorithm on S * S * C channels with no padding of its
    own -- the defects it could show are the plain form's."""
    N, C, K, H, W, nparts = shape
    c = wc.HCase(N, C, K, H, W, nparts, None, 'plain', 'plain', 0, 1, ())
    x, w, b, _ = wc.w43_data(c)
    ref = wc.conv_reference(x, w, b, H, W)
    clean = wc.tile_ratio(wc.wino43_emulated(x, w, b), ref['y'], ref['mag'])
    print('%s: clean emulation %.3g of the tile magnitude' % (shape, clean))
    assert clean <= wc.TOL43, clean
    assert len(wc.w43_sites(c)) == int((x.abs() == wc.OUTLIER).sum()) > 0
    tiles = N * (H // 4) * (W // 4)
    for defect in wc.DEFECTS:
        if (defect == 'swap_images_at_seam' and N == 1) or (defect == 'skip_last_tile_of_block' and tiles < wc.W43_TN) \
                or (defect == 'row_end_reads_next_tile' and H * W <= 16):
            continue
        bad = wc.tile_ratio(wc.wino43_emulated(x, w, b, defect), ref['y'], ref['mag'])
        assert bad > 100 * wc.TOL43, (defect, bad)


# ---- the queries refuse what the launchers refuse ------------------------------------------------------------------------------------

P = 16          # a pointer that is never followed
# (nparts, shift_k, has_pool, has_addx, has_y2, N, C, K, H, W, in_h, in_w, in_oy, in_ox, act)
FWD_REFUSED = [(5, 0, 0, 0, 0, 1, 8, 8, 8, 8, 0, 0, 0, 0, 0), (2, 5, 0, 0, 0, 1, 8, 8, 8, 8, 0, 0, 0, 0, 0), (1, 3, 0, 0, 0, 1, 8, 8, 8, 8, 0, 0, 0, 0, 0),
               (1, 10, 0, 0, 0, 1, 8, 8, 8, 8, 0, 0, 0, 0, 0), (2, 0, 0, 0, 0, 1, 24, 8, 8, 8, 0, 0, 0, 0, 0), (1, 5, 0, 0, 0, 1, 12, 8, 8, 8, 0, 0, 0, 0, 0),
               (1, 0, 0, 0, 1, 1, 8, 8, 8, 8, 0, 0, 0, 0, 0), (1, 5, 0, 0, 0, 1, 32, 8, 8, 8, 16, 16, 0, 2, 1), (1, 5, 0, 0, 0, 1, 32, 8, 8, 8, 12, 16, 1, 2, 1),
               (1, 5, 0, 0, 0, 1, 32, 8, 8, 8, 16, 16, 1, 2, 0), (1, 0, 0, 1, 0, 1, 8, 8, 8, 8, 0, 0, 0, 0, 1), (1, 0, 1, 0, 0, 1 << 10, 8, 1 << 10, 1 << 6, 1 << 6, 0, 0, 0, 0, 0),
               (1, 0, 0, 1, 0, 1, 8, 8, 7, 8, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 1, 8, 8, 8, 8, 8, 9, 0, 0, 0), (1, 0, 0, 0, 0, 0, 8, 8, 8, 8, 0, 0, 0, 0, 0),
               (1, 0, 0, 0, 0, 1, 8, 8, 8, 8, 0, 0, 0, 0, 3), (1, 0, 0, 0, 0, 128, 8, 64, 256, 256, 0, 0, 0, 0, 0), (1, 0, 1, 0, 0, 1, 8, 8, 7, 7, 0, 0, 0, 0, 0),
               (1, 9, 0, 0, 0, 1, 72, 8, 8, 8, 16, 18, 1, 2, 2), (1, 0, 0, 0, 0, 1, 8, 8, 8, 8, 10, 10, 1, 1, 0)]
FWD_ACCEPTED = [(1, 0, 0, 0, 0, 1, 8, 3, 2, 2, 0, 0, 0, 0, 0), (3, 0, 0, 0, 0, 3, 72, 64, 7, 9, 0, 0, 0, 0, 2), (1, 9, 1, 0, 0, 2, 72, 128, 4, 4, 12, 14, 1, 2, 1),
                (1, 0, 0, 1, 1, 2, 8, 70, 8, 8, 10, 12, 1, 2, 0), (1, 5, 0, 0, 0, 1, 32, 8, 8, 8, 13, 16, 1, 2, 1)]
# (N, C, K, H, W, in_h, in_w, in_oy, in_ox); in_h = 0: tai_conv3x3_wino_wrw, else tai_conv3x3_wino_wrw_window
WRW_REFUSED = [(0, 8, 8, 8, 16, 0, 0, 0, 0), (1 << 10, 64, 64, 128, 128, 0, 0, 0, 0), (1, 8, 8, 8, 16, 8, 16, 1, 0), (1, 8, 8, 8, 16, 10, 18, -1, 0),
               (1, 8, 0, 8, 16, 0, 0, 0, 0), (1, 8, 8, 8, 16, 8, 15, 0, 0), (1, 8, 8, 8, 16, 8, 0, 0, 0), (1, 8, 8, 8, 16, 8, -1, 0, 0)]
WRW_ACCEPTED = [(1, 8, 8, 8, 16, 0, 0, 0, 0), (2, 70, 130, 5, 20, 0, 0, 0, 0), (2, 16, 24, 8, 16, 14, 24, 3, 4), (2, 16, 24, 5, 10, 7, 14, 1, 2)]


def _answers(L):
    xs = (ctypes.c_void_p * 4)(P, P, P, P)
    rows = []
    for a in FWD_REFUSED + FWD_ACCEPTED:
        nparts, shift_k, hp, ha, hy = a[:5]
        out = (ctypes.c_int * 9)(*([UNTOUCHED] * 9))
        q = [L.tai_conv3x3_wino_forward_plan(*a, None, out), L.tai_sepconv_last_error().decode(), list(out)]
        launch = [L.tai_conv3x3_wino_forward_ex(xs, nparts, shift_k, P, P, P, P if hp else None, 0, 0, 0, 0, P if ha else None, P if hy else None, *a[5:], None),
                  L.tai_sepconv_last_error().decode()]
        rows.append([q, launch])
    for a in WRW_REFUSED + WRW_ACCEPTED:
        out = (ctypes.c_int * 8)(*([UNTOUCHED] * 8))
        q = [L.tai_conv3x3_wino_wrw_plan(*a, out), L.tai_sepconv_last_error().decode(), list(out)]
        if a[5] == 0:
            launch = [L.tai_conv3x3_wino_wrw(P, P, P, P, P, *a[:5], None), L.tai_sepconv_last_error().decode()]
        else:
            launch = [L.tai_conv3x3_wino_wrw_window(P, P, P, P, P, *a, None), L.tai_sepconv_last_error().decode()]
        rows.append([q, launch])
    return rows


def test_the_queries_refuse_what_the_launchers_refuse():
    from video_frame_inpainting_amd import _native
    _native.verify(_native.LIB_PATH)
    run = subprocess.run([sys.executable, os.path.abspath(__file__), '--answers', _native.LIB_PATH], env=dict(os.environ, **NO_DEVICE),
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = json.loads(run.stdout)
    nf, na = len(FWD_REFUSED), len(FWD_ACCEPTED)
    assert len(rows) == nf + na + len(WRW_REFUSED) + len(WRW_ACCEPTED)
    said = set()
    for args, (q, launch) in zip(FWD_REFUSED, rows):
        assert q[0] == EINVAL and launch[0] == EINVAL and q[1] == launch[1] and q[1].startswith('conv3x3_wino'), (args, q, launch)
        assert q[2] == [UNTOUCHED] * 9, args
        assert wc.fwd22_plan(*args[5:10], args[0], args[1], args[14], bool(args[2]), bool(args[3]), bool(args[4]), args[10:14]) is None, args
        said.add(q[1])
    # every refusal of wino_ex_arguments and wino_forward_plan that needs no registered buffer, timeline stamps or pooled window
    capi = open(os.path.join(CSRC, 'capi_wino.inc')).read()
    body = capi[capi.index('static int wino_forward_plan('):capi.index('// The plan of a launch as a query')] + \
        capi[capi.index('static int wino_ex_arguments('):capi.index('#ifdef TAI_TIMING_VARIANTS\nstatic long long* g_wino_ex_stamps')]
    words = {''.join(re.findall(r'"((?:[^"\\]|\\.)*)"', m)) for m in re.findall(r'fail\(TAI_SEPCONV_EINVAL, "%s",\s*((?:"(?:[^"\\]|\\.)*"\s*)+)\)', body)}
    assert words - said == {'conv3x3_wino: the split-bf16 arithmetic needs even H and W', 'conv3x3_wino: bad pooled-output window'}, words - said
    for args, (q, launch) in zip(FWD_ACCEPTED, rows[nf:nf + na]):
        want = wc.fwd22_plan(*args[5:10], args[0], args[1], args[14], bool(args[2]), bool(args[3]), bool(args[4]), args[10:14])
        assert q[0] == want['grid'] > 0 and q[1] == '' and q[2] == [want[f] for f in wc.FWD_FIELDS] and launch[0] != EINVAL, (args, q, launch)
    for args, (q, launch) in zip(WRW_REFUSED, rows[nf + na:]):
        assert q[0] == EINVAL and launch[0] == EINVAL and q[1] == launch[1], (args, q, launch)
        assert q[1].startswith('conv3x3_wino_wrw: ') or (q[1] == 'conv3x3_wino_wrw_window: bad plane' and args[5] > 0 >= args[6]), (args, q)
        assert q[2] == [UNTOUCHED] * 8, args
    for args, (q, launch) in zip(WRW_ACCEPTED, rows[nf + na + len(WRW_REFUSED):]):
        want = wc.wrw_plan(*args[:5], args[5:] if args[5] else None)
        assert q[0] > 0 and q[1] == '' and q[2] == [want[f] for f in wc.WRW_FIELDS] and launch[0] != EINVAL, (args, q, launch)
    L = _lib()
    assert L.tai_conv3x3_wino_forward_plan(*FWD_ACCEPTED[0], None, None) == EINVAL and L.tai_sepconv_last_error() == b'null pointer'
    assert L.tai_conv3x3_wino_wrw_plan(*WRW_ACCEPTED[0], None) == EINVAL and L.tai_sepconv_last_error() == b'null pointer'


if __name__ == '__main__':
    if sys.argv[1:2] == ['--answers'] and len(sys.argv) == 3:
        assert all(os.environ.get(k) == v for k, v in NO_DEVICE.items())
        import importlib
        _native = importlib.import_module('video-frame-inpainting_amd._native')
        L = ctypes.CDLL(sys.argv[2])
        for name, (restype, argtypes) in _native.signatures().items():
            entry = getattr(L, name)
            entry.restype, entry.argtypes = restype, argtypes
        print(json.dumps(_answers(L)))
        sys.exit(0)
    sys.exit(__doc__)
