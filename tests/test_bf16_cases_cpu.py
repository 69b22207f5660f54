"""Conditions of the case generator in tests/bf16_cases.py, without a GPU.

tests/test_gpu_conv_bf16_kernel.py claims, per case, which kernel instance and which routes inside it a launch takes, and compares
the integer cases with torch.equal.  Here:
  * the Python restatement of cbf16::plan equals the library's own answer (tai_conv_bf16_plan: the function the launcher calls) on
    every case and on a sweep of 2,000 shapes, and its constants are read back from the sources;
  * every flag a case claims holds, and the cases together reach, at each k, both MW values, every activation at MW = 4 and every
    flag (but those no shape can raise at that k: bf16_cases.IMPOSSIBLE, proved by enumeration);
  * every integer case keeps the sum of its absolute terms plus |bias| (plus |addx|) below 2^24, so that any fp32 summation
    order is exact; its fp32 and float64 references are equal and integers; the outliers sit on the seams;
  * tai_conv_bf16_plan refuses what tai_conv_bf16_forward refuses for the same dimensions, with the same words (in a child process
    that sees no device: an accepted forward call fails at its launch there instead of running on dummy pointers)."""
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
import bf16_cases as bc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'video-frame-inpainting_amd', 'csrc')
EINVAL = -1
NO_DEVICE = {'HIP_VISIBLE_DEVICES': '-1', 'ROCR_VISIBLE_DEVICES': '-1'}
INT_CASES = [c for c in bc.CASES if c.data == 'int']

# (N, K, H, W, k): refused by both entry points, then accepted by both
REFUSED = [(0, 16, 4, 4, 3), (-1, 16, 4, 4, 3), (1, 16, 0, 4, 3), (1, 16, 4, 0, 5), (1, 15, 4, 4, 3), (1, 0, 4, 4, 3), (1, 16, 4, 4, 4),
           (1, 16, 4, 4, 1), (1, 16, 4, 4, 9), (1 << 15, 16, 64, 64, 3), (1 << 12, 256, 64, 32, 7), (2, 16, 1 << 13, 1 << 13, 5),
           (1, 1 << 30, 1, 2, 3)]
ACCEPTED = [(1, 16, 1, 1, 3), (3, 16, 1, 1, 3), (8200, 16, 4, 4, 7), (1, 16, 4096, 4096, 5), ((1 << 27) - 1, 16, 1, 1, 3), (1, 256, 64, 64, 7)]


def _lib():
    from video_frame_inpainting_amd import _native
    return _native.lib()


def lib_plan(L, N, K, H, W, k):
    out = (ctypes.c_int * len(bc.PLAN_FIELDS))(*([-7] * len(bc.PLAN_FIELDS)))
    blocks = L.tai_conv_bf16_plan(N, K, H, W, k, out)
    return blocks, list(out)


def _same_plan(L, N, K, H, W, k):
    p = bc.plan(N, K, H, W, k)
    blocks, out = lib_plan(L, N, K, H, W, k)
    assert blocks == p.blocks and out == [getattr(p, f) for f in bc.PLAN_FIELDS], ((N, K, H, W, k), p, blocks, out)
    return p


def test_python_plan_equals_the_library_on_every_case():
    L = _lib()
    for c in bc.CASES:
        p = _same_plan(L, c.N, c.K, c.H, c.W, c.k)
        assert p.MW == c.mw, bc.case_id(c)
        assert p.blocks == p.tiles_x * p.tiles_y * p.groups * -(-c.K // bc.NT)
        assert p.lds_bytes <= 64 * 1024 and p.IMG * p.PH * p.pitch * bc.PIX_BYTES <= bc.MAX_PATCH_BYTES


def sweep_shapes(count=2000, seed=0):
    """N from 1 to 40,000 (log-uniform, so that both MW values and the image counts between occur), K in {16, 51, 64, 80, 256},
    H and W from 1 to 130, k in {3, 5, 7}; the corners of that box first."""
    rnd = random.Random(seed)
    shapes = [(N, K, H, W, k) for N in (1, 40000) for K in (16, 256) for H in (1, 130) for W in (1, 130) for k in (3, 5, 7)]
    while len(shapes) < count:
        N = min(40000, int(round(40000 ** rnd.random())))
        H, W = (rnd.randint(1, 130), rnd.randint(1, 130)) if rnd.random() < 0.5 else (rnd.randint(1, 12), rnd.randint(1, 12))
        shapes.append((N, rnd.choice((16, 51, 64, 80, 256)), H, W, rnd.choice((3, 5, 7))))
    return shapes


def test_python_plan_equals_the_library_on_a_sweep():
    L = _lib()
    seen = set()
    for (N, K, H, W, k) in sweep_shapes():
        if N * K * H * W >= 1 << 31:
            assert lib_plan(L, N, K, H, W, k)[0] == EINVAL
            continue
        p = _same_plan(L, N, K, H, W, k)
        f = bc.flags(N, 16, K, H, W, k)
        seen |= {(k, p.MW)} | {(k, name) for name in bc.FLAGS if f[name]}
    # the sweep itself reaches both MW values and the plan-dependent flags at each k, so the comparison covers those branches
    for k in (3, 5, 7):
        assert (k, 2) in seen and (k, 4) in seen
        for name in ('ragged_n', 'partial_x', 'partial_y', 'used_lt_mt', 'pitch_raised', 'img_capped_by_lds'):
            assert ((k, name) in seen) != ((k, name) in bc.IMPOSSIBLE), (k, name)


def test_every_claimed_flag_holds():
    for c in bc.CASES:
        f = bc.case_flags(c)
        assert f['mw'] == c.mw and f['kblocks'] == -(-c.K // bc.NT), bc.case_id(c)
        assert set(c.claims) <= set(bc.FLAGS), bc.case_id(c)
        assert all(f[name] for name in c.claims), (bc.case_id(c), [n for n in c.claims if not f[n]])
        assert c.C % c.nparts == 0 and c.C >= 16 and c.K >= 16 and c.epi in ('plain', 'pool', 'unpool', 'unpool_sum')
        assert c.epi == 'plain' or (c.H % 2 == 0 and c.W % 2 == 0)
        assert (c.act == 'tanh') <= (c.data == 'float')         # integers saturate tanh: it runs float data
    assert len({bc.case_id(c) for c in bc.CASES}) == len(bc.CASES)
    assert bc.case_flags(bc.FIRST_CASE)['mw'] == 2 and bc.plan(3, 16, 1, 1, 3).blocks == 1


def test_the_cases_cover_every_instance_and_every_route_at_each_k():
    for k in (3, 5, 7):
        cases = [c for c in bc.CASES if c.k == k]
        assert {c.mw for c in cases} == {2, 4}
        assert {c.act for c in cases if c.mw == 4} == {None, 'relu', 'tanh'}
        assert {c.act for c in cases if c.mw == 4 and c.data == 'int'} == {None, 'relu'}
        for name in bc.FLAGS:
            hit = [c for c in cases if bc.case_flags(c)[name]]
            assert bool(hit) != ((k, name) in bc.IMPOSSIBLE), (k, name)
            if hit:
                assert any(name in c.claims for c in hit) or name == 'ragged_k', (k, name)
        # the three epilogues on even planes at both MW values, a transposed weight at each k, a split input
        for mw in (2, 4):
            assert {c.epi for c in cases if c.mw == mw} >= {'plain'}
        assert any(c.transposed for c in cases)
    for mw in (2, 4):
        assert {c.epi for c in bc.CASES if c.mw == mw} == {'plain', 'pool', 'unpool', 'unpool_sum'}
        assert {c.nparts for c in bc.CASES if c.mw == mw} >= {1, 2, 4}
    # the routes that only the MW = 4 instances of the big layers take in the model
    at4 = [bc.case_flags(c) for c in bc.CASES if c.mw == 4]
    for name in ('ragged_n', 'used_lt_mt', 'img_capped_by_lds', 'pitch_raised', 'odd_w', 'odd_h', 'partial_x', 'partial_y', 'ragged_c',
                 'chunk_straddles_parts', 'multi_kblock'):
        assert any(f[name] for f in at4), name
    assert any(f['multi_kblock'] and f['ragged_k'] and f['ragged_c'] for f in at4)
    assert any(not f['pitch_raised'] and bc.plan(c.N, c.K, c.H, c.W, c.k).PW % 8 == 4 for c, f in
               ((c, bc.case_flags(c)) for c in bc.CASES if c.mw == 4))
    # a pitch the cap forbids raising (PW % 8 != 4, left at PW) at MW = 4
    assert any(not f['pitch_raised'] and bc.plan(c.N, c.K, c.H, c.W, c.k).PW % 8 != 4 for c, f in
               ((c, bc.case_flags(c)) for c in bc.CASES if c.mw == 4))
    assert any(c.C == 512 for c in bc.CASES) and {1, 7} <= {c.W for c in bc.CASES if c.H == 1}


def test_flags_that_no_shape_raises():
    """(3, img_capped_by_lds): over every even tile of either MT, the uncut image count stages at most MAX_PATCH_BYTES."""
    assert set(bc.IMPOSSIBLE) == {(3, 'img_capped_by_lds')}
    worst = 0
    for MT in (256, 128):
        for TW in range(2, bc.MAX_TW + 1, 2):
            for TH in range(2, MT // TW + 1, 2):
                worst = max(worst, (MT // (TH * TW)) * (TH + 2) * (TW + 2) * bc.PIX_BYTES)
    assert worst == bc.MAX_PATCH_BYTES


@pytest.mark.parametrize('c', INT_CASES, ids=bc.case_id)
def test_integer_cases_are_exact_in_any_order(c):
    x, w, b, addx = bc.int_case(c)
    for t in (x, w, b) + (() if addx is None else (addx,)):
        assert torch.equal(t, t.round()) and torch.equal(bc.bf16_round(t), t.double())          # integers, exact in bf16
    plain = bc.int_case(c, outliers=False)
    assert float(plain[0].abs().max()) <= 4 and bool((w != 0).all()) and float(w.abs().max()) <= 3 and float(b.abs().max()) <= 8
    assert addx is None or float(addx.abs().max()) <= 8
    # the cap on the absolute values bounds every partial sum of any order and sign pattern.  fp32 is enough to tell: sums of
    # non-negative integers are exact below 2^24, and one that reaches 2^24 cannot round back below it
    cap = bc.conv64(x.abs(), w.abs(), b.abs(), c.transposed, dtype=torch.float32, rounded=False).double()
    if addx is not None:
        cap[:, :, 0::2, 0::2] += addx.abs().double()
    assert float(cap.max()) < bc.CAP, float(cap.max())
    # the signed case: fp32 equals float64, integers throughout, within the cap
    r64 = bc.conv64(x, w, b, c.transposed)
    r32 = bc.conv64(x, w, b, c.transposed, dtype=torch.float32)
    assert torch.equal(r32.double(), r64) and torch.equal(r64, r64.round())
    ref = bc.reference(c, x, w, b, addx)
    for name, t in ref.items():
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= float(cap.max()), name
        assert torch.equal(t.float().double(), t), name
    assert float(ref['y'].abs().max()) > bc.OUTLIER            # the outliers reach the output


@pytest.mark.parametrize('c', INT_CASES, ids=bc.case_id)
def test_outliers_sit_on_the_seams(c):
    p = bc.plan(c.N, c.K, c.H, c.W, c.k)
    x = bc.int_case(c)[0]
    sites = bc.outlier_sites(c)
    assert len({(n, r, col) for n, _, r, col in sites}) == len(sites)
    assert int((x.abs() == bc.OUTLIER).sum()) == len(sites) and all(abs(float(x[s])) == bc.OUTLIER for s in sites)
    assert int((x == bc.OUTLIER).sum()) > 0 and int((x == -bc.OUTLIER).sum()) > 0 or len(sites) == 1
    where = {(n, r, col) for n, _, r, col in sites}
    images = {n for n, _, _, _ in sites}
    # the first and the last image of the first and of the last tile group; the last real image
    last_group = (p.groups - 1) * p.IMG
    assert {0, min(p.IMG, c.N) - 1, last_group, c.N - 1} <= images
    # the plane's corners, and both sides of the first tile edge in each direction
    for n in (0, c.N - 1):
        assert {(n, r, col) for r in (0, c.H - 1) for col in (0, c.W - 1)} <= where
        if c.W > p.TW:
            assert {(n, 0, p.TW - 1), (n, 0, p.TW)} <= where
        if c.H > p.TH:
            assert {(n, p.TH - 1, 0), (n, p.TH, 0)} <= where
    # channel C - 1 and the first channel of each part (where there are sites enough to go round)
    chans = bc.seam_channels(c.C, c.nparts)
    assert {c.C - 1} | {q * (c.C // c.nparts) for q in range(c.nparts)} <= set(chans)
    used = {ch for _, ch, _, _ in sites}
    assert used <= set(chans) and (used == set(chans) or len(sites) < 2 * len(chans))
    # lanes 0 and 63 of each wave: rows 16 f and 16 f + 15 of the first group's tile (0, 0)
    QW, QH = p.TW // 2, p.TH // 2
    for m in range(min(p.IMG, c.N) * p.TH * p.TW):
        if m % 16 in (0, 15):
            q, sub = m >> 2, m & 3
            i, r, col = q // (QW * QH), 2 * ((q // QW) % QH) + (sub >> 1), 2 * (q % QW) + (sub & 1)
            if i < c.N and r < c.H and col < c.W:
                assert (i, r, col) in where, (m, i, r, col)
    again = bc.int_case(c)
    assert all(a is None and b is None or torch.equal(a, b) for a, b in zip(bc.int_case(c), again))


def test_constants_are_the_sources():
    src = open(os.path.join(CSRC, 'conv_bf16.hip.inc')).read()

    def const(name):
        return eval(re.search(r'constexpr int %s = ([^;]+);' % name, src).group(1), {},
                    {'KC': bc.KC, 'FRAG_BYTES': 64 * 16})
    assert const('KC') == bc.KC and const('NT') == bc.NT and const('PIX_BYTES') == bc.PIX_BYTES
    assert const('FRAG_BYTES') == 1024 and const('STEP_BYTES') == bc.STEP_BYTES and const('MAX_PATCH_BYTES') == bc.MAX_PATCH_BYTES
    assert 'constexpr int group_steps(int k) { return k == 3 ? 5 : 7; }' in src and bc.GROUP_STEPS == {3: 5, 5: 7, 7: 7}
    assert 'constexpr int ksteps(int k) { return (k * k + 1) / 2; }' in src
    body = src[src.index('inline Plan plan('):]
    assert 'if (MW == 4 && best.blocks >= %d) break;' % bc.MW4_MIN_BLOCKS in body
    assert '((W + 1) & ~1) < %d ? ((W + 1) & ~1) : %d;' % (bc.MAX_TW, bc.MAX_TW) in body
    assert 'for (int MW = 4; MW >= 2; MW -= 2)' in body and 'const int MT = 64 * MW;' in body
    assert 'int pitch = best.PW + ((12 - best.PW % 8) % 8);' in body
    # the query and the launcher call the same function, and the query's order of out[] is PLAN_FIELDS
    capi = open(os.path.join(CSRC, 'capi_bf16.inc')).read()
    assert len(re.findall(r'cbf16::plan\(N, K, H, W, k\)', capi)) == 2
    order = re.search(r'const int v\[11\] = \{([^}]*)\}', capi).group(1)
    assert [s.strip().replace('pl.', '') for s in order.split(',')] == list(bc.PLAN_FIELDS)
    header = open(os.path.join(ROOT, 'include', 'tai_sepconv.h')).read()
    doc = header[header.index('out[0..10] = '):header.index('int tai_conv_bf16_plan(')]
    at = [doc.index(f if f != 'TW' else 'TW (') for f in bc.PLAN_FIELDS]
    assert at == sorted(at)


def _answers(L):
    """[(plan's answer, forward's answer)] over REFUSED + ACCEPTED, each (return code, message)."""
    xs = (ctypes.c_void_p * 1)(16)
    rows = []
    for (N, K, H, W, k) in REFUSED + ACCEPTED:
        out = (ctypes.c_int * 11)(*([-7] * 11))
        a = [L.tai_conv_bf16_plan(N, K, H, W, k, out), L.tai_sepconv_last_error().decode(), list(out)]
        b = [L.tai_conv_bf16_forward(xs, 1, 16, 16, 16, None, None, None, N, 16, K, H, W, k, 0, None), L.tai_sepconv_last_error().decode()]
        rows.append([a, b])
    return rows


def test_the_query_refuses_what_the_forward_refuses():
    from video_frame_inpainting_amd import _native
    _native.verify(_native.LIB_PATH)
    run = subprocess.run([sys.executable, os.path.abspath(__file__), '--answers', _native.LIB_PATH], env=dict(os.environ, **NO_DEVICE),
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = json.loads(run.stdout)
    assert len(rows) == len(REFUSED) + len(ACCEPTED)
    for shape, (a, b) in zip(REFUSED, rows):
        assert a[0] == EINVAL and b[0] == EINVAL and a[1] == b[1] and a[1].startswith('conv_bf16_forward: '), (shape, a, b)
        assert a[2] == [-7] * 11, shape                       # out untouched
    for shape, (a, b) in zip(ACCEPTED, rows[len(REFUSED):]):
        assert a[0] == bc.plan(*shape).blocks > 0 and a[1] == '' and b[0] != EINVAL, (shape, a, b)
    L = _lib()
    assert L.tai_conv_bf16_plan(1, 16, 4, 4, 3, None) == EINVAL and L.tai_sepconv_last_error() == b'null pointer'


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
