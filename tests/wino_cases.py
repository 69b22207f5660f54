"""Case generator for the kernel-level tests of the Winograd convolutions: F(2x2, 3x3) forward (csrc/wino_conv.hip.inc), its split-bf16
arithmetic (wino_split.hip.inc), F(4x4, 3x3) forward with its displaced-read and split-over-channels forms (wino43_conv.hip.inc) and the
weight gradient in either domain (wino_wrw.hip.inc, conv3x3_wrw_gen).  tests/test_gpu_wino_kernels.py runs the cases,
tests/test_wino_cases_cpu.py checks their conditions without a GPU.

The plans are restated in plain Python -- ``fwd22_plan`` (wino_forward_plan), ``wrw_plan`` (wrw_route), ``w43_splits``
(wino43_split_plan), ``w43_instance`` (wino43_instance), ``w43_placement`` (the workgroup -> (tile block, channel block) branches of
conv3x3_gen) -- and the CPU test holds them to the library's own answers (tai_conv3x3_wino_forward_plan, tai_conv3x3_wino_wrw_plan,
tai_conv3x3_wino43_splits) on every case and on a sweep, and reads the constants below back from the sources.  ``*_flags`` name the
device branches a launch takes, from its plan.

Data:
  * ``int_case`` (the F(2x2, 3x3) family): integers in fp32 -- x in [-4, 4], weights non-zero multiples of 4 in [-8, 8] (G g G^T is
    then exact: G carries 1/2), dy in [-2, 2], bias and addx in [-8, 8] -- with +-OUTLIER in x at ``outlier_sites``: both sides of every
    tile-block seam, the first and the last tile of the first and last image of a block, row ends, plane corners, channel C - 1, the
    first and last channel of each part, lanes 0 and 63 of a wave (the first and last tile of a block), both sides of the split
    boundaries of the weight gradient.  The cap is the ALGORITHM's, not the direct convolution's: ``wino22_abs_terms`` restates the
    stages on absolute values with absolute matrices, and every stage stays below 2^24 quanta (1; 1/4 for the weight gradient's last
    stage), so that any fp32 order is exact and the comparison is torch.equal.  tanh runs float data.
  * ``float_case`` (the F(4x4, 3x3) family: G carries 1/81 and 1/243, nothing is exact): x N(0, 1), w N(0, 2 / (9 C)), the same outlier
    sites.  Bound: TOL = 2e-5 (tests/test_gpu_wino43.py) against 1 + the LARGEST magnitude sum of the output's 4 x 4 tile
    (``tile_mag``): an outlier anywhere in a tile's 6 x 6 patch rounds into all 16 outputs of that tile, so the pixel's own magnitude
    sum does not bound its error, the tile's does.

``wino43_emulated`` is the F(4x4, 3x3) algorithm in fp32 torch (the transform matrices of tools/wino_f43_points_study.py on the
kernel's points (0, +-3/4, +-3/2, inf); not the kernel's summation order) with injectable defects: the CPU test shows that the clean
emulation passes the tile-magnitude bound on every float case and that each defect fails it.
"""
import collections
from fractions import Fraction as Fr

import numpy as np
import torch
import torch.nn.functional as F

# ---- constants of the sources (read back by the CPU test) -----------------------------------------------------------------------
KC, TM, TN = 8, 64, 64              # wino_conv.hip.inc: input channels per chunk, output channels x tiles per workgroup
TTM, TTN = 128, 32                  # ... the "tall" workgroup
CT = 8                              # wino_wrw.hip.inc: tiles per chunk
W43_KC, W43_TM, W43_TN = 4, 64, 32  # wino43_conv.hip.inc
W43_MIN_SPLIT_CHUNKS, W43_MAX_SPLITS = 8, 16
W43_POINTS = (Fr(3, 4), Fr(3, 2))   # PT_A, PT_B
CUS = 256
OUTLIER = 512.0
CAP = float(2 ** 24)
TOL22 = 4e-6                        # tests/test_gpu_wino_conv.py: max |got - ref| / (1 + mag), float data
TOL43 = 2e-5                        # tests/test_gpu_wino43.py
ACTS = {None: 0, 'relu': 1, 'tanh': 2}
FWD_FIELDS = ('split', 'tall', 'parts', 'epi', 'edge', 'kblocks', 'tblocks', 'nchunks', 'grid')        # tai_conv3x3_wino_forward_plan's out[]
WRW_FIELDS = ('tile', 'paired', 'ragged', 'kblocks', 'cblocks', 'nchunks', 'chunks_per_split', 'splits')  # tai_conv3x3_wino_wrw_plan's out[]


def _ceil(a, b):
    return -(-a // b)


# ---- F(2x2, 3x3) forward: wino_ex_arguments + wino_forward_plan ---------------------------------------------------------------------

def halo_geometry(H, W, k):
    """include/tai_sepconv.h on shift_k: image row 0 at row k/2 (in_oy = 1), image column 0 at column in_ox + k/2 - 1 (in_ox = 2),
    in_h >= H + in_oy + 1 + 3 (S - 1), in_w >= W + in_ox + 2 + 3 (S - 1) and even.  -> (S, top, left, in_h, in_w)"""
    S = (k + 2) // 3
    in_h, in_w = H + 2 + 3 * (S - 1), W + 4 + 3 * (S - 1)
    return S, k // 2, k // 2 + 1, in_h, in_w + (in_w & 1)


def fwd22_plan(N, C, K, H, W, nparts=1, shift_k=0, act=0, has_pool=False, has_addx=False, has_y2=False, window=None, split_buf=False,
               tall_on=True):
    """The plan of tai_conv3x3_wino_forward_ex as a dict over FWD_FIELDS, or None where the launcher refuses.  C is the kernel's channel
    count (S^2 Cin with shift_k); window = (in_h, in_w, in_oy, in_ox) or None for the plane H x W at (0, 0); the pooled output is the
    plain [N, K, H/2, W/2] tensor."""
    if nparts < 1 or nparts > 4 or (shift_k != 0 and nparts != 1) or (shift_k != 0 and not 4 <= shift_k <= 9):
        return None
    S = (shift_k + 2) // 3 if shift_k else 0
    if nparts > 1 and (C % nparts != 0 or (C // nparts) % 8 != 0):
        return None
    if S and (C % (S * S) != 0 or (C // (S * S)) % 8 != 0):
        return None
    if has_y2 and not has_addx:
        return None
    in_h, in_w, in_oy, in_ox = window if window else (H, W, 0, 0)
    if in_h == 0:
        in_h, in_w = H, W
    if has_pool and (N * K * (H // 2) * (W // 2) >= 1 << 29):
        return None
    if S and (in_oy < 1 or in_ox < 2 or in_h < H + in_oy + 1 + 3 * (S - 1) or in_w < W + in_ox + 2 + 3 * (S - 1)):
        return None
    if N <= 0 or C <= 0 or K <= 0 or H <= 0 or W <= 0 or not 0 <= act <= 2:
        return None
    ragged = H % 2 != 0 or W % 2 != 0
    if ragged and (has_pool or S or has_addx or (in_h, in_w, in_oy, in_ox) != (H, W, 0, 0)):
        return None
    if in_h < H + in_oy or in_w < W + in_ox or in_oy < 0 or in_ox < 0 or in_ox % 2 or (not ragged and in_w % 2):
        return None
    if N * C * in_h * in_w >= 1 << 29 or N * K * H * W >= 1 << 29:
        return None
    Kpad, nchunks = _ceil(K, TM) * TM, _ceil(C, KC)
    tiles = N * _ceil(H, 2) * _ceil(W, 2)
    epi = (1 if has_y2 else 2) if has_addx else 0
    if split_buf and ragged:
        return None
    tw = W // 2
    tw_ok = tw % 16 == 0 or (tw >= 2 and tw & (tw - 1) == 0)
    if split_buf and not S and tw_ok and not (epi and act != 0):
        p = dict(split=1, tall=0, parts=int(nparts > 1), epi=epi, edge=int(tw > 16 or in_ox > 0 or in_w > W + in_ox), kblocks=Kpad // TM,
                 tblocks=_ceil(tiles, TN), nchunks=nchunks)
    else:
        tall = int(Kpad % TTM == 0 and tall_on)
        pmode = 2 if S else int(nparts > 1)
        if epi and (act != 0 or pmode == 2):
            return None
        if pmode == 2 and act != 1:
            return None
        p = dict(split=0, tall=tall, parts=pmode, epi=epi if epi else (3 if ragged else 0), edge=0, kblocks=Kpad // (TTM if tall else TM),
                 tblocks=_ceil(tiles, TTN if tall else TN), nchunks=nchunks)
    p['grid'] = p['kblocks'] * p['tblocks']
    return p


FWD22_FLAGS = ('ragged_c', 'ragged_k', 'multi_kblock', 'block_straddles_images', 'partial_last_block', 'odd_h', 'odd_w', 'window_origin',
               'pool_window_even', 'pool_window_odd', 'xcd_block', 'no_xcd_block', 'split_declines')


def block_geometry(N, tiles_per_image, wtn):
    """(straddles, partial): some block of `wtn` consecutive tiles holds tiles of two images; the last block is not full."""
    tiles = N * tiles_per_image
    return (N > 1 and tiles_per_image % wtn != 0), tiles % wtn != 0


def fwd22_flags(c):
    p = fwd22_plan(*_fwd22_args(c))
    wtm, wtn = (TTM, TTN) if p['tall'] else (TM, TN)
    straddles, partial = block_geometry(c.N, _ceil(c.H, 2) * _ceil(c.W, 2), wtn)
    tw = c.W // 2
    return dict(p, **{
        'act': ACTS[c.act],
        'ragged_c': c.kernel_C % KC != 0,                       # the last chunk's channels past C read as zero
        'ragged_k': c.K % wtm != 0,                             # output channels past K: bias reads 0, stores dropped
        'multi_kblock': p['kblocks'] > 1,
        'block_straddles_images': straddles,
        'partial_last_block': partial,                          # tiles past the end: loads out of range, stores dropped
        'odd_h': c.H % 2 == 1, 'odd_w': c.W % 2 == 1,
        'window_origin': bool(c.window and not c.shift_k and (c.window[2] > 0 or c.window[3] > 0)),
        'pool_window_even': bool(c.pool and c.pool[2] % 2 == 0), 'pool_window_odd': bool(c.pool and c.pool[2] % 2 == 1),
        'xcd_block': p['grid'] % 8 == 0 and not p['split'],     # xcd_block() permutes the workgroups
        'no_xcd_block': p['grid'] % 8 != 0 and not p['split'],
        # a buffer in split arithmetic on a tile row the split kernel declines: the fp32 kernel on the same buffer
        'split_declines': c.arith == 'split' and not p['split'],
        'nparts': c.nparts, 'shift_k': c.shift_k,
    })


FCase = collections.namedtuple('FCase', 'N C K H W nparts act epi window pool shift_k arith data claims')
FCase.kernel_C = property(lambda c: c.C * ((c.shift_k + 2) // 3) ** 2 if c.shift_k else c.C)


def _fwd22_args(c):
    window = c.window
    if c.shift_k:
        _, _, _, in_h, in_w = halo_geometry(c.H, c.W, c.shift_k)
        window = (in_h, in_w, 1, 2)
    return (c.N, c.kernel_C, c.K, c.H, c.W, c.nparts, c.shift_k, ACTS[c.act], c.epi == 'pool', c.epi.startswith('unpool'), c.epi == 'unpool',
            window, c.arith == 'split')


def _f(N, C, K, H, W, claims='', nparts=1, act=None, epi='plain', window=None, pool=None, shift_k=0, arith='fp32', data=None):
    return FCase(N, C, K, H, W, nparts, act, epi, window, pool, shift_k, arith, data or ('float' if act == 'tanh' else 'int'),
                 tuple(claims.split()))


def _fwd22_cases():
    """Every (ACT, PARTS, TALL, EPI) instance wino_forward_impl selects, each on a shape of a rotating list (so that the flags meet
    different instances), then the cases for single flags.  C is the image's channel count (Cin with shift_k)."""
    out = []
    # (N, C per part, H, W), even planes: one tile; 135 tiles with seams inside images 7 and 14; 3 x 20 tiles; one image of 64 tiles
    even = [(1, 8, 2, 2), (15, 20, 6, 6), (3, 24, 8, 10), (2, 8, 16, 16), (5, 16, 4, 6)]
    odd = [(3, 24, 7, 9), (2, 8, 1, 1), (4, 12, 5, 6), (2, 16, 6, 11), (9, 8, 3, 3)]
    ks = {0: [3, 64, 130, 180], 1: [128, 70, 256, 200]}                # K by TALL: Kpad % 128 decides
    i = 0
    for tall in (0, 1):
        for pmode in (0, 1):
            for act in (None, 'relu', 'tanh'):
                for epi in ('plain', 'odd'):
                    N, cp, H, W = (odd if epi == 'odd' else even)[i % 5]
                    nparts = (2, 3, 4)[i % 3] if pmode else 1
                    cp = _ceil(cp, 8) * 8 if pmode else cp
                    out.append(_f(N, cp * nparts, ks[tall][i % 4], H, W, nparts=nparts, act=act))
                    i += 1
            for epi in ('unpool', 'unpool_sum'):
                N, cp, H, W = even[i % 5]
                nparts = (2, 3, 4)[i % 3] if pmode else 1
                cp = _ceil(cp, 8) * 8 if pmode else cp
                out.append(_f(N, cp * nparts, ks[tall][i % 4], H, W, nparts=nparts, epi=epi))
                i += 1
        # displaced reads (PARTS 2, ReLU): k = 5 and 7 skip the zero tail, k = 9 has none (the zero_taps == 0 branch)
        for k, (N, cin, H, W) in ((5, (3, 8, 6, 8)), (7, (2, 16, 4, 12)), (9, (3, 8, 6, 6)), (4, (1, 8, 4, 4)), (6, (2, 8, 2, 6)), (8, (1, 8, 4, 4))):
            out.append(_f(N, cin, ks[tall][k % 4], H, W, act='relu', shift_k=k, epi='pool' if k == 7 else 'plain'))
    out += [
        _f(1, 8, 3, 2, 2, 'no_xcd_block'),
        _f(15, 20, 130, 6, 6, 'ragged_c ragged_k multi_kblock block_straddles_images partial_last_block no_xcd_block', act='relu'),
        _f(3, 24, 256, 7, 9, 'odd_h odd_w multi_kblock block_straddles_images partial_last_block', act='relu'),
        _f(3, 72, 64, 8, 8, 'no_xcd_block', nparts=3),
        _f(32, 8, 64, 8, 8, 'xcd_block', act='relu'),                                       # 512 tiles: 8 workgroups
        _f(32, 8, 128, 8, 8, 'xcd_block'),                                                  # ... 16 tall ones
        _f(4, 12, 70, 5, 6, 'odd_h ragged_c ragged_k'),
        # an odd channel count: the tall workgroup's lanes 32-63 read the channel after their wave's even one
        _f(3, 11, 128, 4, 4, 'ragged_c'),
        _f(3, 11, 64, 4, 4, 'ragged_c', act='relu'),
        _f(4, 12, 70, 6, 5, 'odd_w ragged_c ragged_k block_straddles_images'),
        # an input window with a non-zero origin (the plane carries real data around the window; zero padding outside the plane only)
        _f(3, 16, 64, 6, 8, 'window_origin', window=(9, 14, 2, 4), act='relu'),
        _f(2, 8, 128, 4, 4, 'window_origin', window=(5, 6, 1, 2), epi='pool'),
        _f(5, 8, 70, 6, 6, 'window_origin partial_last_block', window=(8, 8, 1, 0), epi='unpool'),
        # the pooled output into a window of a larger plane, even and odd pool_oy
        _f(3, 8, 64, 8, 12, 'pool_window_even', epi='pool', pool=(10, 12, 2, 4), act='relu'),
        _f(3, 8, 130, 6, 6, 'pool_window_odd multi_kblock', epi='pool', pool=(7, 5, 3, 1), act='relu'),
        _f(2, 16, 128, 8, 8, 'pool_window_odd', epi='pool', pool=(5, 7, 1, 3)),
        _f(2, 16, 64, 8, 8, '', epi='pool'),
    ]
    # split bf16 arithmetic: every <A, parts, E, edge> instance; edge = a tile row over 16 tiles or an input window
    wide, narrow = (1, 8, 4, 64), (3, 8, 8, 8)            # tw = 32 (edge), tw = 4
    i = 0
    for parts in (0, 1):
        for edge in (0, 1):
            for act, epi in ((None, 'plain'), ('relu', 'plain'), ('tanh', 'plain'), (None, 'unpool'), (None, 'unpool_sum')):
                N, cp, H, W = narrow if (not edge or i % 2) else wide
                nparts = (2, 4, 3)[i % 3] if parts else 1
                window = (H + 2, W + 4, 1, 2) if (edge and i % 2) else None
                out.append(_f(N, cp * nparts, (64, 70, 130)[i % 3], H, W, nparts=nparts, act=act, epi=epi, window=window, arith='split'))
                i += 1
    out += [
        _f(2, 8, 64, 4, 32, '', epi='pool', arith='split', act='relu'),
        # tile rows of 3, 5 and 20 tiles: the split kernel declines, the fp32 kernel reads the same buffer
        _f(2, 8, 64, 6, 6, 'split_declines', arith='split', act='relu'),
        _f(1, 16, 128, 4, 40, 'split_declines', arith='split', epi='unpool'),
        _f(2, 8, 70, 4, 10, 'split_declines', arith='split', shift_k=0, nparts=1),
        # displaced reads never take the split kernel
        _f(2, 8, 64, 4, 8, 'split_declines', arith='split', act='relu', shift_k=5),
    ]
    return out


def _merged(cases, ident):
    """The cases without repeats (same id): the first occurrence, with the claims of all."""
    out = collections.OrderedDict()
    for c in cases:
        key = ident(c)
        out[key] = c if key not in out else out[key]._replace(claims=tuple(dict.fromkeys(out[key].claims + c.claims)))
    return list(out.values())


FWD22_CASES = _merged(_fwd22_cases(), lambda c: c[:-1])


def fwd22_instance(f):
    """The template arguments the launcher selects, from a case's flags: ('fp32', ACT, PARTS, TALL, EPI) or ('split', A, parts, E, edge)."""
    if f['split']:
        return ('split', 0 if f['epi'] else f['act'], f['parts'], f['epi'], f['edge'])
    return ('fp32', f['act'], f['parts'], f['tall'], f['epi'])


def fwd22_all_instances():
    fp32 = {('fp32', a, q, t, e) for a in (0, 1, 2) for q in (0, 1) for t in (0, 1) for e in (0, 3)}
    fp32 |= {('fp32', 0, q, t, e) for q in (0, 1) for t in (0, 1) for e in (1, 2)} | {('fp32', 1, 2, t, 0) for t in (0, 1)}
    split = {('split', a, q, 0, e) for a in (0, 1, 2) for q in (0, 1) for e in (0, 1)}
    split |= {('split', 0, q, E, e) for q in (0, 1) for E in (1, 2) for e in (0, 1)}
    return fp32, split


def fcase_id(c):
    return 'f22-%dx%dx%dx%dx%d-p%d-%s-%s%s%s%s-%s-%s' % (c.N, c.C, c.K, c.H, c.W, c.nparts, c.act or 'none', c.epi,
                                                        '-win%d.%d.%d.%d' % c.window if c.window else '', '-pw%d.%d.%d.%d' % c.pool if c.pool else '',
                                                        '-k%d' % c.shift_k if c.shift_k else '', c.arith, c.data)


# ---- weight gradient: wrw_plan, wrw43_plan, wrw_route --------------------------------------------------------------------------------

def wrw_plan(N, C, K, H, W, window=None, tile_pref=4, paired_on=True):
    """wrw_route as a dict over WRW_FIELDS, or None where the launcher refuses.  window = (in_h, in_w, in_oy, in_ox) or None."""
    in_h, in_w, in_oy, in_ox = window if window else (H, W, 0, 0)
    if in_oy < 0 or in_ox < 0 or in_oy + H > in_h or in_ox + W > in_w:
        return None
    if N <= 0 or C <= 0 or K <= 0 or H <= 0 or W <= 0:
        return None
    if N * C * in_h * in_w * 4 >= 1 << 31 or N * K * H * W * 4 >= 1 << 31:
        return None
    ragged = H % 2 != 0 or W % 16 != 0
    Hx, Wx = _ceil(H, 2) * 2, _ceil(W, 16) * 16
    # -- the F(4x4, 3x3)-domain kernel (wrw43_plan)
    halo = (in_h, in_w) != (H, W)
    if (tile_pref == 4 and H % 4 == 0 and W % 16 == 0 and not (halo and (in_oy < 1 or in_ox < 1 or in_oy + H + 1 > in_h or in_ox + W + 1 > in_w))
            and N * C * in_h * in_w * 4 + (in_w + 1) * 4 < 1 << 31):
        kblocks, cblocks, nchunks = _ceil(K, 64), _ceil(C, 32), N * (H // 4) * (W // 16)
        blocks = kblocks * cblocks

        def rounds(sp):
            return float(_ceil(blocks * sp, CUS)) / sp
        best, sp = 1e30, 1
        while sp <= 32 and sp <= nchunks and (sp == 1 or nchunks // sp >= 16):
            best = min(best, rounds(sp))
            sp += 1
        want = next(sp for sp in range(1, 33) if rounds(sp) <= 1.03 * best)
        if blocks * want < CUS:
            want = min(CUS // blocks, nchunks)
        cps = _ceil(nchunks, want)
        return dict(tile=4, paired=0, ragged=0, kblocks=kblocks, cblocks=cblocks, nchunks=nchunks, chunks_per_split=cps, splits=_ceil(nchunks, cps))
    kblocks, cblocks = _ceil(K, 64), _ceil(C, 64)
    nchunks = N * (Hx // 2) * (Wx // 2) // CT
    want = max(1, min(CUS // (kblocks * cblocks), nchunks))
    cps = _ceil(nchunks, want)
    pair = not ragged and W % 32 == 0
    if pair and cps & 1:
        cps += 1
    return dict(tile=2, paired=int(pair and paired_on), ragged=int(ragged), kblocks=kblocks, cblocks=cblocks, nchunks=nchunks, chunks_per_split=cps,
                splits=_ceil(nchunks, cps))


WRW_FLAGS = ('paired', 'plain', 'ragged_odd_h', 'ragged_w', 'window', 'one_block', 'multi_block', 'ragged_k', 'ragged_c', 'one_chunk_per_split',
             'many_chunks_per_split', 'short_last_split', 'bias', 'no_bias', 'xcd_placement', 'plain_placement')

GCase = collections.namedtuple('GCase', 'N C K H W window tile paired bias placement claims')


def _g(N, C, K, H, W, tile, claims='', window=None, paired=True, bias=True, placement=1):
    return GCase(N, C, K, H, W, window, tile, paired, bias, placement, tuple(claims.split()))


def wrw_flags(c):
    p = wrw_plan(c.N, c.C, c.K, c.H, c.W, c.window, c.tile, c.paired)
    grid = p['kblocks'] * p['cblocks'] * p['splits']
    cw = 32 if p['tile'] == 4 else 64
    return dict(p, **{
        'plain': p['tile'] == 2 and not p['paired'] and not p['ragged'],
        'ragged_odd_h': bool(p['ragged']) and c.H % 2 == 1, 'ragged_w': bool(p['ragged']) and c.W % 16 != 0,
        'window': c.window is not None,
        'one_block': p['kblocks'] * p['cblocks'] == 1, 'multi_block': p['kblocks'] > 1 and p['cblocks'] > 1,
        'ragged_k': c.K % 64 != 0, 'ragged_c': c.C % cw != 0,
        'one_chunk_per_split': p['chunks_per_split'] == 1, 'many_chunks_per_split': p['chunks_per_split'] > 2,
        'short_last_split': p['nchunks'] % p['chunks_per_split'] != 0,
        'bias': c.bias, 'no_bias': not c.bias,
        # conv3x3_wrw_gen permutes the workgroups over the XCDs where the grid is a multiple of 8 and the placement is on
        'xcd_placement': p['tile'] == 4 and grid % 8 == 0 and c.placement == 1,
        'plain_placement': p['tile'] == 4 and (grid % 8 != 0 or c.placement == 0),
    })


WRW_CASES = [
    # ---- tile 2 (the tile a case asks for; the plan may only confirm it)
    _g(2, 8, 8, 4, 32, 2, 'paired one_block ragged_k ragged_c'),
    _g(2, 8, 8, 4, 32, 2, 'plain one_block no_bias', paired=False, bias=False),
    _g(8, 70, 130, 8, 64, 2, 'paired multi_block ragged_k ragged_c many_chunks_per_split'),
    _g(2, 70, 130, 6, 16, 2, 'plain multi_block ragged_k ragged_c'),
    _g(3, 8, 8, 7, 16, 2, 'ragged_odd_h one_block'),
    _g(15, 70, 130, 5, 12, 2, 'ragged_odd_h ragged_w multi_block short_last_split'),
    _g(2, 16, 16, 6, 12, 2, 'ragged_w no_bias', bias=False),
    _g(2, 16, 24, 6, 16, 2, 'window plain', window=(8, 20, 1, 2)),
    _g(2, 16, 24, 5, 10, 2, 'window ragged_odd_h ragged_w', window=(7, 14, 1, 2)),
    _g(41, 200, 200, 6, 16, 2, 'plain multi_block many_chunks_per_split short_last_split'),
    # ---- tile 4 (conv3x3_wrw_gen): blocks of 64 x 32
    _g(2, 70, 130, 32, 64, 4, 'multi_block ragged_k ragged_c many_chunks_per_split short_last_split plain_placement'),
    _g(1, 8, 8, 4, 16, 4, 'one_block one_chunk_per_split plain_placement ragged_k ragged_c'),
    _g(2, 32, 64, 8, 32, 4, 'one_block xcd_placement'),
    _g(2, 32, 64, 8, 32, 4, 'one_block plain_placement no_bias', placement=0, bias=False),
    _g(2, 16, 24, 8, 16, 4, 'window', window=(10, 20, 1, 2)),
    _g(2, 16, 24, 8, 16, 4, 'window', window=(14, 24, 3, 4)),
    _g(3, 40, 70, 4, 48, 4, 'multi_block ragged_c ragged_k'),
]


def gcase_id(c):
    return 'wrw%d-%dx%dx%dx%dx%d%s%s%s%s' % (c.tile, c.N, c.C, c.K, c.H, c.W, '-win%d.%d.%d.%d' % c.window if c.window else '',
                                            '' if c.paired else '-unpaired', '' if c.bias else '-nobias', '' if c.placement else '-order')


# ---- F(4x4, 3x3) forward: wino43_instance, wino43_split_plan, the placement of conv3x3_gen --------------------------------------------

W43_INSTANCES = ((0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (0, 3))        # (ACT, EPI) in the launcher's table order


def w43_instance(act, has_pool, has_addx, has_y2):
    if has_pool:
        return 2 if act == 0 else 3
    if has_addx:
        return 5 if has_y2 else 6
    return 4 if act == 2 else act


def w43_splits(N, C, K, H, W, nparts=1, splitc_on=True):
    """wino43_split_plan: (splits, chunks_per_split)."""
    nchunks = _ceil(C, W43_KC) if C > 0 else 0
    one = (1, nchunks)
    if (not splitc_on or min(N, C, K, H, W) <= 0 or H % 4 or W % 4 or nparts < 1 or nparts > 4 or C % nparts
            or (nparts > 1 and (C // nparts) % W43_KC)):
        return one
    cpp = nchunks if nparts == 1 else C // nparts // W43_KC
    blocks = _ceil(N * (H // 4) * (W // 4), W43_TN) * _ceil(K, W43_TM)

    def cost(sp, cps):
        return float(_ceil(blocks * sp, CUS)) * (cps + 2) + (float(blocks) * (2 * sp + 1) / 64.0 if sp > 1 else 0.0)
    c1 = cost(1, nchunks)
    best, pick = c1, one
    for want in range(2, W43_MAX_SPLITS + 1):
        cps = _ceil(nchunks, want)
        if nparts > 1:
            if cps < cpp:
                while cpp % cps:
                    cps += 1
            else:
                cps = _ceil(cps, cpp) * cpp
        if cps < W43_MIN_SPLIT_CHUNKS:
            break
        sp = _ceil(nchunks, cps)
        if sp < 2:
            continue
        c = cost(sp, cps)
        if c < best:
            best, pick = c, (sp, cps)
    return pick if best <= 0.95 * c1 else one


def w43_placement(nblk, kblocks, placement):
    """The branch conv3x3_gen takes for a grid of nblk workgroups (the unsplit grid under SPLITC): 'order' (set_placement(0)),
    'one_kblock_per_xcd', 'kblocks_over_xcds' or 'fallback'."""
    tblocks = nblk // kblocks
    if not placement:
        return 'order'
    if nblk % 8 == 0 and kblocks <= 8 and 8 % kblocks == 0 and tblocks % (8 // kblocks) == 0:
        return 'one_kblock_per_xcd'
    if nblk % 8 == 0 and kblocks % 8 == 0:
        return 'kblocks_over_xcds'
    return 'fallback'


def w43_block_of(bid, nblk, kblocks, placement):
    """(tb, kb) of workgroup bid, as conv3x3_gen computes it."""
    tblocks, xcd, slot = nblk // kblocks, bid & 7, bid >> 3
    branch = w43_placement(nblk, kblocks, placement)
    if branch == 'one_kblock_per_xcd':
        return (xcd // kblocks) * (tblocks // (8 // kblocks)) + slot, xcd % kblocks
    if branch == 'kblocks_over_xcds':
        per = kblocks // 8
        return slot // per, xcd * per + slot % per
    return bid // kblocks, bid % kblocks


W43_FLAGS = ('ragged_c', 'ragged_k', 'k_not_multiple_of_4', 'block_straddles_images', 'partial_last_block', 'split_inside_part',
             'split_on_part_boundary', 'short_last_split')

HCase = collections.namedtuple('HCase', 'N C K H W nparts act epi form shift_k placement claims')     # form: plain | ws | blocks


def _h(N, C, K, H, W, claims='', nparts=1, act=None, epi='plain', form='plain', shift_k=0, placement=1):
    return HCase(N, C, K, H, W, nparts, act, epi, form, shift_k, placement, tuple(claims.split()))


def w43_flags(c):
    S = (c.shift_k + 2) // 3 if c.shift_k else 1
    kc = c.C * S * S
    kblocks, tblocks = _ceil(c.K, W43_TM), _ceil(c.N * (c.H // 4) * (c.W // 4), W43_TN)
    straddles, partial = block_geometry(c.N, (c.H // 4) * (c.W // 4), W43_TN)
    sp, cps = w43_splits(c.N, kc, c.K, c.H, c.W, c.nparts) if c.form == 'ws' else (1, _ceil(kc, W43_KC))
    nchunks, cpp = _ceil(kc, W43_KC), _ceil(kc // c.nparts, W43_KC)
    return {
        'instance': w43_instance(ACTS[c.act], c.epi == 'pool', c.epi.startswith('unpool'), c.epi == 'unpool'),
        'splits': sp, 'chunks_per_split': cps, 'kblocks': kblocks, 'tblocks': tblocks,
        'placement': w43_placement(kblocks * tblocks, kblocks, c.placement),
        'ragged_c': kc % W43_KC != 0, 'ragged_k': c.K % W43_TM != 0, 'k_not_multiple_of_4': c.K % 4 != 0,
        'block_straddles_images': straddles, 'partial_last_block': partial,
        'split_inside_part': sp > 1 and c.nparts > 1 and cps < cpp,
        'split_on_part_boundary': sp > 1 and c.nparts > 1 and cps >= cpp,
        'short_last_split': sp > 1 and nchunks % cps != 0,
    }


def _w43_cases():
    out = []
    shapes = [(1, 4, 5, 4, 4), (8, 51, 70, 12, 12), (3, 8, 64, 8, 20), (2, 12, 130, 8, 8)]
    epis = {0: (None, 'plain'), 1: ('relu', 'plain'), 2: (None, 'pool'), 3: ('relu', 'pool'), 4: ('tanh', 'plain'), 5: (None, 'unpool'), 6: (None, 'unpool_sum')}
    for inst in range(7):                                   # the 7 instances, plain and behind the split
        act, epi = epis[inst]
        out.append(_h(*shapes[inst % 4], act=act, epi=epi))
        out.append(_h(*((3, 128, 70, 8, 12) if inst % 2 else (2, 70, 64, 8, 8)), act=act, epi=epi, form='ws'))
    for k in (5, 7, 9):                                     # the 4 BLOCKS instances at every k
        for act, epi in ((None, 'plain'), ('relu', 'plain'), (None, 'pool'), ('relu', 'pool')):
            out.append(_h(3 if k == 5 else 2, 4 if k != 7 else 8, 70 if act else 64, 8, 12 if k == 5 else 8, act=act, epi=epi, form='blocks', shift_k=k))
    for placement in (1, 0):                                # each placement branch under both set_placement values
        out += [_h(8, 8, 128, 16, 32, act='relu', placement=placement),          # 32 blocks x 2 channel blocks: an XCD holds one channel block
                _h(1, 4, 1024, 4, 4, placement=placement),                       # 1 x 16: kblocks % 8 == 0
                _h(8, 51, 70, 12, 12, act='relu', placement=placement)]          # 3 x 2 = 6 workgroups: the fallback
    out += [
        _h(1, 4, 5, 4, 4, 'k_not_multiple_of_4 ragged_k partial_last_block'),
        _h(8, 51, 70, 12, 12, 'ragged_c ragged_k k_not_multiple_of_4 block_straddles_images partial_last_block', act='relu'),
        _h(3, 16, 64, 8, 8, '', nparts=2, act='relu'),
        _h(2, 32, 70, 8, 12, 'ragged_k', nparts=4, epi='unpool'),
        # the split over input channels: inside a part, on part boundaries, a shorter last split, ragged C with one part
        _h(3, 128, 70, 8, 12, '', form='ws'),
        _h(2, 74, 64, 8, 8, 'ragged_c short_last_split', form='ws'),
        _h(2, 256, 64, 8, 8, 'split_inside_part', nparts=2, form='ws', act='relu'),
        _h(2, 128, 64, 8, 8, 'split_on_part_boundary', nparts=4, form='ws'),
    ]
    return out


W43_CASES = _merged(_w43_cases(), lambda c: c[:-1])


def hcase_id(c):
    return 'f43-%s-%dx%dx%dx%dx%d-p%d-%s-%s%s%s' % (c.form, c.N, c.C, c.K, c.H, c.W, c.nparts, c.act or 'none', c.epi,
                                                   '-k%d' % c.shift_k if c.shift_k else '', '' if c.placement else '-order')


# A flag that no case of a family can reach, with the reason (asserted in the CPU test).
IMPOSSIBLE = {
    ('wrw2', 'xcd_placement'): 'the placement is an argument of conv3x3_wrw_gen (tile 4) alone',
    ('wrw2', 'plain_placement'): 'the placement is an argument of conv3x3_wrw_gen (tile 4) alone',
    ('wrw4', 'paired'): 'the load schemes are wino::wrw::conv3x3_wrw\'s: a tile-4 plan reports paired 0',
    ('wrw4', 'plain'): 'the load schemes are wino::wrw::conv3x3_wrw\'s',
    ('wrw4', 'ragged_odd_h'): 'wrw43_plan takes H % 4 == 0 only; other shapes run the tile-2 kernel',
    ('wrw4', 'ragged_w'): 'wrw43_plan takes W % 16 == 0 only; other shapes run the tile-2 kernel',
}


# ---- outlier sites -----------------------------------------------------------------------------------------------------------------

def seam_tiles(N, th, tw, wtn, extra=()):
    """Linear tile indices (image-major, row-major) worth an outlier: both sides of the first, a middle and the last block seam, the first
    and last tile of the first and of the last image of the first, a middle and the last block, both ends of the first and last tile
    row, and `extra`."""
    tpi, tiles = th * tw, N * th * tw
    nb = _ceil(tiles, wtn)
    out = {0, tiles - 1}
    for b in sorted({0, 1, nb // 2, nb - 1}):
        lo, hi = b * wtn, min(b * wtn + wtn, tiles) - 1
        if lo > hi:
            continue
        out |= {lo, hi} | ({lo - 1} if lo > 0 else set())
        n_lo, n_hi = lo // tpi, hi // tpi
        for n in (n_lo, n_hi):                   # the first and last tile of that image inside the block
            out |= {max(lo, n * tpi), min(hi, n * tpi + tpi - 1)}
    for n in (0, N - 1):
        for ty in (0, th - 1):
            out |= {(n * th + ty) * tw, (n * th + ty) * tw + tw - 1}
    out |= {t for t in extra if 0 <= t < tiles}
    return sorted(out)


def seam_channels(C, nparts):
    cp = C // nparts
    return sorted({C - 1} | {p * cp for p in range(nparts)} | {p * cp + cp - 1 for p in range(nparts)})


def outlier_sites(N, C, H, W, tile, wtn, nparts=1, extra_tiles=(), tw_ext=None):
    """[(n, channel, row, column)] in an [N, C, H, W] image, one per seam tile, inside the tile at a corner that rotates with the site
    (clipped to the plane: a tile of the zero-extended grid past the plane gets no site).  tile: 2 or 4; tw_ext: tiles per row of an
    extended grid (the ragged weight gradient)."""
    th, tw = _ceil(H, tile), tw_ext or _ceil(W, tile)
    chans = seam_channels(C, nparts)
    sites, seen = [], set()
    for j, t in enumerate(seam_tiles(N, th, tw, wtn, extra_tiles)):
        n, rem = divmod(t, th * tw)
        ty, tx = divmod(rem, tw)
        r, col = tile * ty + (tile - 1) * ((j >> 1) & 1), tile * tx + (tile - 1) * (j & 1)
        if tile * tx >= W:
            continue
        r, col = min(r, H - 1), min(col, W - 1)
        if (n, r, col) in seen:
            continue
        seen.add((n, r, col))
        sites.append((n, chans[j % len(chans)], r, col))
    for n in (0, N - 1):                              # the plane's corners
        for r in (0, H - 1):
            for col in (0, W - 1):
                if (n, r, col) not in seen:
                    seen.add((n, r, col))
                    sites.append((n, chans[len(sites) % len(chans)], r, col))
    return sites


def _put_outliers(x, sites):
    idx = torch.tensor(sites, dtype=torch.long).t()
    sign = torch.ones(len(sites))
    sign[1::2] = -1
    x[idx[0], idx[1], idx[2], idx[3]] = OUTLIER * sign
    return x


def fwd22_sites(c):
    wtn = TTN if fwd22_plan(*_fwd22_args(c))['tall'] else TN
    return outlier_sites(c.N, c.C, c.H, c.W, 2, wtn, c.nparts)


def wrw_sites(c):
    """The forward sites of the chunk grid, plus the tiles on either side of the first, a middle and the last split boundary."""
    p = wrw_plan(c.N, c.C, c.K, c.H, c.W, c.window, c.tile, c.paired)
    tile = p['tile']
    per_chunk = 4 if tile == 4 else CT
    tw_ext = c.W // 4 if tile == 4 else _ceil(c.W, 16) * 16 // 2
    cuts = sorted({s * p['chunks_per_split'] * per_chunk for s in {1, p['splits'] // 2, p['splits'] - 1} if 0 < s < p['splits']})
    extra = [t for cut in cuts for t in (cut - 1, cut)]
    return outlier_sites(c.N, c.C, c.H, c.W, tile, per_chunk * p['chunks_per_split'], 1, extra, tw_ext)


def w43_sites(c):
    return outlier_sites(c.N, c.C, c.H, c.W, 4, W43_TN, c.nparts)


# ---- data --------------------------------------------------------------------------------------------------------------------------

def _ri(g, lo, hi, *s):
    return torch.randint(lo, hi + 1, s, generator=g).float()


def _mult4(g, *s):
    """Non-zero multiples of 4 in [-8, 8]."""
    return torch.tensor([-8., -4., 4., 8.])[torch.randint(0, 4, s, generator=g)]


def fwd22_data(c, seed=1, outliers=True):
    """(x, w, bias, addx or None).  x: the image [N, C, H, W] (with shift_k the Cin-channel image of the k x k convolution and w is
    [K, C, k, k]); with an input window x is the whole plane [N, C, in_h, in_w], real data everywhere, and the sites are placed in the
    window."""
    g = torch.Generator().manual_seed(seed)
    k = c.shift_k or 3
    in_h, in_w, oy, ox = c.window if c.window else (c.H, c.W, 0, 0)
    if c.data == 'int':
        x, w, b = _ri(g, -4, 4, c.N, c.C, in_h, in_w), _mult4(g, c.K, c.C, k, k), _ri(g, -8, 8, c.K)
        addx = _ri(g, -8, 8, c.N, c.K, c.H // 2, c.W // 2) if c.epi.startswith('unpool') else None
    else:
        x, w, b = torch.randn(c.N, c.C, in_h, in_w, generator=g), torch.randn(c.K, c.C, k, k, generator=g) * (2.0 / (k * k * c.C)) ** 0.5, torch.randn(c.K, generator=g)
        addx = torch.randn(c.N, c.K, c.H // 2, c.W // 2, generator=g) if c.epi.startswith('unpool') else None
    if outliers and c.data == 'int':
        _put_outliers(x[:, :, oy:oy + c.H, ox:ox + c.W], fwd22_sites(c))
    return x, w, b, addx


def activate(y, act):
    return torch.relu(y) if act == 'relu' else (torch.tanh(y) if act == 'tanh' else y)


def conv_reference(x, w, b, H, W, window=None, act=None, addx=None, dtype=torch.float64):
    """{'y', 'pool', 'sum' (where addx is given), 'mag'}: the "same" convolution of the plane x (zero padding outside the plane only), cropped
    to the window; mag = the magnitude sum sum |x| |w| + |b| of every output."""
    k = w.shape[2]
    oy, ox = (window[2], window[3]) if window else (0, 0)
    crop = lambda t: t[:, :, oy:oy + H, ox:ox + W]
    y = activate(crop(F.conv2d(x.to(dtype), w.to(dtype), b.to(dtype), padding=k // 2)), act)
    out = {'y': y, 'pool': F.max_pool2d(y, 2) if H % 2 == 0 and W % 2 == 0 else None,
           'mag': crop(F.conv2d(x.to(dtype).abs(), w.to(dtype).abs(), b.to(dtype).abs(), padding=k // 2))}
    if addx is not None:
        s = y.clone()
        s[:, :, 0::2, 0::2] += addx.to(dtype)
        out['sum'] = s
    return out


def block3x3_weight(w):
    """[K, Cin, k, k] -> [K, S^2 Cin, 3, 3]: the header's "k x k filter cut into S x S blocks of 3 x 3 taps, ZERO PAST k", channel block
    (a, b) = a S + b."""
    K, C, k, _ = w.shape
    S = (k + 2) // 3
    wp = F.pad(w, (0, 3 * S - k, 0, 3 * S - k)).view(K, C, S, 3, S, 3).permute(0, 2, 4, 1, 3, 5)
    return wp.reshape(K, S * S * C, 3, 3).contiguous()


def halo_plane(x, k):
    """The plane of halo_geometry with the image inside and zeros around it; -> (plane, in_h, in_w, in_oy, in_ox)."""
    N, C, H, W = x.shape
    _, top, left, in_h, in_w = halo_geometry(H, W, k)
    plane = torch.zeros(N, C, in_h, in_w)
    plane[:, :, top:top + H, left:left + W] = x
    return plane, in_h, in_w, 1, 2


def wrw_data(c, seed=1, outliers=True, integers=True):
    """(x plane [N, C, in_h, in_w], dy [N, K, H, W])."""
    g = torch.Generator().manual_seed(seed)
    in_h, in_w, oy, ox = c.window if c.window else (c.H, c.W, 0, 0)
    if integers:
        x, dy = _ri(g, -4, 4, c.N, c.C, in_h, in_w), _ri(g, -2, 2, c.N, c.K, c.H, c.W)
    else:
        x, dy = torch.randn(c.N, c.C, in_h, in_w, generator=g), torch.randn(c.N, c.K, c.H, c.W, generator=g)
    if outliers:
        _put_outliers(x[:, :, oy:oy + c.H, ox:ox + c.W], wrw_sites(c))
    return x, dy


def wrw_reference(x, dy, H, W, window=None):
    """(dw [K, C, 3, 3], db [K]) in float64: dw[k, c, a, b] = sum dy[n, k, y, x] plane[n, c, oy + y + a - 1, ox + x + b - 1], zeros outside
    the plane."""
    oy, ox = (window[2], window[3]) if window else (0, 0)
    xp = F.pad(x.double(), (1, 1, 1, 1))
    d = dy.double()
    dw = torch.stack([torch.stack([torch.einsum('nkyx,ncyx->kc', d, xp[:, :, oy + a:oy + a + H, ox + b:ox + b + W]) for b in range(3)], -1)
                      for a in range(3)], -2)
    return dw, d.sum((0, 2, 3))


def w43_data(c, seed=1, outliers=True):
    """(x [N, C, H, W], w [K, C, k, k], bias, addx or None), float; the outliers in x."""
    g = torch.Generator().manual_seed(seed)
    k = c.shift_k or 3
    x = torch.randn(c.N, c.C, c.H, c.W, generator=g)
    w = torch.randn(c.K, c.C, k, k, generator=g) * (2.0 / (k * k * c.C)) ** 0.5
    b = torch.randn(c.K, generator=g)
    addx = torch.randn(c.N, c.K, c.H // 2, c.W // 2, generator=g) if c.epi.startswith('unpool') else None
    if outliers:
        _put_outliers(x, w43_sites(c))
    return x, w, b, addx


def tile_mag(mag, tile=4):
    """The largest magnitude sum of each tile x tile output tile, at every pixel of that tile (tiles counted from the plane's origin; a
    plane whose side is no multiple of ``tile`` ends in partial tiles)."""
    H, W = mag.shape[-2:]
    m = F.max_pool2d(mag, tile, ceil_mode=True)
    return m.repeat_interleave(tile, -2).repeat_interleave(tile, -1)[..., :H, :W]


def tile_ratio(got, ref, mag):
    """max |got - ref| / (1 + the tile's largest mag); NaN in got counts as infinite."""
    err = (got.double() - ref).abs() / (1 + tile_mag(mag))
    return float('inf') if bool(torch.isnan(err).any()) else float(err.max())


# ---- the staged cap of the F(2x2, 3x3) algorithm -----------------------------------------------------------------------------------

_BT2 = torch.tensor([[1., 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
_G2 = torch.tensor([[1., 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
_AT2 = torch.tensor([[1., 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


def fwd22_patch_source(c, x):
    """[N, kernel C, H + 2, W + 2] (sides rounded up to even): what the patches of a case's tiles are cut from -- the image in its frame of
    zero padding; the window of a plane in its frame of plane pixels (zeros outside the plane); with shift_k the S x S displaced copies of
    the halo-carrying plane, channel block a S + b displaced by (3a, 3b)."""
    H, W = c.H, c.W
    if c.shift_k:
        S = (c.shift_k + 2) // 3
        plane, _, _, oy, ox = halo_plane(x, c.shift_k)
        src = torch.cat([plane[:, :, oy - 1 + 3 * a:oy + 3 * a + H + 1, ox - 1 + 3 * b:ox + 3 * b + W + 1] for a in range(S) for b in range(S)], 1)
    else:
        oy, ox = (c.window[2], c.window[3]) if c.window else (0, 0)
        src = F.pad(x, (1, 1, 1, 1))[:, :, oy:oy + H + 2, ox:ox + W + 2]
    return F.pad(src, (0, W % 2, 0, H % 2))


def wino22_abs_terms(src, w, b=None, addx=None):
    """The stages of the F(2x2, 3x3) forward on absolute values with absolute matrices, each as its largest value in units of its quantum 1:
    {'V': |B^T| |d| |B|, 'U': |G| |g| |G^T|, 'M': sum over channels of U V (+ |bias| at the position it rides in), 'Y': |A^T| M |A| (+ |addx|)}.
    src: fwd22_patch_source; w: the 3 x 3 weight the kernel sees ([K, kernel C, 3, 3]).  Every partial sum of every order and sign pattern
    is bounded by these; all are integers on int_case data."""
    bt, gg, at = _BT2.abs(), _G2.abs(), _AT2.abs()
    V = torch.einsum('ai,nctuij,bj->nctuab', bt, src.double().abs().unfold(2, 4, 2).unfold(3, 4, 2), bt)
    U = torch.einsum('ai,kcij,bj->kcab', gg, w.double().abs(), gg)
    M = torch.einsum('kcab,nctuab->nktuab', U, V)
    if b is not None:
        M = M + b.double().abs().view(1, -1, 1, 1, 1, 1)
    Y = torch.einsum('ia,nktuab,jb->nktuij', at, M, at)
    out = {'V': float(V.max()), 'U': float(U.max()), 'M': float(M.max()), 'Y': float(Y.max())}
    if addx is not None:
        out['Y'] += float(addx.abs().max())
    return out


def wino22_wrw_abs_terms(x, dy, H, W, window=None):
    """The same for the weight gradient: 'V' as above (of the window's patches), 'D': |A| |dy| |A^T|, 'M': sum over all tiles of D V (quantum
    1), 'dw': |G^T| M |G| in units of its quantum 1/4, 'db': sum |dy|."""
    oy, ox = (window[2], window[3]) if window else (0, 0)
    xp = F.pad(x.double().abs(), (1, 1, 1, 1))[:, :, oy:oy + H + 2, ox:ox + W + 2]       # the window with its one-pixel frame
    xp = F.pad(xp, (0, W % 2, 0, H % 2))
    bt, gg, at = _BT2.abs(), _G2.abs(), _AT2.abs()
    V = torch.einsum('ai,nctuij,bj->nctuab', bt, xp.unfold(2, 4, 2).unfold(3, 4, 2), bt)
    d = F.pad(dy.double().abs(), (0, W % 2, 0, H % 2)).unfold(2, 2, 2).unfold(3, 2, 2)
    D = torch.einsum('ia,nktuij,jb->nktuab', at, d, at)
    M = torch.einsum('nktuab,nctuab->kcab', D, V)
    dw = torch.einsum('ai,kcab,bj->kcij', gg, M, gg)
    return {'V': float(V.max()), 'D': float(D.max()), 'M': float(M.max()), 'dw': 4 * float(dw.max()), 'db': float(dy.double().abs().sum((0, 2, 3)).max())}


# ---- F(4x4, 3x3) in fp32 torch, with defects -----------------------------------------------------------------------------------------

def w43_matrices():
    """(A^T [4, 6], G [6, 3], B^T [6, 6]) of Cook-Toom F(4, 3) for correlation on the points (0, a, -a, b, -b, inf), float64."""
    a, b = W43_POINTS
    P = [Fr(0), a, -a, b, -b]
    G, AT = [], [[None] * 6 for _ in range(4)]
    for j, p in enumerate(P):
        n = Fr(1)
        for l, q in enumerate(P):
            if l != j:
                n *= (p - q)
        G.append([p ** k / n for k in range(3)])
        for i in range(4):
            AT[i][j] = p ** i
    G.append([Fr(0), Fr(0), Fr(1)])
    for i in range(4):
        AT[i][5] = Fr(1) if i == 3 else Fr(0)
    A = np.array([[float(AT[i][j] * G[j][k]) for j in range(6)] for i in range(4) for k in range(3)])
    BT = np.zeros((6, 6))
    for l in range(6):
        rhs = np.array([1.0 if l == i + k else 0.0 for i in range(4) for k in range(3)])
        BT[:, l] = np.linalg.lstsq(A, rhs, rcond=None)[0]
    BT = np.array([[float(Fr(v).limit_denominator(1 << 16)) for v in row] for row in BT])
    f = lambda m: np.array([[float(v) for v in row] for row in m])
    return f(AT), f(G), BT


DEFECTS = ('drop_last_channel', 'row_end_reads_next_tile', 'replicate_padding', 'skip_last_tile_of_block', 'swap_images_at_seam')


def wino43_emulated(x, w, b, defect=None):
    """conv(x, w) + b as F(4x4, 3x3) in fp32 (transforms and the channel reduction as fp32 einsums / bmm).  defect: one of DEFECTS --
    channel C - 1 left out; the last tile of every tile row reads the first column of the NEXT row's first tile where the zero padding
    should be; replicated instead of zero padding; the last tile of every 32-tile block never stored (NaN); the two images on either
    side of the first block seam that lies between images... swapped in the output."""
    assert defect is None or defect in DEFECTS
    AT, G, BT = w43_matrices()
    N, C, H, W = x.shape
    K = w.shape[0]
    Gt, bt, at = torch.tensor(G), torch.tensor(BT).float(), torch.tensor(AT).float()
    if defect == 'drop_last_channel':
        x = x.clone()
        x[:, C - 1] = 0
    xp = F.pad(x, (1, 1, 1, 1), mode='replicate' if defect == 'replicate_padding' else 'constant')
    d = xp.unfold(2, 6, 4).unfold(3, 6, 4).clone()                          # [N, C, TH, TW, 6, 6]
    TH, TW = d.shape[2], d.shape[3]
    if defect == 'row_end_reads_next_tile':
        flat = x.reshape(N, C, H * W)
        for ty in range(TH):
            for i in range(6):
                r = 4 * ty - 1 + i
                if 0 <= r < H and (r + 1) * W < H * W:
                    d[:, :, ty, TW - 1, i, 5] = flat[:, :, (r + 1) * W]       # the pixel after the row's end in memory
    U = torch.einsum('ai,kcij,bj->abkc', Gt, w.double(), Gt).float().reshape(36, K, C)
    t = torch.einsum('ai,nctuij->nctuaj', bt, d)
    V = torch.einsum('nctuaj,bj->abcntu', t, bt).reshape(36, C, N * TH * TW)
    Mm = torch.bmm(U, V).reshape(6, 6, K, N, TH, TW)
    Y = torch.einsum('ibkntu,jb->nktiuj', torch.einsum('ia,abkntu->ibkntu', at, Mm), at).reshape(N, K, H, W) + b.view(1, -1, 1, 1)
    if defect == 'skip_last_tile_of_block':
        Yt = Y.view(N, K, TH, 4, TW, 4)
        for tlin in range(W43_TN - 1, N * TH * TW, W43_TN):
            n, rem = divmod(tlin, TH * TW)
            Yt[n, :, rem // TW, :, rem % TW, :] = float('nan')
    if defect == 'swap_images_at_seam' and N > 1:
        n = max(1, min(N - 1, W43_TN // (TH * TW)))                            # the image that starts at (or after) the first block seam
        Y = Y.clone()
        Y[[n - 1, n]] = Y[[n, n - 1]]
    return Y
