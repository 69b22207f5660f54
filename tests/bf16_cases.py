"""Case generator for the kernel-level tests of the opt-in bf16 convolution (csrc/conv_bf16.hip.inc, 18 instances
conv_bf16<KS, MW, ACT>): tests/test_gpu_conv_bf16_kernel.py runs the cases, tests/test_bf16_cases_cpu.py checks their conditions
without a GPU.

``plan`` restates cbf16::plan (the tile, the image count and the patch pitch of a launch) in plain Python; the CPU test holds it to
the library's own answer (tai_conv_bf16_plan) on every case and on a sweep, and reads the constants below back from the sources.
``flags`` names the routes a launch takes inside the kernel, from its plan.

Data:
  * ``int_case``: integers stored in fp32 -- x in [-4, 4], weights in [-3, 3] and never zero, bias (and addx) in [-8, 8] -- with
    +-OUTLIER on the seams where the kernel changes hands (``outlier_sites``): tile corners and the pixels on either side of a tile
    edge, the first and last image of a multi-image tile, the last real image of a ragged group, channel C - 1 and the first and
    last channel of each part, and the pixels that lanes 0 and 63 of each wave own.  All are exact in bf16, and the sum of the
    absolute terms of every output stays below 2^24 (asserted per case in the CPU test): any fp32 summation order gives the
    float64 value, so the comparison is torch.equal.
  * ``float_case``: tests/test_gpu_conv_bf16.py's data, x N(0, 1), w N(0, 1 / sqrt(C k^2)), bias N(0, 0.1).

``reference``: float64 convolution of the bf16-rounded operands (bf16_emulation.bf16_round), then bias, activation, 2 x 2 max pool
and fixed unpooling in float64.
"""
import collections
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bf16_emulation import bf16_round  # noqa: E402

KC = 16                     # input channels per chunk
NT = 64                     # output channels per workgroup
PIX_BYTES = 2 * KC          # one staged pixel
STEP_BYTES = 4 * 64 * 16    # the four B fragments of one k-step
MAX_PATCH_BYTES = 32 * 1024
MAX_TW = 32
MW4_MIN_BLOCKS = 512        # MW = 4 where its grid has at least this many workgroups
GROUP_STEPS = {3: 5, 5: 7, 7: 7}
OUTLIER = 512.0
CAP = float(2 ** 24)
ACTS = {None: 0, 'relu': 1, 'tanh': 2}
PLAN_FIELDS = ('MW', 'TH', 'TW', 'IMG', 'PH', 'PW', 'pitch', 'tiles_x', 'tiles_y', 'groups', 'lds_bytes')     # tai_conv_bf16_plan's out[]

Plan = collections.namedtuple('Plan', PLAN_FIELDS + ('blocks',))


def ksteps(k):
    return (k * k + 1) // 2


def _ceil(a, b):
    return -(-a // b)


def plan(N, K, H, W, k):
    """cbf16::plan: the even TH x TW and the image count IMG that need the fewest workgroups of MT = 64 MW pixels (ties: the fewest
    staged pixels; first found wins, TW outer and TH inner, ascending), the patch within MAX_PATCH_BYTES; MW = 4 where that grid
    has MW4_MIN_BLOCKS workgroups, else 2; the pitch raised to 4 mod 8 where the patch still fits."""
    P, kblocks = k // 2, _ceil(K, NT)
    best = None
    for MW in (4, 2):
        MT = 64 * MW
        best_blocks, best_staged = -1, 0
        wmax, hmax = min((W + 1) & ~1, MAX_TW), (H + 1) & ~1
        for TW in range(2, wmax + 1, 2):
            for TH in range(2, hmax + 1, 2):
                if TH * TW > MT:
                    break
                PH, PW = TH + 2 * P, TW + 2 * P
                IMG = min(MT // (TH * TW), N)
                while IMG > 1 and IMG * PH * PW * PIX_BYTES > MAX_PATCH_BYTES:
                    IMG -= 1
                if IMG * PH * PW * PIX_BYTES > MAX_PATCH_BYTES:
                    continue
                tiles = _ceil(N, IMG) * _ceil(H, TH) * _ceil(W, TW)
                staged = tiles * IMG * PH * PW
                if best_blocks < 0 or tiles < best_blocks or (tiles == best_blocks and staged < best_staged):
                    best_blocks, best_staged = tiles, staged
                    best = dict(MW=MW, TH=TH, TW=TW, IMG=IMG, PH=PH, PW=PW, pitch=PW, tiles_x=_ceil(W, TW), tiles_y=_ceil(H, TH),
                                groups=_ceil(N, IMG), blocks=tiles * kblocks)
        if MW == 4 and best['blocks'] >= MW4_MIN_BLOCKS:
            break
    pitch = best['PW'] + (12 - best['PW'] % 8) % 8
    if best['IMG'] * best['PH'] * pitch * PIX_BYTES <= MAX_PATCH_BYTES:
        best['pitch'] = pitch
    best['lds_bytes'] = ((best['IMG'] * best['PH'] * best['pitch'] * PIX_BYTES + 15) & ~15) + GROUP_STEPS[k] * STEP_BYTES
    return Plan(**best)


FLAGS = ('ragged_n', 'partial_x', 'partial_y', 'used_lt_mt', 'pitch_raised', 'odd_w', 'odd_h', 'img_capped_by_lds', 'multi_kblock',
         'ragged_k', 'ragged_c', 'chunk_straddles_parts')


def flags(N, C, K, H, W, k, nparts=1):
    """The routes of one launch, from its plan: {'mw': 4 or 2, 'kblocks': n, flag: bool for every name in FLAGS}."""
    p = plan(N, K, H, W, k)
    MT = 64 * p.MW
    return {
        'mw': p.MW,
        'kblocks': _ceil(K, NT),
        'ragged_n': N % p.IMG != 0,                                 # a group with images past N: staged as zero, stores skipped
        'partial_x': W % p.TW != 0,
        'partial_y': H % p.TH != 0,
        'used_lt_mt': p.IMG * p.TH * p.TW < MT,                     # rows (and whole quads) of the tile past its pixels
        'pitch_raised': p.pitch != p.PW,
        'odd_w': W % 2 == 1,                                        # the scalar store path and its `right` guard
        'odd_h': H % 2 == 1,                                        # the `below` guard
        'img_capped_by_lds': p.IMG < min(MT // (p.TH * p.TW), N),   # IMG cut by the patch cap
        'multi_kblock': K > NT,
        'ragged_k': K % NT != 0,
        'ragged_c': C % KC != 0,                                    # the last chunk's channels past C are staged as zero
        'chunk_straddles_parts': nparts > 1 and (C // nparts) % KC != 0,
    }


# ---- the cases -------------------------------------------------------------------------------------------------------------

Case = collections.namedtuple('Case', 'N K H W k C nparts act epi transposed data mw claims')


def _c(N, K, H, W, k, mw, claims, C=16, nparts=1, act=None, epi='plain', transposed=False, data='int'):
    return Case(N, K, H, W, k, C, nparts, act, epi, transposed, data, mw, tuple(claims.split()))


# (N, K, H, W, k), the MW its plan gives, the flags it is there for; then C, parts, activation, epilogue, weight form, data.
# epi: plain | pool (y and ypool) | unpool (y and y2 = y + unpool(addx)) | unpool_sum (y receives the sum).  tanh runs float data.
CASES = [
    # ---- MW = 4
    _c(8200, 16, 4, 4, 3, 4, 'ragged_n', act='relu', epi='pool'),
    _c(8200, 16, 4, 4, 3, 4, 'ragged_n ragged_c', C=24, epi='unpool'),
    _c(8200, 16, 4, 4, 3, 4, 'ragged_n', act='tanh', epi='unpool_sum', data='float'),
    _c(2041, 256, 4, 4, 3, 4, 'ragged_n multi_kblock', act='relu'),
    _c(2100, 16, 7, 9, 3, 4, 'odd_h odd_w partial_x partial_y ragged_n ragged_c chunk_straddles_parts', C=40, nparts=2),
    _c(128, 16, 32, 32, 3, 4, 'pitch_raised', act='relu', epi='unpool', transposed=True),
    _c(128, 16, 32, 32, 3, 4, 'pitch_raised', data='float'),
    _c(128, 16, 32, 32, 7, 4, 'pitch_raised', act='relu', epi='pool'),
    _c(128, 16, 32, 32, 7, 4, 'pitch_raised', act='tanh', data='float'),
    _c(512, 16, 16, 16, 5, 4, '', act='relu', epi='pool'),
    _c(512, 16, 16, 16, 5, 4, 'chunk_straddles_parts', C=48, nparts=4, epi='unpool_sum', transposed=True),
    _c(512, 16, 16, 16, 5, 4, '', act='tanh', epi='unpool', data='float'),
    _c(128, 16, 31, 33, 5, 4, 'partial_x partial_y odd_h odd_w', act='relu'),
    _c(8200, 16, 4, 4, 7, 4, 'img_capped_by_lds used_lt_mt', epi='unpool'),
    _c(2050, 16, 8, 8, 7, 4, 'ragged_n', act='relu', epi='unpool_sum'),
    _c(33000, 16, 1, 1, 3, 4, 'odd_h odd_w partial_x partial_y ragged_n', act='relu'),
    _c(420, 16, 15, 20, 3, 4, 'partial_y odd_h', C=24, act='relu'),
    _c(700, 80, 10, 13, 7, 4, 'multi_kblock ragged_k ragged_c chunk_straddles_parts odd_w partial_x', C=40, nparts=2),
    _c(8, 16, 127, 129, 3, 4, 'odd_h odd_w partial_x partial_y'),
    # ---- MW = 2
    _c(17, 16, 4, 4, 3, 2, 'ragged_n', epi='pool'),
    _c(17, 16, 4, 4, 3, 2, 'ragged_n', act='tanh', epi='unpool', data='float'),
    _c(5, 16, 6, 6, 7, 2, 'ragged_n', act='relu', epi='unpool', transposed=True),
    _c(5, 16, 6, 6, 7, 2, 'ragged_n ragged_c used_lt_mt', epi='pool', C=24),
    _c(3, 16, 7, 9, 5, 2, 'odd_h odd_w', act='relu'),
    _c(3, 16, 1, 1, 3, 2, 'odd_h odd_w used_lt_mt'),
    _c(3, 16, 1, 1, 3, 2, 'odd_h odd_w used_lt_mt', data='float'),
    _c(9, 80, 3, 5, 3, 2, 'multi_kblock ragged_k ragged_c', C=24, act='relu'),
    _c(9, 80, 3, 5, 3, 2, 'multi_kblock ragged_k', C=512, nparts=2),
    _c(1, 16, 5, 34, 3, 2, 'partial_x partial_y', act='relu'),
    _c(2, 16, 1, 7, 5, 2, 'odd_h odd_w', C=48, nparts=4, transposed=True),
    # ---- the routes the shapes above leave open at one k: at k = 5 ragged N, several channel blocks with a ragged K and a ragged
    # last chunk, a raised pitch at MW = 4 and the cut of IMG at either MW; at k = 7 an odd H with a partial tile row
    _c(4100, 80, 4, 4, 5, 4, 'ragged_n multi_kblock ragged_k ragged_c', C=24),
    _c(2100, 16, 1, 29, 5, 4, 'pitch_raised odd_h odd_w', act='relu'),
    _c(17000, 16, 1, 1, 5, 4, 'img_capped_by_lds used_lt_mt ragged_n'),
    _c(33, 16, 1, 1, 5, 2, 'img_capped_by_lds used_lt_mt ragged_n', act='relu'),
    _c(5, 16, 6, 6, 5, 2, 'ragged_n pitch_raised', epi='unpool_sum'),
    _c(3, 16, 7, 9, 7, 2, 'odd_h odd_w partial_y', act='relu'),
]

# The smallest single-tile case: the first GPU run settles on it whether the MFMA sums exact integer products exactly.
FIRST_CASE = next(c for c in CASES if (c.N, c.H, c.W, c.k, c.data) == (3, 1, 1, 3, 'int'))

# A flag that no shape can raise at a given k, with the reason (asserted by enumeration in the CPU test).
IMPOSSIBLE = {
    (3, 'img_capped_by_lds'): 'at k = 3 every even tile of up to 256 pixels with its MT / (TH TW) images stages at most 32 KiB: '
                              'the 2 x 2 tile with 64 images of 4 x 4 patch pixels is exactly 32 KiB',
}


def case_id(c):
    return '%dx%dx%dx%dx%d-k%d-mw%d-p%d-%s-%s%s-%s' % (c.N, c.C, c.K, c.H, c.W, c.k, c.mw, c.nparts, c.act or 'none', c.epi,
                                                      '-T' if c.transposed else '', c.data)


def case_flags(c):
    return flags(c.N, c.C, c.K, c.H, c.W, c.k, c.nparts)


# ---- data ------------------------------------------------------------------------------------------------------------------

def _ri(g, lo, hi, *s):
    return torch.randint(lo, hi + 1, s, generator=g).float()


def _nonzero(t):
    """Zeros become +1 / -1 alternately: every weight counts, so a dropped or misplaced term always moves the sum."""
    flat = t.reshape(-1)
    alt = torch.ones_like(flat)
    alt[1::2] = -1
    return torch.where(flat == 0, alt, flat).view(t.shape)


def seam_images(N, IMG):
    """The first and last image of the tile groups at the start, in the middle and at the end of the batch, and the last real
    image (of a ragged group: its last member)."""
    groups = _ceil(N, IMG)
    out = set()
    for gi in sorted({0, 1, groups // 2, groups - 2, groups - 1}):
        if 0 <= gi < groups:
            out |= {gi * IMG, min(gi * IMG + IMG - 1, N - 1)}
    out.add(N - 1)
    return sorted(out)


def seam_channels(C, nparts):
    """Channel C - 1, and the first and the last channel of each part."""
    cp = C // nparts
    return sorted({C - 1} | {p * cp for p in range(nparts)} | {p * cp + cp - 1 for p in range(nparts)})


def seam_pixels(p, H, W):
    """[(image within its group, row, column)]: tile corners with the pixels on either side of every tile edge (first, a middle
    and last edge in each direction, and the plane's own corners), and the pixels lanes 0 and 63 of each wave own in tile (0, 0):
    row m = 16 f and 16 f + 15 of the tile's pixel list m = 4 q + 2 dy + dx."""
    def edges(n, T):
        cuts = sorted({1, n // T // 2, (n - 1) // T}) if n > T else []
        at = {0, n - 1}
        for c in cuts:
            if 0 < c * T < n:
                at |= {c * T - 1, c * T}
        return sorted(at)
    sites = [(0, r, c) for r in edges(H, p.TH) for c in edges(W, p.TW)]
    QW, QH = p.TW // 2, p.TH // 2
    for m in range(p.IMG * p.TH * p.TW):
        if m % 16 in (0, 15):
            q, sub = m >> 2, m & 3
            i, qy, qx = q // (QW * QH), (q // QW) % QH, q % QW
            r, c = 2 * qy + (sub >> 1), 2 * qx + (sub & 1)
            if r < H and c < W:
                sites.append((i, r, c))
    return list(dict.fromkeys(sites))


def outlier_sites(c):
    """[(n, channel, row, column)] in x, without repeats."""
    p = plan(c.N, c.K, c.H, c.W, c.k)
    chans = seam_channels(c.C, c.nparts)
    pixels = seam_pixels(p, c.H, c.W)
    sites, j = [], 0
    for n in seam_images(c.N, p.IMG):
        for (i, r, col) in pixels:
            if i == 0:                          # the tile seams, in every seam image
                sites.append((n, chans[j % len(chans)], r, col))
                j += 1
    for g0 in sorted({0, (_ceil(c.N, p.IMG) - 1) * p.IMG}):      # the lane seams: the first and the last group's tile (0, 0)
        for (i, r, col) in pixels:
            if g0 + i < c.N:
                sites.append((g0 + i, chans[j % len(chans)], r, col))
                j += 1
    seen, out = set(), []
    for s in sites:
        if (s[0], s[2], s[3]) not in seen:
            seen.add((s[0], s[2], s[3]))
            out.append(s)
    return out


def _wshape(c):
    return (c.C, c.K, c.k, c.k) if c.transposed else (c.K, c.C, c.k, c.k)


def int_case(c, seed=1, outliers=True):
    """(x [N, C, H, W], w, bias [K], addx [N, K, H/2, W/2] or None) as integers in fp32."""
    g = torch.Generator().manual_seed(seed)
    x = _ri(g, -4, 4, c.N, c.C, c.H, c.W)
    w = _nonzero(_ri(g, -3, 3, *_wshape(c)))
    b = _ri(g, -8, 8, c.K)
    addx = _ri(g, -8, 8, c.N, c.K, c.H // 2, c.W // 2) if c.epi.startswith('unpool') else None
    if outliers:
        s = outlier_sites(c)
        idx = torch.tensor(s, dtype=torch.long).t()
        sign = torch.ones(len(s))
        sign[1::2] = -1
        x[idx[0], idx[1], idx[2], idx[3]] = OUTLIER * sign
    return x, w, b, addx


def float_case(c, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(c.N, c.C, c.H, c.W, generator=g)
    w = torch.randn(*_wshape(c), generator=g) / np.sqrt(c.C * c.k * c.k)
    b = torch.randn(c.K, generator=g) * 0.1
    addx = torch.randn(c.N, c.K, c.H // 2, c.W // 2, generator=g) if c.epi.startswith('unpool') else None
    return x, w, b, addx


def case_data(c, seed=1):
    return int_case(c, seed) if c.data == 'int' else float_case(c, seed)


# ---- the reference ---------------------------------------------------------------------------------------------------------

def conv64(x, w, b, transposed, dtype=torch.float64, rounded=True):
    """Bias + the stride-1, padding k / 2 convolution of the bf16-rounded operands in `dtype`, N at a time in slices that keep the
    unfolded image small."""
    k = w.shape[2]
    xr = (bf16_round(x) if rounded else x).to(dtype)
    wr = (bf16_round(w) if rounded else w).to(dtype)
    fn = F.conv_transpose2d if transposed else F.conv2d
    per = max(1, (1 << 25) // max(1, x.shape[1] * k * k * x.shape[2] * x.shape[3]))
    return torch.cat([fn(xr[i:i + per], wr, b.to(dtype), padding=k // 2) for i in range(0, x.shape[0], per)], 0)


def activate(y, act):
    return torch.relu(y) if act == 'relu' else (torch.tanh(y) if act == 'tanh' else y)


def reference(c, x, w, b, addx):
    """{'y': act(conv + bias), 'pool': its 2 x 2 max pool, 'sum': y + fixed_unpool(addx)} in float64, each where the case's
    epilogue produces it."""
    y = activate(conv64(x, w, b, c.transposed), c.act)
    out = {'y': y}
    if c.epi == 'pool':
        out['pool'] = F.max_pool2d(y, 2)
    if c.epi.startswith('unpool'):
        s = y.clone()
        s[:, :, 0::2, 0::2] += addx.double()
        out['sum'] = s
    return out


def pack_layout(w, K, C, k, transposed):
    """The documented layout of tai_conv_bf16_pack_weights as uint16 bf16 bits: Wp[kb][chunk][s][j][lane][e] = w_conv[o][c][t / k][t % k]
    with o = 64 kb + 16 j + (lane & 15), t = 2 s + (lane >> 5), c = 16 chunk + 8 ((lane >> 4) & 1) + e; zero past K, C or k^2.
    transposed: w is [C][K][k][k] and w_conv[o][c][ky][kx] = w[c][o][k - 1 - ky][k - 1 - kx]."""
    wc = w.permute(1, 0, 2, 3).flip(2, 3) if transposed else w
    bits = (bf16_round(wc.contiguous()).float().numpy().view(np.uint32) >> 16).astype(np.uint16).reshape(K, C, k * k)
    kblocks, nchunks, S = _ceil(K, NT), _ceil(C, KC), ksteps(k)
    full = np.zeros((kblocks * NT, nchunks * KC, 2 * S), dtype=np.uint16)
    full[:K, :C, :k * k] = bits
    out = np.zeros((kblocks, nchunks, S, 4, 64, 8), dtype=np.uint16)
    for lane in range(64):
        for e in range(8):
            cl = 8 * ((lane >> 4) & 1) + e
            for j in range(4):
                # [kb, chunk, s]
                o = np.arange(kblocks) * NT + 16 * j + (lane & 15)
                cc = np.arange(nchunks) * KC + cl
                t = 2 * np.arange(S) + (lane >> 5)
                out[:, :, :, j, lane, e] = full[o[:, None, None], cc[None, :, None], t[None, None, :]]
    return out.reshape(-1)


def tie_values():
    """fp32 values around every bf16 rounding tie of the binades 2^-24 .. 2^24: (1 + (2 j + 1) 2^-8) 2^e for j = 0 .. 127, the fp32
    value one ulp below and the one above, both signs.  A tie rounds to the even bf16 neighbour, its fp32 neighbours to
    either side: truncation, round-half-up and round-half-away all differ from nearest-even somewhere here."""
    j = np.arange(128, dtype=np.uint32)
    vals = []
    for e in range(-24, 25):
        tie = ((np.uint32(127 + e) << np.uint32(23)) | (j << np.uint32(16)) | np.uint32(0x8000)).astype(np.uint32)
        vals += [tie, tie - np.uint32(1), tie + np.uint32(1)]
    bits = np.concatenate(vals)
    bits = np.concatenate([bits, bits | np.uint32(0x80000000)])
    return torch.from_numpy(bits.view(np.float32).copy())
