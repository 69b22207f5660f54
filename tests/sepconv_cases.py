"""Case generators for the separable convolution's backward tests (tests/test_gpu_sepconv_backward.py; their conditions
are checked without a GPU in tests/test_sepconv_cases_cpu.py).

Two kinds of data:
  * ``int_case``: small integers stored in fp32, with a few outliers of +-OUTLIER on the tile seams and the image corners.
    Every partial sum of every gradient is then an integer below 2^24, so ANY fp32 summation order -- fused or not, atomics
    included -- gives exactly the oracle's value: the comparison is torch.equal, and one missing, doubled or misplaced term
    fails it.  The cap is asserted, per shape, on the absolute values of the operands (test_sepconv_cases_cpu.py).
  * ``float_case``: tests/test_gpu_sepconv.py's generator (tanh-range image, taps N(0, 0.1)), compared within its BWD_TOL.

The tiling constants restate csrc/sepconv_fwd.hip.inc / sepconv_bwd.hip.inc; the CPU test reads them back from the sources.
"""
import torch

TILE_W = 128            # fwd::TILE_W: columns of every tile
GV_TILE_H = 8           # rows of a gV / gH tile (sepconv_grad_vh_ab, sepconv_grad_[vh]_tiled)
GI_R = 10               # gi2::R: source rows of a gI strips tile
GI_SLAB = 60 * 180      # gi2::SLAB = (R + ks - 1) rows x SPITCH floats per tile and channel
OUTLIER = 512.0
CAP = float(2 ** 24)

# (B, C, H, W, ks)
AB_SHAPES = [                   # C = 1: sepconv_grad_vh_ab and the gI strips
    (2, 1, 8, 128, 51),         # one exact tile
    (1, 1, 7, 124, 51),         # one tile, ragged both ways
    (1, 1, 9, 132, 51),         # H % 8 = 1, a four-column last tile
    (2, 1, 17, 260, 51),        # three column tiles x three row tiles, ragged, B > 1
    (1, 1, 10, 128, 51),        # gI's 10-row tile exact ...
    (1, 1, 11, 128, 51),        # ... one row over ...
    (1, 1, 21, 128, 51),        # ... and three tiles, the last of one row
]
C3_SHAPES = [                   # sepconv_grad_[vh]_tiled<51, 3>
    (1, 3, 9, 132, 51),         # two column tiles; gI's slabs do not fit (64,800 against 60,588): atomics
    (2, 3, 17, 260, 51),        # 3 x 3 tiles, ragged; the slabs fit
]
SLAB_SHAPES = [                 # either side of "the tile slabs fit the borrowed tap-gradient buffer"
    (1, 1, 2, 108, 51),         # fits: 11,016 >= 10,800
    (1, 1, 2, 104, 51),         # does not: 10,608
    (1, 3, 5, 128, 51),         # fits: 32,640 >= 32,400
    (1, 3, 5, 124, 51),         # does not: 31,620
    (1, 3, 11, 132, 51),        # four tiles, does not fit: the atomic flush runs across tile seams
]
TILEABLE_SHAPES = AB_SHAPES + C3_SHAPES + SLAB_SHAPES
GENERIC_SHAPES = [
    (1, 4, 5, 8, 51),           # the gather's 3 + 1 channel split
    (1, 5, 3, 6, 51),           # 3 + 1 + 1
    (1, 1, 6, 10, 51),          # W % 4 != 0
    (1, 2, 5, 9, 7),
    (1, 1, 4, 6, 1),
]
ALL_SHAPES = TILEABLE_SHAPES + GENERIC_SHAPES
SUBSET_SHAPES = [(1, 1, 9, 132, 51), (1, 3, 9, 132, 51), (1, 1, 2, 108, 51), (1, 4, 5, 8, 51)]
BAND_SHAPES = SLAB_SHAPES[:4] + [(1, 1, 9, 132, 51)]
REPEAT_SHAPES = [(2, 1, 17, 260, 51), (2, 3, 17, 260, 51)]
SUBSETS = [(True, True, True), (True, True, False), (True, False, True), (False, True, True),
           (True, False, False), (False, True, False), (False, False, True)]       # (gI, gV, gH)


def shape_id(s):
    return 'x'.join(str(d) for d in s[:4]) + '-ks%d' % s[4]


def tileable(C, W, ks):
    """tai_sepconv_backward's own condition for the tiled kernels."""
    return ks == 51 and W % 4 == 0 and C in (1, 3)


def slab_floats(B, C, H, W):
    """Floats of tile slabs the gI strips kernel writes for this shape."""
    tiles_x, tiles_y = (W + TILE_W - 1) // TILE_W, (H + GI_R - 1) // GI_R
    return B * tiles_x * tiles_y * C * GI_SLAB


def slabs_fit(B, C, H, W, ks):
    """The slabs fit a tap-gradient buffer of B * ks * H * W floats (the launcher then borrows it; else: atomics)."""
    return slab_floats(B, C, H, W) <= B * ks * H * W


def outlier_sites(B, C, H, W, ks):
    """[(b, c, row, col)] for gO and for input: rows 0, 7/8 (the gV / gH tile seam), 9/10 (gI's) and H-1 x columns 0, 127/128
    and W-1, those that exist; for the input also its last padded row and column.  Each site carries its outlier in ONE sample
    and ONE channel, cycling, so a row or column of the input holds only a few in the channel a gO outlier multiplies."""
    Hp, Wp = H + ks - 1, W + ks - 1
    pick = lambda idx, n: sorted({i for i in idx if 0 <= i < n})
    rows, cols = pick((0, 7, 8, 9, 10, H - 1), H), pick((0, 127, 128, W - 1), W)
    irows, icols = pick((0, 7, 8, 9, 10, H - 1, Hp - 1), Hp), pick((0, 127, 128, W - 1, Wp - 1), Wp)
    g_sites = [(k % B, k % C, r, c) for k, (r, c) in enumerate((r, c) for r in rows for c in cols)]
    i_sites = [(k % B, k % C, r, c) for k, (r, c) in enumerate((r, c) for r in irows for c in icols)]
    return g_sites, i_sites


def int_case(B, C, H, W, ks, seed, outliers=True):
    """(input, v, h, gO): integers in fp32 -- input in [-4, 4], gO in [-3, 3], taps in [-2, 2] -- plus the outliers."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    inp = ri(-4, 4, B, C, H + ks - 1, W + ks - 1)
    v = ri(-2, 2, B, ks, H, W)
    h = ri(-2, 2, B, ks, H, W)
    gO = ri(-3, 3, B, C, H, W)
    if outliers:
        g_sites, i_sites = outlier_sites(B, C, H, W, ks)
        for k, (b, c, r, col) in enumerate(g_sites):
            gO[b, c, r, col] = OUTLIER if k % 2 == 0 else -OUTLIER
            # the taps at an outlier's pixel are never zero: the outlier reaches every gradient it belongs to
            v[b, :, r, col] = torch.where(v[b, :, r, col] == 0, torch.ones(()), v[b, :, r, col])
            h[b, :, r, col] = torch.where(h[b, :, r, col] == 0, -torch.ones(()), h[b, :, r, col])
        for k, (b, c, r, col) in enumerate(i_sites):
            inp[b, c, r, col] = -OUTLIER if k % 3 == 0 else OUTLIER
    return inp, v, h, gO


def float_case(B, C, H, W, ks, seed):
    """tests/test_gpu_sepconv.py's _case: tanh-range image, taps N(0, 0.1), gO N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    inp = torch.rand(B, C, H + ks - 1, W + ks - 1, generator=g) * 2 - 1
    v = torch.randn(B, ks, H, W, generator=g) * 0.1
    h = torch.randn(B, ks, H, W, generator=g) * 0.1
    gO = torch.randn(B, C, H, W, generator=g)
    return inp, v, h, gO
