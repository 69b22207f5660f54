"""Case generators for the separable convolution's kernel-level tests, both directions: the gradients
(tests/test_gpu_sepconv_backward.py) and the forward (tests/test_gpu_sepconv_forward.py, the FWD_* lists and fwd_* functions
at the end of this file).  Their conditions are checked without a GPU in tests/test_sepconv_cases_cpu.py.

Two kinds of data:
  * ``int_case``: small integers stored in fp32, with a few outliers of +-OUTLIER on the tile seams and the image corners.
    Every partial sum of every gradient is then an integer below 2^24, so ANY fp32 summation order -- fused or not, atomics
    included -- gives exactly the oracle's value: the comparison is torch.equal, and one missing, doubled or misplaced term
    fails it.  The cap is asserted, per shape, on the absolute values of the operands (test_sepconv_cases_cpu.py).
  * ``float_case``: tests/test_gpu_sepconv.py's generator (tanh-range image, taps N(0, 0.1)), compared within its BWD_TOL.

The tiling constants restate csrc/sepconv_fwd.hip.inc / sepconv_bwd.hip.inc, the forward route predicates restate
csrc/capi_sepconv.inc's persistent_policy; the CPU test reads them back from the sources.
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


# ---- the forward ----------------------------------------------------------------------------------------------------------

FWD_TILE_H = 16         # rows of a tile of the 8-wave kernels (7-14, 16-27)
FWD_TILE_H_SMALL = 8    # rows of a tile of the 4-wave kernels (2-6, 15)
PATCH_ROWS = 66         # PR = FWD_TILE_H + 51 - 1: rows of the input patch of a 16-row tile
PATCH_PITCH = 180       # floats per patch row in LDS: 128 + 50 columns, rounded up to whole 16-byte chunks
PATCH_CHUNKS = 45       # stage_patch_dma's CH: 16-byte chunks per patch row
PERSISTENT_ROUNDS = 3   # tiles per workgroup the persistent cases ask for: both patch buffers are used a second time

# (H, W) of single-channel planes for the persistent kernel; B comes from the CU count of the device (fwd_persistent_shape)
FWD_PERSISTENT_PLANES = [
    (20, 132),          # a 4-column last column tile, a 4-row last row tile
    (40, 320),          # a 64-column last column tile: a published frame width
    (26, 208),          # an 80-column last column tile: the other published width
    (17, 128),          # a one-row last row tile at full width: the control
]
FWD_C3_SHAPES = [               # the colour route (kernels 19 / 17 and what they leave to kernel 16)
    (1, 3, 17, 132, 51),        # C = 3 on two column tiles, ragged rows
    (2, 3, 33, 260, 51),        # C = 3 on 3 x 3 tiles
    (1, 3, 31, 320, 51),        # C = 3 at the published width
    (2, 2, 9, 132, 51),         # no three-channel launch: kernel 16 twice
    (1, 4, 17, 132, 51),        # 3 + 1 channels
    (1, 5, 9, 260, 51),         # 3 + 2 channels
    (1, 6, 20, 132, 51),        # two three-channel launches, c0 = 3
    (2, 7, 5, 4, 51),           # 3 + 3 + 1 channels on a one-lane tile
]
FWD_SMALL_SHAPES = [
    (8, 1, 1, 4, 51),           # one row, one lane
    (1, 1, 9, 132, 51),         # H % 8 = 1 for the 8-row kernels
    (1, 1, 16, 124, 51),        # a narrow single tile
    (1, 1, 6, 10, 51),          # generic kernel: W % 4 != 0
    (1, 2, 5, 9, 7),            # generic kernel, other ks
    (1, 1, 4, 6, 1),            # generic kernel, ks 1
]
FWD_FIXED_SHAPES = FWD_C3_SHAPES + FWD_SMALL_SHAPES
FWD_VARIANTS = tuple(range(28))                     # 0 = automatic, 1-27 as include/tai_sepconv.h lists them
FWD_PERSISTENT_VARIANTS = (20, 21, 22, 23, 24, 25, 26, 27)
MIXED_WAVE_SHAPES = [(2, 40, 256), (1, 16, 132), (3, 16, 128), (1, 24, 4)]      # (B, H, W) test_gpu_sepconv.py asks variant 20 for


def fwd_tileable(W, ks):
    """tai_sepconv_forward's own condition for every variant but the generic kernel (any C)."""
    return ks == 51 and W % 4 == 0


def fwd_tiles(B, H, W):
    """Tiles of the 16-row kernels: what fwd_persistent counts."""
    return B * ((W + TILE_W - 1) // TILE_W) * ((H + FWD_TILE_H - 1) // FWD_TILE_H)


def fwd_persistent_runs(B, H, W, cus, forced=False):
    """csrc/capi_sepconv.inc's persistent_policy at C = 1: a multiple of 8 tiles, more tiles than workgroups unless the variant
    was asked for by number, tap offsets that fit 32 bits, a device of at least 8 CUs."""
    ntiles, grid = fwd_tiles(B, H, W), cus // 8 * 8
    return grid >= 8 and ntiles % 8 == 0 and (forced or ntiles > grid) and B * 51 * H * W * 4 <= 0xffffffff


def fwd_rounds(B, H, W, cus):
    """(largest, smallest) number of tiles a workgroup of the persistent kernel walks: workgroup (xcd, slot) takes the tiles
    slot, slot + slots, ... below per_xcd of its XCD's eighth of the list."""
    ntiles = fwd_tiles(B, H, W)
    grid = min(cus // 8 * 8, ntiles)
    per_xcd, slots = ntiles // 8, grid // 8
    walked = [len(range(slot, per_xcd, slots)) for slot in range(slots)]
    return max(walked), min(walked)


def persistent_batch(H, W, cus, rounds):
    """The smallest B for which the tile count is a multiple of 8 and at least one workgroup walks `rounds` tiles."""
    B = 1
    while not (fwd_tiles(B, H, W) % 8 == 0 and fwd_rounds(B, H, W, cus)[0] >= rounds):
        B += 1
    return B


def fwd_persistent_shape(plane, cus):
    H, W = plane
    return (persistent_batch(H, W, cus, PERSISTENT_ROUNDS), 1, H, W, 51)


def fwd_fallback_shapes(plane, cus):
    """The same plane with B chosen to break one condition of the persistent route each -> {name: shape}:
    'ragged': more tiles than workgroups, but no multiple of 8 of them (kernel 18 whatever was asked for);
    'few': a multiple of 8 tiles, at most one per workgroup (kernel 18 on the automatic route; persistent, one tile per
    workgroup, when asked for by number)."""
    H, W = plane
    grid = cus // 8 * 8
    ragged = next(B for B in range(1, 1 << 20) if fwd_tiles(B, H, W) > grid and fwd_tiles(B, H, W) % 8 != 0)
    few = next(B for B in range(1, 1 << 20) if fwd_tiles(B, H, W) % 8 == 0)
    return {'ragged': (ragged, 1, H, W, 51), 'few': (few, 1, H, W, 51)}


def fwd_all_shapes(cus):
    """Every forward shape on a device of `cus` compute units."""
    derived = [fwd_persistent_shape(p, cus) for p in FWD_PERSISTENT_PLANES]
    for p in FWD_PERSISTENT_PLANES:
        derived += list(fwd_fallback_shapes(p, cus).values())
    return FWD_FIXED_SHAPES + derived


def fwd_outlier_sites(B, C, H, W, ks):
    """[(b, c, row, col)] of the padded input: the forward's seams.  Rows 0, 15/16 (the row-tile seam), 65/66 (the last patch row
    of the first row tile and the first row only the second tile reads), H-1, and the last two padded rows; columns 0, 127/128,
    177/178 (the last patch column of the first column tile and the first only the second reads), W-1, and the last two padded
    columns (the pair stage_patch_dma writes separately) -- those that exist.  One sample and one channel per site, cycling."""
    Hp, Wp = H + ks - 1, W + ks - 1
    pick = lambda idx, n: sorted({i for i in idx if 0 <= i < n})
    rows = pick((0, 15, 16, 65, 66, H - 1, Hp - 2, Hp - 1), Hp)
    cols = pick((0, 127, 128, 177, 178, W - 1, Wp - 2, Wp - 1), Wp)
    return [(k % B, k % C, r, c) for k, (r, c) in enumerate((r, c) for r in rows for c in cols)]


def fwd_readers(site, H, W, ks):
    """(rows, columns) of the output pixels whose window holds the input element of `site`, as slices."""
    _, _, r, col = site
    return slice(max(0, r - ks + 1), min(H - 1, r) + 1), slice(max(0, col - ks + 1), min(W - 1, col) + 1)


def fwd_int_case(B, C, H, W, ks, seed, outliers=True):
    """(input, v, h): integers in fp32 -- input in [-4, 4], taps in [-2, 2] -- plus +-OUTLIER at fwd_outlier_sites.  The taps of
    every output pixel that reads an outlier are never zero: the outlier reaches every output it belongs to."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    inp = ri(-4, 4, B, C, H + ks - 1, W + ks - 1)
    v = ri(-2, 2, B, ks, H, W)
    h = ri(-2, 2, B, ks, H, W)
    if outliers:
        reads = torch.zeros(B, 1, H, W, dtype=torch.bool)
        for k, site in enumerate(fwd_outlier_sites(B, C, H, W, ks)):
            b, c, r, col = site
            inp[b, c, r, col] = -OUTLIER if k % 3 == 0 else OUTLIER
            ys, xs = fwd_readers(site, H, W, ks)
            reads[b, 0, ys, xs] = True
        v = torch.where(reads & (v == 0), torch.ones(()), v)
        h = torch.where(reads & (h == 0), -torch.ones(()), h)
    return inp, v, h
