"""Host side of the F(4x4, 3x3) forward's split over input channels (tai_conv3x3_wino43_splits / _workspace_floats, conv_ops._wino43_ok):
which layers split, into how many runs of chunks, and where the runs break.  No GPU: the plan is host code."""
import ctypes

import pytest


def _lib():
    from video_frame_inpainting_amd import _native
    return _native.lib()


def _plan(N, C, K, H, W, nparts=1):
    cps = ctypes.c_int(-1)
    S = _lib().tai_conv3x3_wino43_splits(N, C, K, H, W, nparts, ctypes.byref(cps))
    return S, cps.value


def _groups(N, K, H, W):
    return ((N * (H // 4) * (W // 4) + 31) // 32) * ((K + 63) // 64)


SMALL = [(160, 512, 512, 4, 4, 1), (160, 512, 512, 8, 8, 1), (64, 256, 128, 16, 16, 1), (64, 128, 256, 16, 16, 1),
         (32, 128, 128, 32, 32, 1), (64, 512, 256, 16, 16, 2), (32, 512, 128, 32, 32, 2), (160, 256, 256, 8, 8, 1),
         (160, 512, 256, 8, 8, 1), (160, 512, 51, 8, 8, 1)]
LARGE = [(64, 256, 256, 32, 32, 1), (32, 64, 64, 128, 128, 1), (160, 64, 64, 64, 64, 1), (64, 512, 1024, 16, 16, 2)]


@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'x'.join(map(str, s)))
def test_small_grids_split_into_fuller_rounds(shape):
    N, C, K, H, W, nparts = shape
    S, cps = _plan(*shape)
    nchunks = (C + 3) // 4
    g = _groups(N, K, H, W)
    assert S > 1 and g < 256
    # the runs cover every chunk once, none empty, each at least 8 chunks (the floor), at most 16 splits
    assert (S - 1) * cps < nchunks <= S * cps and cps >= 8 and S <= 16
    # more of the chip per round: the last round of the split grid is fuller than the unsplit grid's only round
    assert (g * S) % 256 == 0 or (g * S) % 256 > g
    assert _lib().tai_conv3x3_wino43_workspace_floats(*shape) == S * N * K * H * W


def test_whole_rounds_where_the_chunks_allow():
    # 40 and 80 workgroups: 6 and 3 splits are exactly 240 workgroups -- one round of 256 CUs with 16 idle
    assert _plan(160, 512, 512, 4, 4) == (6, 22)
    assert _plan(160, 256, 256, 8, 8)[0] * _groups(160, 256, 8, 8) == 240
    # 64 / 128 workgroups: 4 / 2 splits fill one round exactly
    assert _plan(64, 256, 128, 16, 16)[0] * _groups(64, 128, 16, 16) == 256
    assert _plan(64, 128, 256, 16, 16)[0] * _groups(64, 256, 16, 16) == 256


@pytest.mark.parametrize('shape', LARGE, ids=lambda s: 'x'.join(map(str, s)))
def test_large_grids_keep_one_split(shape):
    assert _plan(*shape)[0] == 1
    assert _lib().tai_conv3x3_wino43_workspace_floats(*shape) == 0


def test_chunk_floor():
    # 32 input channels = 8 chunks: two runs of 4 would break the floor
    assert _plan(64, 32, 64, 8, 8)[0] == 1
    S, cps = _plan(160, 512, 51, 8, 8)     # 20 workgroups: as many splits as the floor allows a fuller chip
    assert cps >= 8 and S * cps >= 128


@pytest.mark.parametrize('shape', [(64, 512, 256, 16, 16, 2), (32, 512, 128, 32, 32, 2), (64, 512, 256, 16, 16, 4),
                                   (40, 768, 256, 8, 8, 3), (64, 384, 64, 8, 8, 3)], ids=lambda s: 'x'.join(map(str, s)))
def test_splits_break_on_part_boundaries(shape):
    N, C, K, H, W, nparts = shape
    S, cps = _plan(*shape)
    cpp = C // nparts // 4
    assert cpp % cps == 0 or cps % cpp == 0, (S, cps, cpp)
    bounds = set(range(0, (C + 3) // 4, cps))
    assert set(range(0, (C + 3) // 4, cpp)) <= bounds or cps % cpp == 0


def test_switch_and_argument_checks():
    L = _lib()
    assert L.tai_conv3x3_wino43_set_splitc(0) == 1
    try:
        assert _plan(160, 512, 512, 8, 8) == (1, 128)
        assert L.tai_conv3x3_wino43_workspace_floats(160, 512, 512, 8, 8, 1) == 0
    finally:
        assert L.tai_conv3x3_wino43_set_splitc(1) == 0
    assert _plan(160, 512, 512, 8, 8)[0] > 1
    assert _plan(64, 512, 256, 16, 18)[0] == 1          # W % 4: not an F(4x4) layer
    assert _plan(64, 510, 256, 16, 16, 2)[0] == 1       # parts whose channels are no multiple of 4


def test_dispatch_counts_workgroups_after_the_split_outside_the_recurrence():
    import torch
    from video_frame_inpainting_amd import conv_ops
    # MC-Net's own layers below the threshold keep F(2x2, 3x3)
    assert not conv_ops._wino43_ok(64, 512, 256, 16, 16, nparts=2)
    assert not conv_ops._wino43_ok(160, 512, 512, 4, 4)
    # a layer outside the recurrence: 64 workgroups x 4 splits = 256 >= WINO43_MIN_WORKGROUPS
    conv = torch.nn.Conv2d(256, 128, 3, padding=1)
    conv_ops.mark_outside_recurrence(conv)
    assert _groups(64, 128, 16, 16) < conv_ops.WINO43_MIN_WORKGROUPS
    assert conv_ops._wino43_ok(64, 256, 128, 16, 16, 1, conv.weight)
    L = _lib()
    L.tai_conv3x3_wino43_set_splitc(0)
    try:
        assert not conv_ops._wino43_ok(64, 256, 128, 16, 16, 1, conv.weight)
    finally:
        L.tai_conv3x3_wino43_set_splitc(1)
