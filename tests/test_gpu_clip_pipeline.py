"""The clip pipeline's kernels (csrc/clip_pipeline.hip.inc) against the host path of this repository -- data._ClipReader.clip on the way
in, util.frames_to_uint8 on the way out.  Tolerance: zero (torch.equal / np.array_equal) throughout."""

import numpy as np
import pytest
import torch

from video_frame_inpainting_amd import _native, clip_pipeline
from video_frame_inpainting_amd.data import _ArrayVideo, _ClipReader
from video_frame_inpainting_amd.util import bgr2gray, fore_transform, frames_to_uint8

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
EINVAL = -1


def _frames(rng, t, h, w):
    return rng.randint(0, 256, (t, h, w, 3), dtype=np.uint8)


def host_clip(frames, c_dim, size, pad, mirror, reverse):
    """The host path itself: _ClipReader.clip on a source that holds exactly these frames."""
    return _ClipReader(c_dim, size, pad).clip(_ArrayVideo(frames, 'test'), range(frames.shape[0]), mirror, reverse)


def raw_item(frames, mirror, reverse):
    """What a raw-mode dataset hands over for the same clip (data._ClipReader.raw_clip)."""
    f = _ClipReader(1, None, None).raw_clip(_ArrayVideo(frames, 'test'), range(frames.shape[0]), reverse)
    return {'frames': f, 'mirror': mirror, 'clip_label': 'test'}


def device_clips(items, c_dim, size, pad, builder=None):
    builder = builder or clip_pipeline.DeviceClipBuilder(c_dim, size, pad, DEV)
    return builder.build(clip_pipeline.collate_raw(items))


# (source h, w) -> (output H, W), padding
CASES = [((120, 160), (128, 128), (0, 0)),
         ((240, 320), (240, 320), (16, 0)),
         ((240, 320), (128, 128), (0, 0)),
         ((480, 640), (128, 128), (0, 0)),
         ((48, 64), (128, 128), (0, 0)),
         ((37, 53), (15, 20), (1, 3)),
         ((1, 1), (8, 8), (0, 0)),
         ((128, 128), (128, 128), (0, 0))]


@pytest.mark.parametrize('c_dim', [1, 3])
@pytest.mark.parametrize('src,size,pad', CASES, ids=['%dx%d-%dx%d' % (c[0] + c[1]) for c in CASES])
def test_way_in_equals_the_host_clip(src, size, pad, c_dim):
    rng = np.random.RandomState(src[0] * 7 + size[1] + c_dim)
    frames = _frames(rng, 3, *src)
    builder = clip_pipeline.DeviceClipBuilder(c_dim, size, pad, DEV)
    for mirror in (False, True):
        for reverse in (False, True):
            want = host_clip(frames, c_dim, list(size), list(pad), mirror, reverse)
            got = device_clips([raw_item(frames, mirror, reverse)], c_dim, size, pad, builder)
            assert tuple(got.shape) == (1, 3, c_dim, size[0] + pad[0], size[1] + pad[1]) and got.dtype == torch.float32
            assert torch.equal(got[0].cpu(), want), (src, size, pad, c_dim, mirror, reverse)


def test_padding_values():
    # the pad is uint8 0: -1.0 in colour; in gray 0.9999 x -1 summed in fp32, -0.99990004 and not -1
    frames = _frames(np.random.RandomState(0), 1, 9, 9)
    t = clip_pipeline.level_tables()
    gray = ((t[1, 0] + t[2, 0]) + t[3, 0]).item()
    assert abs(gray + 0.99990004) < 1e-7 and gray != -1.0
    for c_dim, value in ((3, -1.0), (1, gray)):
        got = device_clips([raw_item(frames, False, False)], c_dim, (8, 8), (2, 4)).cpu()
        assert torch.equal(got, host_clip(frames, c_dim, [8, 8], [2, 4], False, False)[None])
        assert (got[..., 8:, :] == value).all() and (got[..., :, 8:] == value).all()


@pytest.mark.parametrize('c_dim', [1, 3])
def test_all_256_levels_in_every_channel(c_dim):
    # an identity-size frame [3 * 256, 4]: row block c ramps channel c over all levels, the other two channels hold other ramps
    k = np.arange(256, dtype=np.uint8)
    frame = np.zeros((768, 4, 3), dtype=np.uint8)
    for c in range(3):
        frame[c * 256:(c + 1) * 256, :, c] = k[:, None]
        frame[c * 256:(c + 1) * 256, :, (c + 1) % 3] = k[::-1, None]
        frame[c * 256:(c + 1) * 256, :, (c + 2) % 3] = ((k.astype(np.int64) * 37 + 11) % 256).astype(np.uint8)[:, None]
    frames = frame[None]
    want = host_clip(frames, c_dim, [768, 4], [0, 0], False, False)
    got = device_clips([raw_item(frames, False, False)], c_dim, (768, 4), (0, 0))
    assert torch.equal(got[0].cpu(), want)
    if c_dim == 3:      # every level met the range map, in every output channel
        for c in range(3):
            assert torch.unique(got[0, 0, c]).numel() == 256


def test_gray_of_200000_random_triples():
    rng = np.random.RandomState(77)
    frames = rng.randint(0, 256, (1, 400, 500, 3), dtype=np.uint8)           # 200,000 (R, G, B) triples, identity size
    want = host_clip(frames, 1, [400, 500], [0, 0], False, False)
    got = device_clips([raw_item(frames, False, False)], 1, (400, 500), (0, 0))
    assert torch.equal(got[0].cpu(), want)
    # and the restatement the kernel's tables stand for
    bgr = fore_transform(torch.from_numpy(np.ascontiguousarray(frames[0, :, :, ::-1])).permute(2, 0, 1).float().div(255))
    assert torch.equal(want[0], bgr2gray(bgr[None])[0])


@pytest.mark.parametrize('c_dim', [1, 3])
def test_ragged_batch_equals_per_clip_results_and_is_reproducible(c_dim):
    rng = np.random.RandomState(3)
    size, pad = (32, 48), (4, 8)
    clips = [(_frames(rng, 4, 60, 80), True, False), (_frames(rng, 4, 17, 23), False, True), (_frames(rng, 4, 32, 48), True, True)]
    items = [raw_item(*c) for c in clips]
    builder = clip_pipeline.DeviceClipBuilder(c_dim, size, pad, DEV)
    together = device_clips(items, c_dim, size, pad, builder).cpu()
    for i, (frames, mirror, reverse) in enumerate(clips):
        assert torch.equal(together[i], host_clip(frames, c_dim, list(size), list(pad), mirror, reverse))
        alone = device_clips([items[i]], c_dim, size, pad, builder).cpu()          # batch independence
        assert torch.equal(alone[0], together[i])
    again = device_clips(items, c_dim, size, pad, builder).cpu()                   # the other staging slot, same bits
    assert torch.equal(again, together)
    direct = builder.build(clip_pipeline.collate_items(items)).cpu()               # packed straight into pinned staging
    assert torch.equal(direct, together)


def _step_values():
    """fp32 values a few ulp either side of every uint8 step of u(x) = trunc(255 * ((x + 1) / 2)), values outside [-1, 1]."""
    k = np.arange(0, 257, dtype=np.float64)
    centre = (k / 255.0 * 2.0 - 1.0).astype(np.float32)
    vals = [centre]
    up, down = centre.copy(), centre.copy()
    for _ in range(4):
        up = np.nextafter(up, np.float32(4)).astype(np.float32)
        down = np.nextafter(down, np.float32(-4)).astype(np.float32)
        vals += [up.copy(), down.copy()]
    vals.append(np.array([-7.5, -1.0000001, 1.0000001, 3.0, -0.0, 0.0, 1e-30, -1e-30, np.inf, -np.inf], dtype=np.float32))
    return np.concatenate(vals)


def host_uint8(x, h, w, rgb):
    u = frames_to_uint8(x.reshape((-1,) + tuple(x.shape[-3:])))[:, :h, :w]
    u = u[..., ::-1] if rgb else u
    return np.ascontiguousarray(u).reshape(tuple(x.shape[:-3]) + (h, w, x.shape[-3]))


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('shape,crop', [((2, 3, 33, 47), (33, 47)), ((2, 3, 33, 47), (30, 41)), ((1, 5, 144, 128), (128, 128)),
                                        ((4, 1, 7, 5), (1, 1))])
def test_way_out_equals_frames_to_uint8(C, shape, crop):
    B, T, Hs, Ws = shape
    rng = np.random.RandomState(Hs + C)
    n = B * T * C * Hs * Ws
    steps = _step_values()
    x = (rng.randn(n) * 0.8).astype(np.float32)                     # plain noise, part of it outside [-1, 1]
    x[:min(n, steps.size)] = steps[:min(n, steps.size)]
    x = torch.from_numpy(rng.permutation(x).reshape(B, T, C, Hs, Ws))
    for rgb in ((False, True) if C == 3 else (False,)):
        got = clip_pipeline.to_uint8_host(x.to(DEV), crop[0], crop[1], rgb)
        assert got.dtype == np.uint8 and got.shape == (B, T, crop[0], crop[1], C)
        assert np.array_equal(got, host_uint8(x, crop[0], crop[1], rgb))


def test_way_out_every_step_value_and_nan():
    steps = _step_values()
    x = torch.from_numpy(steps.copy()).view(1, 1, 1, -1)
    assert np.array_equal(clip_pipeline.to_uint8_host(x.to(DEV)), host_uint8(x, 1, steps.size, False))
    nan = torch.full((1, 1, 2, 2), float('nan'))
    assert (clip_pipeline.to_uint8_host(nan.to(DEV)) == 0).all()             # documented: NaN -> 0


def test_both_kernels_in_one_graph_replay_equals_eager():
    rng = np.random.RandomState(9)
    size, pad, c_dim, T = (32, 32), (0, 0), 3, 4
    L = _native.lib()
    levels = clip_pipeline.level_tables().to(DEV)

    def batch(seed):
        r = np.random.RandomState(seed)
        return clip_pipeline.collate_raw([raw_item(_frames(r, T, 40, 56), True, False), raw_item(_frames(r, T, 24, 24), False, True)])

    first, second = batch(1), batch(2)
    assert torch.equal(clip_pipeline.table_of(first), clip_pipeline.table_of(second))     # same geometry, new pixels
    n, head = 2 * T, clip_pipeline.header_bytes(2 * T)
    staged = first['packed'].to(DEV)
    clip = torch.empty(2, T, c_dim, 32, 32, device=DEV)
    consumed = torch.empty_like(clip)
    pixels = torch.empty(2, T, 32, 32, c_dim, dtype=torch.uint8, device=DEV)

    def run(stream):
        _native.check(L.tai_clip_from_frames(staged.data_ptr() + head, staged.numel() - head, staged.data_ptr(),
                                             first['packed'].data_ptr(), levels.data_ptr(), clip.data_ptr(), n, c_dim, 32, 32, 0, 0,
                                             stream), 'tai_clip_from_frames')
        torch.mul(clip, 0.5, out=consumed)                                        # the stand-in consumer
        clip_pipeline.frames_to_uint8_device(consumed, 32, 32, True, out=pixels)

    run(torch.cuda.current_stream().cuda_stream)                                   # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(torch.cuda.current_stream().cuda_stream)
    staged.copy_(second['packed'].to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    replayed_clip, replayed_pixels = clip.cpu().clone(), pixels.cpu().clone()
    eager = clip_pipeline.DeviceClipBuilder(c_dim, size, pad, DEV).build(second)
    assert torch.equal(replayed_clip, eager.cpu())
    assert torch.equal(replayed_pixels, clip_pipeline.frames_to_uint8_device(eager * 0.5, 32, 32, True).cpu())
    assert not torch.equal(replayed_clip, clip_pipeline.DeviceClipBuilder(c_dim, size, pad, DEV).build(first).cpu())


def test_bad_arguments_are_refused_on_the_host_side():
    L = _native.lib()
    err = lambda: L.tai_sepconv_last_error().decode()
    item = raw_item(_frames(np.random.RandomState(0), 2, 8, 8), False, False)
    packed = clip_pipeline.collate_raw([item])['packed']
    head = clip_pipeline.header_bytes(2)
    dev = packed.to(DEV)
    levels = clip_pipeline.level_tables().to(DEV)
    out = torch.full((2, 3, 8, 8), 5.0, device=DEV)
    s = torch.cuda.current_stream().cuda_stream

    def call(frames=None, nbytes=None, table=None, host=None, lv=None, o=None, N=2, c_dim=3, H=8, W=8):
        pick = lambda given, default: default if given is None else (None if given == 0 else given)
        return L.tai_clip_from_frames(pick(frames, dev.data_ptr() + head), packed.numel() - head if nbytes is None else nbytes,
                                      pick(table, dev.data_ptr()), pick(host, packed.data_ptr()), pick(lv, levels.data_ptr()),
                                      pick(o, out.data_ptr()), N, c_dim, H, W, 0, 0, s)

    for kwargs, text in (({'frames': 0}, 'null'), ({'table': 0}, 'null'), ({'host': 0}, 'null'), ({'lv': 0}, 'null'), ({'o': 0}, 'null'),
                         ({'c_dim': 2}, 'c_dim'), ({'H': 0}, '> 0'), ({'W': 0}, '> 0'), ({'N': 0}, '> 0'),
                         ({'nbytes': 8 * 8 * 3 * 2 - 1}, 'past the stated length')):
        assert call(**kwargs) == EINVAL, kwargs
        assert text in err(), (kwargs, err())
    bad = packed.clone()
    clip_pipeline.table_of({'packed': bad, 'B': 1, 'T': 2})[1, 0] = 8 * 8 * 3 + 1          # second frame one byte too far
    assert call(host=bad.data_ptr()) == EINVAL and 'past the stated length' in err()
    clip_pipeline.table_of({'packed': bad, 'B': 1, 'T': 2})[1, 0] = -1
    assert call(host=bad.data_ptr()) == EINVAL
    x = torch.zeros(2, 3, 8, 8, device=DEV)
    u = torch.full((2, 8, 8, 3), 9, dtype=torch.uint8, device=DEV)
    for args, text in (((None, u.data_ptr(), 2, 3, 8, 8, 8, 8), 'null'), ((x.data_ptr(), None, 2, 3, 8, 8, 8, 8), 'null'),
                       ((x.data_ptr(), u.data_ptr(), 2, 2, 8, 8, 8, 8), 'C must be'), ((x.data_ptr(), u.data_ptr(), 2, 3, 8, 8, 0, 8), 'needs'),
                       ((x.data_ptr(), u.data_ptr(), 2, 3, 8, 8, 8, 9), 'needs'), ((x.data_ptr(), u.data_ptr(), 0, 3, 8, 8, 8, 8), 'needs')):
        assert L.tai_frames_to_uint8(*(args + (0, s))) == EINVAL, args
        assert text in err(), (args, err())
    torch.cuda.synchronize()
    assert (out == 5.0).all() and (u == 9).all()                                   # nothing was launched
    assert call() == 0 and err() == ''
    torch.cuda.synchronize()
    assert torch.equal(out.view(1, 2, 3, 8, 8).cpu(), host_clip(item['frames'].numpy(), 3, [8, 8], [0, 0], False, False)[None])
