"""Partly damaged frames without a GPU: the block scan's CPU path against a per-block loop, the identity with the frame scan, the rule that
tells damage from content on a hand-made map, the frame flags at their threshold, the tap tables against ``resize_bilinear`` itself, the
composite's restatement, ``--dry_run`` end to end, the report with the feature off, every refusal of the two C entries (argument checks run
before any runtime call, so they need no device) and the kernels' launch constants."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))          # (for the child process of the refusal test)
from block_scan_ref import block_scan_ref, damage_runs_ref  # noqa: E402
from damage_composite_ref import alpha_ref, core_ref, damage_composite_ref, tap_tables_ref  # noqa: E402

from video_frame_inpainting_amd import _native, restore  # noqa: E402
from video_frame_inpainting_amd.data import resize_bilinear  # noqa: E402
from video_frame_inpainting_amd.restore import MOSTLY, PARTIAL, block_flags, block_scan, classify_blocks, damage_runs, tap_tables  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the scan

def _loop(frames, bs, tol):
    n, h, w, c = frames.shape
    Bh, Bw = -(-h // bs), -(-w // bs)
    out = np.zeros((n, Bh, Bw, 4), dtype=np.int64)
    for i in range(n):
        for y in range(h):
            for x in range(w):
                for k in range(c):
                    v = int(frames[i, y, x, k])
                    row = out[i, y // bs, x // bs]
                    row[0] += v
                    row[1] += v * v
                    if i > 0:
                        d = abs(v - int(frames[i - 1, y, x, k]))
                        row[2] += d
                        row[3] += d > tol
    return out


@pytest.mark.parametrize('shape,bs,tol', [((1, 1, 1, 1), 8, 0), ((3, 17, 17, 3), 8, 0), ((4, 9, 33, 3), 16, 3), ((3, 40, 23, 4), 32, 254),
                                          ((2, 33, 70, 2), 16, 3), ((3, 16, 48, 1), 8, 0)])
def test_the_cpu_path_and_the_restatement_are_the_per_block_loop_and_block_rows_sum_to_frame_rows(shape, bs, tol):
    rng = np.random.RandomState(sum(shape) + bs)
    frames = rng.randint(0, 256, shape).astype(np.uint8)
    frames[-1, ::2] = frames[-2, ::2] if shape[0] > 1 else frames[-1, ::2]
    want = _loop(frames, bs, tol)
    assert np.array_equal(block_scan_ref(frames, bs, tol), want)
    got = block_scan(torch.from_numpy(frames), bs, tol)
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape and np.array_equal(got.numpy(), want)
    whole = restore._scan_numpy(frames.reshape(shape[0], -1), tol)
    assert np.array_equal(got.numpy().sum(axis=(1, 2)), whole)


def test_what_the_cpu_path_refuses():
    ok = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    for bad, bs, tol in ((ok.float(), 8, 0), (ok[0], 8, 0), (ok[:, :, ::2], 8, 0), (ok, 12, 0), (ok, 8, 255), (ok, 8, -1),
                         (torch.zeros(2, 8, 8, 5, dtype=torch.uint8), 8, 0), (ok[:0], 8, 0)):
        with pytest.raises(ValueError):
            block_scan(bad, bs, tol)


# ---------------------------------------------------------------------------------------------------------------- the classifier

def test_classify_blocks_uses_the_bytes_of_each_block():
    # frames of 10 x 12 x 1 in blocks of 8: blocks of 64, 32, 16 and 8 bytes
    h, w, bs = 10, 12, 8
    row = lambda s1, s2, nd: [s1, s2, 0, nd]
    stats = np.zeros((2, 2, 2, 4), dtype=np.int64)
    # frame 1: every block has 2 differing bytes; floor(share nb) with share 1/16 is 4, 2, 1, 0
    stats[1] = np.array([[row(1, 9, 2), row(1, 9, 2)], [row(1, 9, 2), row(1, 9, 2)]])
    stats[0] = stats[1]
    raw = classify_blocks(stats, h, w, 1, bs, ('dup',), block_dup_share=1 / 16.0)
    assert raw[0].tolist() == [[False, False], [False, False]]                       # frame 0 is never a repeat
    assert raw[1].tolist() == [[True, True], [False, False]]
    assert classify_blocks(stats, h, w, 1, bs, ('dup',))[1].tolist() == [[False, False], [False, False]]
    # blank: nb s2 - s1^2 <= var nb^2.  A constant block of level 3: s1 = 3 nb, s2 = 9 nb; one level off it is not blank at var 0
    for by, bx, nb in ((0, 0, 64), (0, 1, 32), (1, 0, 16), (1, 1, 8)):
        stats[:, by, bx] = row(3 * nb, 9 * nb, 9)
    assert classify_blocks(stats, h, w, 1, bs, ('blank',)).all()
    stats[1, 1, 1] = row(3 * 8 + 1, 9 * 8 + 7, 9)                                   # one byte at 4: variance 79/8 - (25/8)^2 = 7/64
    assert classify_blocks(stats, h, w, 1, bs, ('blank',))[1].tolist() == [[True, True], [True, False]]
    assert classify_blocks(stats, h, w, 1, bs, ('blank',), block_blank_var=7 / 64.0)[1, 1, 1]
    assert not classify_blocks(stats, h, w, 1, bs, ('blank',), block_blank_var=6 / 64.0)[1, 1, 1]
    assert not classify_blocks(stats, h, w, 1, bs, ()).any()
    for kw in ({'block_dup_share': 1.5}, {'block_blank_var': -1.0}):
        with pytest.raises(ValueError):
            classify_blocks(stats, h, w, 1, bs, ('dup',), **kw)
    with pytest.raises(ValueError):
        classify_blocks(stats, h, w, 1, bs, ('missing',))
    with pytest.raises(ValueError):
        classify_blocks(stats, 64, 64, 1, bs, ('dup',))
    assert restore.parse_detect_blocks('dup, blank') == {'dup', 'blank'} and restore.parse_detect_blocks('none') == set() == restore.parse_detect_blocks('')
    with pytest.raises(ValueError):
        restore.parse_detect_blocks('missing')


def test_the_run_rule_on_a_hand_made_map():
    n, max_T = 20, 3
    raw = np.zeros((n, 3, 4), dtype=bool)
    want = np.zeros_like(raw)
    raw[5, 0, 0] = want[5, 0, 0] = True                              # a run of 1
    raw[5:8, 0, 1] = want[5:8, 0, 1] = True                          # a run of max_T
    raw[5:9, 0, 2] = True                                            # max_T + 1: dropped
    raw[0:2, 0, 3] = True                                            # touches frame 0: dropped
    raw[18:20, 1, 0] = True                                          # touches the last frame: dropped
    raw[:, 2, :] = True                                              # a letterbox row over all frames: dropped
    raw[4:6, 1, 1] = want[4:6, 1, 1] = True                          # two short runs separated by one clean frame: both kept
    raw[7:10, 1, 1] = want[7:10, 1, 1] = True
    raw[1, 1, 2] = want[1, 1, 2] = True                              # next to frame 0 but not touching it
    raw[18, 1, 3] = want[18, 1, 3] = True
    got = damage_runs(raw, max_T)
    assert got.dtype == bool and np.array_equal(got, want) and np.array_equal(damage_runs_ref(raw, max_T), want)
    rng = np.random.RandomState(0)
    for T in (1, 2, 5):
        noise = rng.rand(17, 2, 3) < 0.45
        assert np.array_equal(damage_runs(noise, T), damage_runs_ref(noise, T))


def test_partial_and_mostly_at_the_threshold_and_a_damage_map_of_the_wrong_shape(tmp_path):
    damaged = np.zeros((5, 3, 4), dtype=bool)                        # share 0.45: floor(0.45 * 12) = 5 blocks
    damaged[1].flat[:1] = True
    damaged[2].flat[:5] = True
    damaged[3].flat[:6] = True
    damaged[4] = True
    assert block_flags(damaged, 0.45).tolist() == [0, PARTIAL, PARTIAL, MOSTLY, MOSTLY]
    assert block_flags(damaged, 0.5).tolist() == [0, PARTIAL, PARTIAL, PARTIAL, MOSTLY]
    assert block_flags(damaged, 0).tolist() == [0, MOSTLY, MOSTLY, MOSTLY, MOSTLY]
    assert (PARTIAL, MOSTLY) == (16, 32)
    np.save(str(tmp_path / 'ok.npy'), damaged.astype(np.uint8) * 7)
    assert np.array_equal(restore.load_damage_map(str(tmp_path / 'ok.npy'), (5, 3, 4)), damaged)
    with pytest.raises(ValueError, match=r'\(5, 3, 4\).*\(5, 4, 3\)'):
        restore.load_damage_map(str(tmp_path / 'ok.npy'), (5, 4, 3))
    np.save(str(tmp_path / 'float.npy'), damaged.astype(np.float32))
    with pytest.raises(ValueError):
        restore.load_damage_map(str(tmp_path / 'float.npy'), (5, 3, 4))


# ---------------------------------------------------------------------------------------------------------------- the composite

@pytest.mark.parametrize('n_in,n_out', [(48, 32), (20, 33), (24, 24)])
def test_tap_tables_list_exactly_the_indices_resize_bilinear_gives_weight_to(n_in, n_out):
    i0, i1 = tap_tables(n_in, n_out)
    r0, r1 = tap_tables_ref(n_in, n_out)
    assert i0.dtype == i1.dtype == np.int32 and np.array_equal(i0, r0) and np.array_equal(i1, r1)
    # one source row at a time set to 255 on a black frame of two columns: the output rows that move are the rows that read it
    touched = [set() for _ in range(n_out)]
    for k in range(n_in):
        frame = np.zeros((n_in, 2, 1), dtype=np.uint8)
        frame[k] = 255
        out = resize_bilinear(frame, n_out, 2) if n_in != n_out else frame
        for i in np.nonzero(out[:, 0, 0])[0]:
            touched[i].add(k)
    assert touched == [{int(a), int(b)} for a, b in zip(i0, i1)]
    if n_in == n_out:
        assert np.array_equal(i0, np.arange(n_in)) and np.array_equal(i1, i0)


def test_the_composite_restatement_is_pred_on_the_core_src_beyond_the_feather_and_monotone_between():
    h, w, bs, feather = 40, 44, 8, 4
    taps = tap_tables(48, h) + tap_tables(66, w)
    blocks = np.zeros((6, 9), dtype=np.uint8)
    blocks[2, 3] = 1
    D = core_ref(blocks, taps, bs, h, w)
    ys, xs = np.nonzero(D)
    # source rows 16..23 are read by model rows 13..19 ((y + .5) * 1.2 - .5 and its neighbour), columns 24..31 by 16..21
    assert (ys.min(), ys.max(), xs.min(), xs.max()) == (13, 19, 16, 21) and D[13:20, 16:22].all()
    A = alpha_ref(D, feather)
    assert (A[D] == 5).all() and A[12, 16] == 4 and A[8, 16] == 0 and A[9, 16] == 1 and A[9, 11] == 0 and A[9, 12] == 1 and A[20, 25] == 1 and A[20, 26] == 0
    pred, src = np.full((1, h + 3, w + 2), 1.0, np.float32), np.full((1, h + 3, w + 2), -1.0, np.float32)
    out = damage_composite_ref(pred, src, blocks, taps, bs, h, w, feather, False)[:, :, 0].astype(int)
    assert (out[D] == 255).all() and (out[A == 0] == 0).all()
    assert out[16, 21:28].tolist() == [255, 204, 153, 102, 51, 0, 0] and (np.diff(out[16, 21:]) <= 0).all() and (np.diff(out[:14, 18]) >= 0).all()
    hard = damage_composite_ref(pred, src, blocks, taps, bs, h, w, 0, False)[:, :, 0]
    assert np.array_equal(hard == 255, D) and np.array_equal(hard == 0, ~D)
    # a single pixel: A = R gives u(pred), A = 0 gives u(src)
    P, S = np.full((1, 1, 1), 0.0, np.float32), np.full((1, 1, 1), -0.5, np.float32)            # u = 127, 63
    one = lambda f, b: int(damage_composite_ref(P, S, np.array([[b]]), (np.zeros(1, np.int32),) * 4, 8, 1, 1, f, False)[0, 0, 0])
    assert one(3, 1) == 127 and one(3, 0) == 63
    # no block damaged / all damaged: the pixels of src / pred, channels reversed when asked, NaN -> 0
    rng = np.random.RandomState(1)
    pred3 = rng.uniform(-1.3, 1.3, (3, 9, 9)).astype(np.float32)
    src3 = rng.uniform(-1.3, 1.3, (3, 9, 9)).astype(np.float32)
    pred3[0, 0, 0] = np.nan
    ident = tap_tables(8, 8) + tap_tables(7, 7)
    from video_frame_inpainting_amd.util import frames_to_uint8
    for rev in (False, True):
        none = damage_composite_ref(pred3, src3, np.zeros((1, 1)), ident, 8, 8, 7, 4, rev)
        every = damage_composite_ref(pred3, src3, np.ones((1, 1)), ident, 8, 8, 7, 4, rev)
        want_s = frames_to_uint8(torch.from_numpy(src3[None]))[0, :8, :7]
        want_p = frames_to_uint8(torch.from_numpy(np.nan_to_num(pred3, nan=-1.0)[None]))[0, :8, :7]
        assert np.array_equal(none, want_s[:, :, ::-1] if rev else want_s) and np.array_equal(every, want_p[:, :, ::-1] if rev else want_p)


# ---------------------------------------------------------------------------------------------------------------- the dry run

def _smooth(rng, t, h, w):
    """The moving blobs plus noise of tests/test_restore_cpu.py."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    frames = np.zeros((t, h, w, 3))
    for c in range(3):
        cx, cy, vx, vy = rng.uniform(0.2, 0.8) * w, rng.uniform(0.2, 0.8) * h, rng.uniform(-2, 2), rng.uniform(-2, 2)
        for k in range(t):
            frames[k, :, :, c] = 255 * np.exp(-((x - cx - vx * k) ** 2 + (y - cy - vy * k) ** 2) / (2 * (0.2 * w) ** 2))
    return np.clip(frames + rng.uniform(0, 20, frames.shape), 0, 255).astype(np.uint8)


def _write_dir(root, frames):
    os.makedirs(str(root))
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(str(root), '%04d.png' % i))


COMMON = ['--name', 'x', '--K', '3', '--T', '2', '--F', '3', '--c_dim', '1', '--image_size', '32', '--model_key', 'MCNet_gray', '--dry_run']


def test_dry_run_reports_a_painted_block_as_a_partial_frame(tmp_path):
    import restore as restore_cli
    frames = _smooth(np.random.RandomState(5), 40, 40, 56)               # blocks of 16: 3 x 4, the last row and column ragged
    frames[10, 16:32, 32:48] = 77
    frames[:, 32:, :] = 0                                                # a bar at the bottom of EVERY frame: content
    _write_dir(tmp_path / 'video', frames)
    report = restore_cli.main(COMMON + ['--input', str(tmp_path / 'video'), '--output_dir', str(tmp_path / 'out'), '--detect_blocks', 'blank',
                                        '--chunk_frames', '7'])
    on_disk = json.load(open(str(tmp_path / 'out' / 'report.json')))
    assert on_disk == json.loads(json.dumps(report))
    assert [f['flags'] for f in on_disk['frames']] == [PARTIAL if i == 10 else 0 for i in range(40)]
    assert [f['blocks'] for f in on_disk['frames']] == [[[1, 2]] if i == 10 else [] for i in range(40)]
    assert [(g['start'], g['T'], g['K'], g['F'], g['status'], g['positions'], g['composited']) for g in on_disk['gaps']] == [
        (10, 1, 3, 3, 'fill', [10], [10])]
    s = on_disk['settings']
    assert (s['detect_blocks'], s['block_size'], s['feather'], s['block_share'], s['block_dup_share'], s['block_blank_var'], s['damage_map']) == \
        (['blank'], 16, 4, 0.5, 0.0, 0.0, '')
    # the block rows of the driver cross the chunks of 7 frames and are the restatement's
    r = restore.Restorer(None, restore_cli_options(tmp_path, ['--detect_blocks', 'dup', '--chunk_frames', '7']))
    reader, present = restore.open_source(str(tmp_path / 'video'))
    r.plan(reader, present, torch.device('cpu'))
    assert np.array_equal(r.block_stats.numpy(), block_scan_ref(frames, 16, 0))
    # a damage map alone: OR-ed in unfiltered (frame 0 included), no detector run; a wrong shape is refused and names both shapes
    named = np.zeros((40, 3, 4), dtype=np.uint8)
    named[0, 0, 0] = named[20, 2, 3] = named[21] = 1
    np.save(str(tmp_path / 'map.npy'), named)
    report = restore_cli.main(COMMON + ['--input', str(tmp_path / 'video'), '--output_dir', str(tmp_path / 'out2'), '--damage_map',
                                        str(tmp_path / 'map.npy')])
    assert [f['flags'] for f in report['frames']] == [{0: PARTIAL, 20: PARTIAL, 21: MOSTLY}.get(i, 0) for i in range(40)]
    assert report['frames'][20]['blocks'] == [[2, 3]] and report['gaps'][1]['composited'] == [20] and report['gaps'][0]['composited'] == []
    np.save(str(tmp_path / 'wrong.npy'), named[:, :, :3])
    for bad in (['--damage_map', str(tmp_path / 'wrong.npy')], ['--detect_blocks', 'missing'], ['--detect_blocks', 'dup', '--feather', '16'],
                ['--detect_blocks', 'dup', '--block_share', '1.5']):
        with pytest.raises(SystemExit) as e:
            restore_cli.main(COMMON + ['--input', str(tmp_path / 'video'), '--output_dir', str(tmp_path / 'out3')] + bad)
        assert e.value.code not in (0, None), bad
    with pytest.raises(SystemExit, match=r'\(40, 3, 3\).*\(40, 3, 4\)'):
        restore_cli.main(COMMON + ['--input', str(tmp_path / 'video'), '--output_dir', str(tmp_path / 'out3'), '--damage_map',
                                   str(tmp_path / 'wrong.npy')])


def restore_cli_options(tmp_path, extra):
    from video_frame_inpainting_amd.options import RestoreOptions
    return RestoreOptions().parse(COMMON + ['--input', str(tmp_path / 'video'), '--output_dir', str(tmp_path / 'unused')] + extra,
                                  require_gpu=False)


def test_with_the_feature_off_the_report_has_the_keys_it_had(tmp_path):
    import restore as restore_cli
    frames = _smooth(np.random.RandomState(6), 12, 32, 32)
    frames[5, :16, :16] = 77                                             # a painted block nobody asked to look for
    frames[8] = frames[7]
    _write_dir(tmp_path / 'video', frames)
    report = restore_cli.main(COMMON + ['--input', str(tmp_path / 'video'), '--output_dir', str(tmp_path / 'out'), '--detect', 'dup'])
    assert set(report) == {'input', 'n_frames', 'dry_run', 'settings', 'frames', 'gaps'}
    assert set(report['settings']) == {'K', 'T', 'F', 'max_T', 'detect', 'gaps', 'dup_tol', 'dup_share', 'blank_var', 'chunk_frames',
                                       'batch_size', 'c_dim', 'image_size', 'padding_size'}
    assert all(set(f) == {'index', 's1', 's2', 'sad', 'ndiff', 'flags'} for f in report['frames'])
    assert len(report['gaps']) == 1 and set(report['gaps'][0]) == {'start', 'T', 'K', 'F', 'status', 'positions'}
    assert [f['flags'] for f in report['frames']] == [restore.DUPLICATE if i == 8 else 0 for i in range(12)]
    r = restore.Restorer(None, restore_cli_options(tmp_path, []))
    assert not r.blocks_on and r.detect_blocks == frozenset()


# ---------------------------------------------------------------------------------------------------------------- the C ABI's refusals

P = 16                          # a pointer that is never followed: a refused call reads none of its buffers
EINVAL = -1


def _scan(frames=P, n=4, h=16, w=16, c=3, bs=8, tol=0, stats=P, workspace=P):
    return [frames, n, h, w, c, bs, tol, stats, workspace]


# (arguments, the words the message holds)
SCAN_REFUSALS = [
    (_scan(frames=None), 'frames'), (_scan(stats=None), 'stats'),
    (_scan(n=0), 'n_frames'), (_scan(n=-3), 'n_frames'),
    (_scan(h=0), 'h and w'), (_scan(w=-1), 'h and w'),
    (_scan(c=0), 'c must'), (_scan(c=5), 'c must'),
    (_scan(bs=0), 'bs'), (_scan(bs=12), 'bs'), (_scan(bs=64), 'bs'),
    (_scan(h=1 << 15, w=1 << 15, c=2), 'h x w x c must be below'), (_scan(h=(1 << 31) - 1, w=(1 << 31) - 1, c=4), 'h x w x c must be below'),
    (_scan(n=(1 << 20) + 1, h=1024, w=1024, c=1), 'n_frames x h x w x c'), (_scan(n=1 << 62, h=1, w=1, c=1), 'n_frames x h x w x c'),
    (_scan(tol=-1), 'tol'), (_scan(tol=255), 'tol'),
    (_scan(stats=P + 4), 'aligned'),
]
SIZE_WORDS = ('n_frames', 'h and w', 'c must', 'bs', 'h x w x c must be below', 'n_frames x h x w x c')


def _comp(pred=P, pred_elems=4096, src=P, src_elems=8192, table=P, items=(0, 0, 0, 0), n_items=1, blocks=P, n_maps=2, Bh=2, Bw=2, bs=16,
          r0=P, r1=P, c0=P, c1=P, out=P, n_out=2, C=1, Hs=32, Ws=32, h=32, w=32, feather=4, reverse=0):
    return [pred, pred_elems, src, src_elems, table, ('i64', list(items)) if items is not None else None, n_items, blocks, n_maps, Bh, Bw, bs,
            r0, r1, c0, c1, out, n_out, C, Hs, Ws, h, w, feather, reverse]


COMP_REFUSALS = [
    (_comp(pred=None), 'null'), (_comp(src=None), 'null'), (_comp(table=None), 'null'), (_comp(items=None), 'null'), (_comp(blocks=None), 'null'),
    (_comp(r0=None), 'null'), (_comp(r1=None), 'null'), (_comp(c0=None), 'null'), (_comp(c1=None), 'null'), (_comp(out=None), 'null'),
    (_comp(C=2), 'C must'), (_comp(C=4), 'C must'), (_comp(bs=4), 'bs'), (_comp(feather=-1), 'feather'), (_comp(feather=16), 'feather'),
    (_comp(n_items=0), 'n_items'), (_comp(n_maps=0), 'n_items'), (_comp(n_out=0), 'n_items'), (_comp(Bh=0), 'n_items'), (_comp(Bw=-1), 'n_items'),
    (_comp(h=0), 'h <= Hs'), (_comp(h=33), 'h <= Hs'), (_comp(w=33), 'h <= Hs'), (_comp(w=0), 'h <= Hs'),
    (_comp(Hs=1 << 16, Ws=1 << 15), 'index space'), (_comp(n_maps=1 << 29), 'index space'),
    (_comp(items=(3073, 0, 0, 0)), 'predicted frame'), (_comp(items=(-1, 0, 0, 0)), 'predicted frame'), (_comp(pred_elems=1023), 'predicted frame'),
    (_comp(items=(0, 7169, 0, 0)), 'source frame'), (_comp(items=(0, -1, 0, 0)), 'source frame'),
    (_comp(items=(0, 0, 2, 0)), 'block map'), (_comp(items=(0, 0, -1, 0)), 'block map'),
    (_comp(items=(0, 0, 0, 2)), 'output frame'), (_comp(items=(0, 0, 0, -1)), 'output frame'),
    (_comp(items=(3072, 7168, 1, 1, 0, 0, 0, 5), n_items=2), 'output frame'),           # the first item at its limits is taken, the second refused
]


def _answers(lib_path):
    """Run in a child process that sees no device: (return code, message) of every refusal -- calls that end before any launch -- and the
    workspace query's answers for the scan's sizes."""
    L = ctypes.CDLL(lib_path)
    for name, (restype, argtypes) in _native.signatures().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    scan, comp = [], []
    for args, _ in SCAN_REFUSALS:
        rc = L.tai_block_scan(*args, None)
        scan.append([rc, L.tai_sepconv_last_error().decode(), L.tai_block_scan_workspace_bytes(*args[1:6])])
    for args, _ in COMP_REFUSALS:
        keep = [(ctypes.c_longlong * len(a[1]))(*a[1]) if isinstance(a, tuple) else a for a in args]
        rc = L.tai_damage_composite(*[ctypes.cast(a, ctypes.c_void_p) if isinstance(a, ctypes.Array) else a for a in keep], None)
        comp.append([rc, L.tai_sepconv_last_error().decode()])
    return {'scan': scan, 'comp': comp}


def test_every_refusal_of_both_entries_returns_the_error_and_names_the_argument_without_a_device():
    _native.verify(_native.LIB_PATH)
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1')
    child = subprocess.run([sys.executable, os.path.abspath(__file__), '--answers', _native.LIB_PATH], env=env, capture_output=True, text=True,
                           timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    got = json.loads(child.stdout)
    assert len(got['scan']) == len(SCAN_REFUSALS) and len(got['comp']) == len(COMP_REFUSALS)
    for (args, word), (rc, message, query) in zip(SCAN_REFUSALS, got['scan']):
        assert rc == EINVAL and message.startswith('block_scan: ') and word in message, (args, rc, message)
        assert query == (EINVAL if word in SIZE_WORDS else 0), (args, query)          # this version needs no workspace
    for (args, word), (rc, message) in zip(COMP_REFUSALS, got['comp']):
        assert rc == EINVAL and message.startswith('damage_composite: ') and word in message, (args, rc, message)
    # every message of both refusal() functions is reached
    for name, prefix, rows, count in (('block_scan.hip.inc', 'block_scan', got['scan'], 10), ('damage_composite.hip.inc', 'damage_composite',
                                                                                               got['comp'], 11)):
        source = open(os.path.join(_native.CSRC, name)).read()
        said = {r[1] for r in rows}
        assert len(said) == count and set(re.findall(r'return "(%s: [^"]*)";' % prefix, source)) == said


# ---------------------------------------------------------------------------------------------------------------- header, library

# restated; tests/test_gpu_block_scan.py and tests/test_gpu_damage_composite.py build their shapes from them
SCAN_THREADS, RUN, SCAN_GRID_CAP, SEG_BYTES = 256, 8, 1 << 14, 1024
TILE_H, TILE_W, COMP_GRID_CAP, MAX_FEATHER = 32, 64, 1 << 12, 15


def test_the_header_declares_the_entries_and_the_launch_constants_are_the_sources():
    header = open(os.path.join(ROOT, 'include', 'tai_sepconv.h')).read()
    assert {'tai_block_scan', 'tai_block_scan_workspace_bytes', 'tai_damage_composite'} <= set(_native.declared_symbols())
    assert 'long long tai_block_scan_workspace_bytes(long long n_frames, int h, int w, int c, int bs);' in header
    assert 'gives row i of tai_frame_scan' in header                                   # the identity the GPU test holds
    V, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    sigs = _native.signatures()
    assert sigs['tai_block_scan'] == (I, [V, LL, I, I, I, I, I, V, V, V]) and sigs['tai_block_scan_workspace_bytes'] == (LL, [LL, I, I, I, I])
    assert sigs['tai_damage_composite'] == (I, [V, LL, V, LL, V, V, LL, V, LL, I, I, I, V, V, V, V, V, LL, I, I, I, I, I, I, I, V])
    assert not re.search(r'tai_(block_scan|damage_composite)\s*\([^)]*hip_stream\)', _native._header_text())
    L = ctypes.CDLL(_native.LIB_PATH)
    L.tai_sepconv_version.restype = ctypes.c_int
    assert L.tai_sepconv_version() >= 890
    main = open(_native.MAIN_SOURCE).read()
    for name in ('block_scan.hip.inc', 'damage_composite.hip.inc'):
        assert os.path.join(_native.CSRC, name) in _native.sources() and '#include "%s"' % name in main
    scan = open(os.path.join(_native.CSRC, 'block_scan.hip.inc')).read()
    for line in ('constexpr int THREADS = %d;' % SCAN_THREADS, 'constexpr int RUN = %d;' % RUN, 'constexpr int VEC_BYTES = 16;',
                 'constexpr int SEG_BYTES = 64 * VEC_BYTES;', 'constexpr long long GRID_CAP = 1LL << 14;',
                 'constexpr int MAX_BLOCK_BYTES = 32 * 32 * 4;', 'constexpr long long MAX_TOTAL_BYTES = 1LL << 40;',
                 'static_assert((unsigned long long)MAX_BLOCK_BYTES * 255 * 255 < (1ULL << 32)'):
        assert line in scan, line
    assert 32 * 32 * 4 * 255 * 255 < 2 ** 32 and SEG_BYTES == 64 * 16
    # every block size times every channel count is a whole number of 8-byte units and fits a segment
    assert all((bs * c) % 8 == 0 and SEG_BYTES // (bs * c) >= 1 for bs in (8, 16, 32) for c in (1, 2, 3, 4))
    comp = open(os.path.join(_native.CSRC, 'damage_composite.hip.inc')).read()
    for line in ('constexpr int THREADS = 256;', 'constexpr int TILE_H = %d, TILE_W = %d;' % (TILE_H, TILE_W),
                 'constexpr int MAX_FEATHER = %d;' % MAX_FEATHER, 'constexpr long long GRID_CAP = 1LL << 12;'):
        assert line in comp, line
    assert (TILE_W * 1) % 16 == 0 and (TILE_W * 3) % 16 == 0 and restore.MAX_FEATHER == MAX_FEATHER
    for source in (scan, comp):
        assert 'atomic' not in source.replace('no atomics', '').replace('No atomics', '') and 'asm' not in source


if __name__ == '__main__':
    if sys.argv[1:2] == ['--answers'] and len(sys.argv) == 3:
        assert os.environ.get('HIP_VISIBLE_DEVICES') == '-1' and os.environ.get('ROCR_VISIBLE_DEVICES') == '-1'
        print(json.dumps(_answers(sys.argv[2])))
