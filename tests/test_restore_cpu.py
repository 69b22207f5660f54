"""restore.py without a GPU: the scan's restatement and the module's CPU path, the classifier's thresholds, the planner's rule on hand-written
masks, the sources' ``present`` masks, ``--dry_run`` end to end, every refusal of the two C entries (argument checks run before any
runtime call, so they need no device) and the kernel's launch constants."""
import ctypes
import json
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))          # (for the child process of the refusal test)
from frame_scan_ref import frame_scan_ref  # noqa: E402

from video_frame_inpainting_amd import _native, restore, synthetic  # noqa: E402
from video_frame_inpainting_amd.restore import BLANK, DUPLICATE, LISTED, MISSING, classify, parse_gaps, plan_gaps, scan_frames  # noqa: E402
from video_frame_inpainting_amd.util import frames_to_uint8  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the scan

def _loop(frames, tol):
    n = len(frames)
    flat = [list(map(int, f.reshape(-1))) for f in frames]
    out = []
    for i in range(n):
        s1 = s2 = sad = nd = 0
        for k, v in enumerate(flat[i]):
            s1 += v
            s2 += v * v
            if i > 0:
                d = abs(v - flat[i - 1][k])
                sad += d
                nd += d > tol
        out.append([s1, s2, sad, nd])
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize('shape,tol', [((1, 1), 0), ((4, 7), 0), ((5, 3, 2, 3), 3), ((3, 17), 254), ((6, 4, 4), 100)])
def test_the_restatement_is_the_per_byte_loop_and_the_cpu_path_is_the_restatement(shape, tol):
    rng = np.random.RandomState(len(shape) * 100 + tol)
    frames = rng.randint(0, 256, shape).astype(np.uint8)
    frames[-1].flat[0] = 255
    want = _loop(frames, tol)
    got = frame_scan_ref(frames, tol)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    mine = scan_frames(torch.from_numpy(frames), tol)
    assert mine.dtype == torch.int64 and mine.shape == (shape[0], 4) and np.array_equal(mine.numpy(), want)


def test_differences_of_exactly_tol_and_tol_plus_one_and_what_the_cpu_path_refuses():
    frames = np.array([[10, 10, 10, 200], [13, 14, 6, 197]], dtype=np.uint8)        # |d| = 3, 4, 4, 3
    assert scan_frames(torch.from_numpy(frames), 3)[1].tolist() == [230, 13 * 13 + 14 * 14 + 36 + 197 * 197, 14, 2]
    assert scan_frames(torch.from_numpy(frames), 4)[1, 3] == 0 and scan_frames(torch.from_numpy(frames), 2)[1, 3] == 4
    for bad in (torch.zeros(3, 4), torch.zeros(0, 4, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8),
                torch.zeros(4, 6, dtype=torch.uint8)[:, ::2]):
        with pytest.raises(ValueError):
            scan_frames(bad, 0)
    for tol in (-1, 255):
        with pytest.raises(ValueError):
            scan_frames(torch.zeros(2, 2, dtype=torch.uint8), tol)


# ---------------------------------------------------------------------------------------------------------------- flags

ALL = ('missing', 'dup', 'blank')


def test_classify_on_each_side_of_every_threshold():
    n = 100                                                   # bytes per frame
    present, none = np.ones(4, dtype=bool), np.zeros(4, dtype=bool)
    row = lambda s1, s2, ndiff: [s1, s2, 0, ndiff]
    # exact repeat / one byte moved; constant (n s2 == s1^2) / one level off it
    stats = np.array([row(500, 2500, 0), row(500, 2500, 0), row(501, 2511, 1), row(1000, 10000, 100)], dtype=np.int64)
    assert classify(stats, n, present, none, ALL).tolist() == [BLANK, DUPLICATE | BLANK, 0, BLANK]
    assert classify(stats, n, present, none, ('dup',)).tolist() == [0, DUPLICATE, 0, 0]          # frame 0 is never a duplicate
    assert classify(stats, n, present, none, ()).tolist() == [0, 0, 0, 0]
    # dup_share: floor(0.035 * 100) = 3 bytes may differ
    stats = np.array([row(9, 1000, 0), row(9, 1000, 3), row(9, 1000, 4), row(9, 1000, 100)], dtype=np.int64)
    assert classify(stats, n, present, none, ('dup',), dup_share=0.035).tolist() == [0, DUPLICATE, 0, 0]
    assert classify(stats, n, present, none, ('dup',), dup_share=0.04).tolist() == [0, DUPLICATE, DUPLICATE, 0]
    assert classify(stats, n, present, none, ('dup',), dup_share=1.0).tolist() == [0, DUPLICATE, DUPLICATE, DUPLICATE]
    # blank_var: n s2 - s1^2 <= var n^2; s1 = 1000: var 2.5 means s2 <= 10250
    stats = np.array([row(1000, 10250, 50), row(1000, 10251, 50), row(1000, 10000, 50), row(0, 0, 50)], dtype=np.int64)
    assert classify(stats, n, present, none, ('blank',), blank_var=2.5).tolist() == [BLANK, 0, BLANK, BLANK]
    assert classify(stats, n, present, none, ('blank',)).tolist() == [0, 0, BLANK, BLANK]
    # the source's mask and the caller's list
    present = np.array([True, False, True, False])
    listed = np.array([False, False, True, True])
    assert classify(stats, n, present, listed, ('missing',)).tolist() == [0, MISSING, LISTED, MISSING | LISTED]
    assert classify(stats, n, present, listed, ('blank',)).tolist() == [0, 0, BLANK | LISTED, BLANK | LISTED]
    assert classify(torch.from_numpy(stats), n, present, None, ('missing',)).tolist() == [0, MISSING, 0, MISSING]
    # integers beyond float64: n s2 and s1^2 near 2^62 differ by one
    big = np.array([[2 ** 31 - 1, (2 ** 31 - 1) ** 2 // 4 + 1, 0, 9]], dtype=np.int64)
    assert classify(big, 4, [True], None, ('blank',)).tolist() == [0]
    assert classify(big - [[0, 1, 0, 0]], 4, [True], None, ('blank',)).tolist() == [BLANK]
    for kw in ({'dup_share': -0.1}, {'dup_share': 1.5}, {'blank_var': -1.0}):
        with pytest.raises(ValueError):
            classify(stats, n, present, None, ALL, **kw)
    with pytest.raises(ValueError):
        classify(stats, n, present, None, ('duplicate',))


def test_gaps_and_detect_parse_and_refuse():
    assert parse_gaps('', 5).tolist() == [False] * 5 and parse_gaps(None, 2).tolist() == [False, False]
    assert parse_gaps('1-2, 4', 6).tolist() == [False, True, True, False, True, False]
    assert parse_gaps('0-5', 6).all() and parse_gaps('5-5', 6).tolist() == [False] * 5 + [True]
    for bad in ('3-1', '2-6', '6', 'a-b', '1-', '-1', '1--2', '1.5'):
        with pytest.raises(ValueError):
            parse_gaps(bad, 6)
    assert restore.parse_detect('missing,dup') == {'missing', 'dup'} and restore.parse_detect('none') == set() == restore.parse_detect('')
    with pytest.raises(ValueError):
        restore.parse_detect('missing,static')


# ---------------------------------------------------------------------------------------------------------------- the planner

def _mask(n, *flagged):
    m = np.zeros(n, dtype=np.uint8)
    for a in flagged:
        m[a] = MISSING
    return m


def _brief(gaps):
    return [(g['start'], g['T'], g['K'], g['F'], g['status']) for g in gaps]


def test_plan_gaps_on_hand_written_masks():
    K = F = 3
    assert plan_gaps(_mask(12), K, F, 4) == []
    # a single frame; a run
    assert _brief(plan_gaps(_mask(12, 5), K, F, 4)) == [(5, 1, 3, 3, 'fill')]
    g = plan_gaps(_mask(12, 4, 5, 6), K, F, 4)
    assert _brief(g) == [(4, 3, 3, 3, 'fill')] and g[0]['positions'] == [4, 5, 6]
    # a run at frame 0, a run ending at the last frame
    assert _brief(plan_gaps(_mask(12, 0, 1), K, F, 4)) == [(0, 2, 0, 3, 'no_context_before')]
    assert _brief(plan_gaps(_mask(12, 10, 11), K, F, 4)) == [(10, 2, 3, 0, 'no_context_after')]
    # one intact frame at index 0, then a gap; one intact frame behind a gap; two on each side are enough
    assert _brief(plan_gaps(_mask(12, 1, 2), K, F, 4)) == [(1, 2, 1, 3, 'no_context_before')]
    assert _brief(plan_gaps(_mask(12, 9, 10), K, F, 4)) == [(9, 2, 3, 1, 'no_context_after')]
    assert _brief(plan_gaps(_mask(6, 2, 3), K, F, 4)) == [(2, 2, 2, 2, 'fill')]
    # two runs one frame apart: merged, the frame between kept
    g = plan_gaps(_mask(14, 5, 7, 8), K, F, 4)
    assert _brief(g) == [(5, 4, 3, 3, 'fill')] and g[0]['positions'] == [5, 7, 8]
    # three such runs in a chain
    g = plan_gaps(_mask(16, 4, 6, 8, 9), K, F, 8)
    assert _brief(g) == [(4, 6, 3, 3, 'fill')] and g[0]['positions'] == [4, 6, 8, 9]
    # runs two frames apart: not merged; the gap behind gets K = 2, the gap in front F = 2
    assert _brief(plan_gaps(_mask(16, 5, 8, 9), K, F, 4)) == [(5, 1, 3, 2, 'fill'), (8, 2, 2, 3, 'fill')]
    # K and F cut short by a neighbouring gap (and by the ends of the video)
    assert _brief(plan_gaps(_mask(20, 2, 6, 7, 13), 5, 5, 4)) == [(2, 1, 2, 3, 'fill'), (6, 2, 3, 5, 'fill'), (13, 1, 5, 5, 'fill')]
    # T = max_T and max_T + 1; the merged span counts
    assert _brief(plan_gaps(_mask(12, 4, 5, 6, 7), K, F, 4)) == [(4, 4, 3, 3, 'fill')]
    assert _brief(plan_gaps(_mask(12, 4, 5, 6, 7), K, F, 3)) == [(4, 4, 3, 3, 'too_long')]
    assert _brief(plan_gaps(_mask(14, 5, 7, 8), K, F, 3)) == [(5, 4, 3, 3, 'too_long')]
    # a gap that is not filled is no context for its neighbour, and the context statuses come first
    assert _brief(plan_gaps(_mask(12, 0, 1, 2, 3, 4, 5, 7), K, F, 2)) == [(0, 8, 0, 3, 'no_context_before')]
    assert _brief(plan_gaps(np.full(5, LISTED, dtype=np.uint8), K, F, 9)) == [(0, 5, 0, 0, 'no_context_before')]
    # any flag bit makes a frame part of a gap
    assert _brief(plan_gaps(np.array([0, 0, DUPLICATE, BLANK | LISTED, 0, 0], dtype=np.uint8), K, F, 4)) == [(2, 2, 2, 2, 'fill')]


# ---------------------------------------------------------------------------------------------------------------- sources

def _smooth(rng, t, h, w):
    """The moving blobs plus noise of tests/test_gpu_device_preprocess_drivers.py."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    frames = np.zeros((t, h, w, 3))
    for c in range(3):
        cx, cy, vx, vy = rng.uniform(0.2, 0.8) * w, rng.uniform(0.2, 0.8) * h, rng.uniform(-2, 2), rng.uniform(-2, 2)
        for k in range(t):
            frames[k, :, :, c] = 255 * np.exp(-((x - cx - vx * k) ** 2 + (y - cy - vy * k) ** 2) / (2 * (0.2 * w) ** 2))
    return np.clip(frames + rng.uniform(0, 20, frames.shape), 0, 255).astype(np.uint8)


def _write_dir(root, frames, first=0, skip=(), pattern='%04d.png'):
    os.makedirs(str(root))
    for i, f in enumerate(frames):
        if i not in skip:
            Image.fromarray(f).save(os.path.join(str(root), pattern % (first + i)))


def test_a_numbered_directory_reports_its_absent_numbers_and_other_names_fall_back_to_plain_order(tmp_path):
    frames = _smooth(np.random.RandomState(3), 10, 12, 16)
    _write_dir(tmp_path / 'numbered', frames, first=3, skip=(4, 5))               # 0003.png .. 0012.png without 0007 and 0008
    assert sorted(os.listdir(str(tmp_path / 'numbered')))[3:5] == ['0006.png', '0009.png']
    reader, present = restore.open_source(str(tmp_path / 'numbered'))
    assert reader.get_length() == 10 and present.tolist() == [True] * 4 + [False, False] + [True] * 4
    for i in range(10):
        assert np.array_equal(reader.get_data(i), frames[3 if i in (4, 5) else i])       # a missing frame repeats the last present one
    with pytest.raises(IndexError):
        reader.get_data(10)
    _write_dir(tmp_path / 'prefixed', frames[:4], first=7, pattern='shot_b_%d.png')
    assert restore.open_source(str(tmp_path / 'prefixed'))[1].tolist() == [True] * 4
    # mixed names, names without a number, a repeated number: plain order, nothing missing
    _write_dir(tmp_path / 'mixed', frames[:3], first=5)
    Image.fromarray(frames[3]).save(str(tmp_path / 'mixed' / 'last.png'))
    reader, present = restore.open_source(str(tmp_path / 'mixed'))
    assert present.tolist() == [True] * 4 and np.array_equal(reader.get_data(3), frames[3]) and np.array_equal(reader.get_data(0), frames[0])
    _write_dir(tmp_path / 'twice', frames[:2], first=1)
    Image.fromarray(frames[2]).save(str(tmp_path / 'twice' / 'a_0003.png'))
    Image.fromarray(frames[3]).save(str(tmp_path / 'twice' / 'b_3.png'))
    assert restore.open_source(str(tmp_path / 'twice'))[1].tolist() == [True] * 4
    np.save(str(tmp_path / 'a.npy'), frames)
    reader, present = restore.open_source(str(tmp_path / 'a.npy'))
    assert present.all() and len(present) == 10 and np.array_equal(reader.get_data(9), frames[9])
    with pytest.raises(IOError), pytest.warns(UserWarning):
        restore.open_source(str(tmp_path / 'nothing.npy'))


def _chunk(fourcc, payload):
    return fourcc + struct.pack('<I', len(payload)) + payload + (b'\x00' if len(payload) & 1 else b'')


def _write_raw_avi(path, frames, drop):
    """A minimal uncompressed 24-bit AVI 1.0 file (bottom-up BGR rows padded to four bytes); frames in ``drop`` get a chunk of length 0."""
    T, H, W, _ = frames.shape
    row = (3 * W + 3) & ~3
    movi = b''
    for t in range(T):
        rows = np.zeros((H, row), np.uint8)
        rows[:, :3 * W] = frames[t][:, :, ::-1].reshape(H, -1)
        movi += _chunk(b'00db', b'' if t in drop else rows[::-1].tobytes())
    bih = struct.pack('<IiiHH4sIiiII', 40, W, H, 1, 24, b'\x00' * 4, 0, 0, 0, 0, 0)
    strl = _chunk(b'LIST', b'strl' + _chunk(b'strh', b'vids' + b'\x00' * 52) + _chunk(b'strf', bih))
    body = b'AVI ' + _chunk(b'LIST', b'hdrl' + _chunk(b'avih', b'\x00' * 56) + strl) + _chunk(b'LIST', b'movi' + movi)
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', len(body)) + body)


def test_an_avi_reports_its_zero_length_chunks(tmp_path):
    from video_frame_inpainting_amd import video_io
    frames = _smooth(np.random.RandomState(4), 6, 10, 14)
    _write_raw_avi(str(tmp_path / 'v.avi'), frames, drop=(2, 3))
    assert video_io.AviVideo(str(tmp_path / 'v.avi')).dropped_frames() == [2, 3]
    reader, present = restore.open_source(str(tmp_path / 'v.avi'))
    assert present.tolist() == [True, True, False, False, True, True]
    for i in range(6):
        assert np.array_equal(reader.get_data(i), frames[1 if i in (2, 3) else i])
    _write_raw_avi(str(tmp_path / 'w.avi'), frames, drop=(0,))                   # nothing precedes it: the first present frame
    reader, present = restore.open_source(str(tmp_path / 'w.avi'))
    assert present.tolist() == [False] + [True] * 5 and np.array_equal(reader.get_data(0), frames[1])
    _write_raw_avi(str(tmp_path / 'whole.avi'), frames, drop=())
    assert restore.open_source(str(tmp_path / 'whole.avi'))[1].all()


# ---------------------------------------------------------------------------------------------------------------- undamaged videos

def _flags_of(video):
    video = np.ascontiguousarray(video)
    stats = scan_frames(torch.from_numpy(video), 0)
    assert np.array_equal(stats.numpy(), frame_scan_ref(video, 0))
    n = len(video)
    return stats, classify(stats, video[0].size, np.ones(n, dtype=bool), None, ALL)


@pytest.mark.parametrize('c,h,w', [(1, 32, 32), (3, 33, 35), (1, 128, 128)])
def test_undamaged_synthetic_clips_are_flagged_nowhere(c, h, w):
    for clip in synthetic.make_clips(2, 9, c, h, w, 1001):
        video = frames_to_uint8(torch.from_numpy(clip))
        stats, flags = _flags_of(video)
        n = video[0].size
        s1, s2, ndiff = (stats[:, k].numpy().astype(object) for k in (0, 1, 3))
        print('smallest share of bytes that differ %.3f, smallest variance %.1f' % (min(ndiff[1:]) / n, min((n * s2 - s1 * s1)) / (n * n)))
        assert not flags.any()


@pytest.mark.parametrize('t,h,w', [(14, 40, 56), (12, 32, 32), (11, 24, 40)])
def test_undamaged_smooth_videos_are_flagged_nowhere(t, h, w):
    _, flags = _flags_of(_smooth(np.random.RandomState(21), t, h, w))
    assert not flags.any()


# ---------------------------------------------------------------------------------------------------------------- the dry run

def _damaged_dir(root):
    """40 smooth frames: 10-11 copies of 9, 20 constant, files 30 and 31 deleted."""
    frames = _smooth(np.random.RandomState(5), 40, 32, 32)
    frames[10] = frames[11] = frames[9]
    frames[20] = 77
    _write_dir(root, frames, skip=(30, 31), pattern='%04d.png')
    return frames


def test_dry_run_writes_the_expected_report(tmp_path, capsys):
    import restore as restore_cli
    frames = _damaged_dir(tmp_path / 'video')
    common = ['--name', 'x', '--K', '3', '--T', '2', '--F', '3', '--c_dim', '1', '--image_size', '32', '--model_key', 'MCNet_gray',
              '--input', str(tmp_path / 'video'), '--dry_run']
    report = restore_cli.main(common + ['--output_dir', str(tmp_path / 'out'), '--detect', 'missing,dup,blank', '--gaps', '5-5',
                                        '--chunk_frames', '7'])
    assert os.listdir(str(tmp_path / 'out')) == ['report.json']
    on_disk = json.load(open(str(tmp_path / 'out' / 'report.json')))
    assert on_disk == json.loads(json.dumps(report)) and on_disk['dry_run'] is True and on_disk['n_frames'] == 40
    delivered = frames.copy()
    delivered[30] = delivered[31] = frames[29]
    want = frame_scan_ref(delivered, 0)
    assert [[f['s1'], f['s2'], f['sad'], f['ndiff']] for f in on_disk['frames']] == want.tolist()        # across the chunks of 7 frames
    flags = {5: LISTED, 10: DUPLICATE, 11: DUPLICATE, 20: BLANK, 30: MISSING | DUPLICATE, 31: MISSING | DUPLICATE}
    assert [f['flags'] for f in on_disk['frames']] == [flags.get(i, 0) for i in range(40)]
    assert [(g['start'], g['T'], g['K'], g['F'], g['status'], g['positions']) for g in on_disk['gaps']] == [
        (5, 1, 3, 3, 'fill', [5]), (10, 2, 3, 3, 'fill', [10, 11]), (20, 1, 3, 3, 'fill', [20]), (30, 2, 3, 3, 'fill', [30, 31])]
    assert on_disk['settings']['detect'] == ['blank', 'dup', 'missing'] and on_disk['settings']['max_T'] == 2
    text = capsys.readouterr().out
    assert text.count('gap at frame') == 4 and 'gap at frame 30: T=2 K=3 F=3 fill' in text and '40 frames, 6 flagged, 4 gaps' in text
    # the default detects what the source lacks and nothing else; --max_T 1 leaves the two-frame gap
    report = restore_cli.main(common + ['--output_dir', str(tmp_path / 'out2'), '--max_T', '1'])
    assert [(g['start'], g['status']) for g in report['gaps']] == [(30, 'too_long')]
    assert [f['flags'] for f in report['frames']] == [MISSING if i in (30, 31) else 0 for i in range(40)]
    for bad in (['--gaps', '41-42'], ['--gaps', '9-3'], ['--detect', 'static'], ['--dup_tol', '255']):
        with pytest.raises(SystemExit) as e:
            restore_cli.main(common + ['--output_dir', str(tmp_path / 'out3')] + bad)
        assert e.value.code not in (0, None), bad


# ---------------------------------------------------------------------------------------------------------------- the C ABI's refusals

P = 16                          # a pointer that is never followed: a refused call reads none of its buffers
EINVAL = -1


def _call(frames=P, n=4, frame_bytes=64, tol=0, stats=P, workspace=P):
    return [frames, n, frame_bytes, tol, stats, workspace]


# (arguments, the argument the message names)
REFUSALS = [
    (_call(frames=None), 'frames'), (_call(stats=None), 'stats'), (_call(workspace=None), 'workspace'),
    (_call(n=0), 'n_frames'), (_call(n=-3), 'n_frames'),
    (_call(frame_bytes=0), 'frame_bytes'), (_call(frame_bytes=-64), 'frame_bytes'), (_call(frame_bytes=1 << 31), 'frame_bytes'),
    (_call(frame_bytes=1 << 40), 'frame_bytes'),
    (_call(tol=-1), 'tol'), (_call(tol=255), 'tol'),
    (_call(n=(1 << 20) + 1, frame_bytes=1 << 20), 'n_frames x frame_bytes'), (_call(n=1 << 62, frame_bytes=(1 << 31) - 1), 'n_frames x frame_bytes'),
    (_call(n=(1 << 40) + 1, frame_bytes=1), 'n_frames x frame_bytes'),
    (_call(stats=P + 4), 'aligned'), (_call(workspace=P + 2), 'aligned'),
]


def _answers(lib_path):
    """Run in a child process that sees no device: (return code, message) for REFUSALS -- calls that end before any launch -- and the
    workspace query's answers for the same sizes."""
    L = ctypes.CDLL(lib_path)
    for name, (restype, argtypes) in _native.signatures().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    out = []
    for args, _ in REFUSALS:
        rc = L.tai_frame_scan(*args, None)
        out.append([rc, L.tai_sepconv_last_error().decode(), L.tai_frame_scan_workspace_bytes(args[1], args[2])])
    return out


def test_every_refusal_returns_the_error_and_names_the_argument_without_a_device():
    _native.verify(_native.LIB_PATH)
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1')
    child = subprocess.run([sys.executable, os.path.abspath(__file__), '--answers', _native.LIB_PATH], env=env, capture_output=True, text=True,
                           timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    got = json.loads(child.stdout)
    assert len(got) == len(REFUSALS)
    for (args, word), (rc, message, query) in zip(REFUSALS, got):
        assert rc == EINVAL and message.startswith('frame_scan: ') and word in message, (args, rc, message)
        sizes_refused = word in ('n_frames', 'frame_bytes', 'n_frames x frame_bytes')
        assert (query == EINVAL) if sizes_refused else (query == 4 * 1 * 4 * 8), (args, query)
    # every message the launcher can give is reached
    source = open(os.path.join(_native.CSRC, 'frame_scan.hip.inc')).read()
    said = {m for _, m, _ in got}
    assert len(said) == 8 and set(re.findall(r'return "(frame_scan: [^"]*)";', source)) == said


def test_the_workspace_query_counts_segments():
    q = _native.lib().tai_frame_scan_workspace_bytes
    # one int64 per frame, segment of 256 16-byte vectors and statistic
    assert q(1, 1) == 32 and q(10, 4096) == 10 * 32 and q(10, 4096 + 15) == 10 * 32 and q(10, 4096 + 16) == 10 * 2 * 32
    assert q(256, 240 * 320 * 3) == 256 * 57 * 32 and q(512, 128 * 128) == 512 * 4 * 32
    assert q(1, (1 << 31) - 1) == (1 << 19) * 32 and q(1 << 40, 1) == (1 << 40) * 32


# ---------------------------------------------------------------------------------------------------------------- header, library

THREADS, RUN, VEC_BYTES, GRID_CAP = 256, 8, 16, 1 << 14            # restated; tests/test_gpu_frame_scan.py builds its shapes from them
SEG_BYTES, LANE_BYTES = THREADS * VEC_BYTES, VEC_BYTES + 1


def test_the_header_declares_the_entries_and_the_launch_constants_are_the_sources():
    header = open(os.path.join(ROOT, 'include', 'tai_sepconv.h')).read()
    assert {'tai_frame_scan', 'tai_frame_scan_workspace_bytes'} <= set(_native.declared_symbols())
    assert 'long long tai_frame_scan_workspace_bytes(long long n_frames, long long frame_bytes);' in header
    V, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    sigs = _native.signatures()
    assert sigs['tai_frame_scan'] == (I, [V, LL, LL, I, V, V, V]) and sigs['tai_frame_scan_workspace_bytes'] == (LL, [LL, LL])
    L = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(L, 'tai_frame_scan') and hasattr(L, 'tai_frame_scan_workspace_bytes')
    L.tai_sepconv_version.restype = ctypes.c_int
    assert L.tai_sepconv_version() >= 880
    assert os.path.join(_native.CSRC, 'frame_scan.hip.inc') in _native.sources() and os.path.join(_native.CSRC, 'capi_scan.inc') in _native.sources()
    source = open(os.path.join(_native.CSRC, 'frame_scan.hip.inc')).read()
    for line in ('constexpr int THREADS = %d;' % THREADS, 'constexpr int RUN = %d;' % RUN, 'constexpr int VEC_BYTES = %d;' % VEC_BYTES,
                 'constexpr long long SEG_BYTES = THREADS * VEC_BYTES;', 'constexpr int LANE_BYTES = VEC_BYTES + 1;',
                 'constexpr long long GRID_CAP = 1LL << 14;', 'constexpr long long MAX_TOTAL_BYTES = 1LL << 40;'):
        assert line in source, line
    # a lane's 32-bit accumulators at all-255 input; 8 frames x 4 statistics x 8 threads is the workgroup
    assert LANE_BYTES * 255 * 255 < 2 ** 32 and THREADS * LANE_BYTES * 255 * 255 < 2 ** 63 and RUN * 4 * 8 == THREADS
    assert 'atomic' not in source.replace('No atomics', '') and 'asm' not in source
    main = open(_native.MAIN_SOURCE).read()
    assert '#include "frame_scan.hip.inc"' in main and '#include "capi_scan.inc"' in main


if __name__ == '__main__':
    if sys.argv[1:2] == ['--answers'] and len(sys.argv) == 3:
        assert os.environ.get('HIP_VISIBLE_DEVICES') == '-1' and os.environ.get('ROCR_VISIBLE_DEVICES') == '-1'
        print(json.dumps(_answers(sys.argv[2])))
