"""train.py --resumable on the GPU: the state digest kernel against its numpy restatement, and a run cut into two processes against
the same run made in one -- synthetic clips, a video list (host and device clip pipeline), a stop request, --graph_step.  Every
comparison is bit equality or an exact integer."""
import os
import re
import signal
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import state_digest_ref as ref  # noqa: E402

from video_frame_inpainting_amd import environments, run_state  # noqa: E402

pytestmark = pytest.mark.gpu

SPEC = '{"class": "TAIFillInModel", "args": [4, 1, 3, 51], "kwargs": {"num_block": 5, "kf_dim": 2}}'
K, T, F, SIZE = 3, 2, 3, 32
DEV = 'cuda:0'


# ---------------------------------------------------------------------------------------------------------------- digest kernel

def _table():
    g = torch.Generator().manual_seed(11)
    table = []
    for n in (1, 3, 4, 5, 63, 64, 65, 1000003):
        table.append(torch.randn(n, generator=g))
        table.append(torch.randint(-2 ** 62, 2 ** 62, (n,), generator=g))
    table.insert(5, torch.zeros(0))
    return table


def _on_device(table, offset_views=True):
    """The same values on the GPU; every other fp32 entry a view that starts 4 bytes behind a 16-byte boundary."""
    out = []
    for i, t in enumerate(table):
        if offset_views and t.dtype == torch.float32 and t.numel() and i % 4 == 0:
            buf = torch.empty(t.numel() + 8, device=DEV)
            first = 1 + (16 - buf.data_ptr() % 16) % 16 // 4                            # the word behind a 16-byte boundary
            view = buf[first:first + t.numel()]
            assert view.data_ptr() % 16 == 4
            view.copy_(t)
            out.append(view)
        else:
            out.append(t.to(DEV))
    return out


def test_digest_kernel_equals_the_numpy_restatement():
    table = _table()
    want = ref.digest(table)
    dev = _on_device(table)
    assert any(t.data_ptr() % 16 == 4 for t in dev) and any(t.numel() == 0 for t in dev)
    have = run_state.digest_tensors(dev)
    print('digest %016x, restatement %016x' % (have, want))
    assert have == want
    assert run_state.digest_tensors(dev) == want                                        # two launches agree
    assert run_state.digest_tensors(_on_device(table, offset_views=False)) == want      # other addresses, other alignment
    for seg_words in (4, 64, 1 << 20):                                                  # other segments, another grid
        assert run_state.digest_tensors(dev, seg_words=seg_words) == want
    mixed = list(dev)
    mixed[3], mixed[-1] = table[3], table[-1]                                           # entries held on the host
    assert run_state.digest_tensors(mixed) == want
    assert run_state.digest_tensors(table) == want                                      # ... all of them


def test_digest_kernel_sensitivity():
    g = torch.Generator().manual_seed(12)
    a, b = torch.randn(100000, generator=g), torch.randn(37, generator=g)
    base = run_state.digest_tensors([a.to(DEV), b.to(DEV)])
    assert base == ref.digest([a, b])

    def both(x, y):
        d = run_state.digest_tensors([x.to(DEV), y.to(DEV)])
        assert d == ref.digest([x, y])
        return d
    flipped = a.clone()
    flipped.view(torch.int32)[70001] ^= 1 << 17
    assert both(flipped, b) != base
    swapped = a.clone()
    swapped[[10, 50000]] = a[[50000, 10]]
    assert both(swapped, b) != base
    assert both(a[:-1], torch.cat([a[-1:], b])) != base                                # a word moves to the next tensor
    z = torch.zeros(8)
    nz = z.clone()
    nz[3] = -0.0
    assert both(z, b) != both(nz, b)


# ---------------------------------------------------------------------------------------------------------------- straight against split

def _args(tmp_path, name, max_iter, extra):
    return ['--name', name, '--K', str(K), '--T', str(T), '--F', str(F), '--c_dim', '1', '--image_size', str(SIZE), '--model_key', SPEC,
            '--checkpoints_dir', str(tmp_path / 'ckpt'), '--batch_size', '2', '--max_iter', str(max_iter), '--print_freq', '1',
            '--df_dim', '8', '--resumable', '--sample_KTF', '--val_synthetic', '3', '--validate_freq', '1'] + list(extra)


def _train(tmp_path, capsys, name, max_iter, extra):
    import train
    capsys.readouterr()
    train.main(_args(tmp_path, name, max_iter, extra))
    return capsys.readouterr().out


def _latest(tmp_path, name):
    return torch.load(str(tmp_path / 'ckpt' / name / 'model_latest.ckpt'), map_location='cpu', weights_only=False)


def _flat(snap):
    out = {}
    for part in ('generator', 'discriminator'):
        out.update((part + '.' + k, v) for k, v in snap[part].items())
    for part in ('optimizer_G', 'optimizer_D'):
        for i, st in snap[part]['state'].items():
            assert set(st) == {'step', 'exp_avg', 'exp_avg_sq'}
            out.update(('%s.%s.%s' % (part, i, k), torch.as_tensor(v)) for k, v in st.items())
    us = snap['run_state']['u']
    assert us and all(u is not None for u in us.values())
    out.update(('u.' + k, v) for k, v in us.items())
    return out


def _assert_same_run(a, b):
    fa, fb = _flat(a), _flat(b)
    assert set(fa) == set(fb) and a['updates'] == b['updates']
    different = [k for k in fa if not torch.equal(fa[k], fb[k])]
    assert not different, 'first of %d differing tensors: %s' % (len(different), different[0])
    assert a['run_state']['digest'] == b['run_state']['digest']
    assert (a['sum_avg_psnr_err'], a['sum_avg_ssim_err']) == (b['sum_avg_psnr_err'], b['sum_avg_ssim_err'])


def _states(out):
    return dict((int(i), s) for i, s in re.findall(r'^iter (\d+) .* state=([0-9a-f]{16})$', out, re.M))


def _straight_and_split(tmp_path, capsys, tag, extra, n=4, m=2):
    out_a = _train(tmp_path, capsys, tag + 'A', n, extra)
    out_b1 = _train(tmp_path, capsys, tag + 'B', m, extra)
    out_b2 = _train(tmp_path, capsys, tag + 'B', n, extra)
    assert 'carries no run_state' not in out_b2 and 'falling back' not in out_b2
    sa, sb1, sb2 = _states(out_a), _states(out_b1), _states(out_b2)
    assert sorted(sa) == list(range(1, n + 1)) and sorted(sb1) == list(range(1, m + 1)) and sorted(sb2) == list(range(m + 1, n + 1))
    print(tag, 'straight', sa, 'split', sb1, sb2)
    a, b = _latest(tmp_path, tag + 'A'), _latest(tmp_path, tag + 'B')
    assert a['updates'] == n
    _assert_same_run(a, b)
    assert sa == {**sb1, **sb2}                                                       # readable from the logs alone
    assert len(set(sa.values())) == n
    return a


def test_straight_against_split_synthetic(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _straight_and_split(tmp_path, capsys, 'syn', ['--synthetic', '4'])


def _video_list(tmp_path):
    rng = np.random.RandomState(21)
    lines = []
    for i in range(7):                      # three batches of two per epoch: the split at update 2 is inside epoch 0, update 4 in epoch 1
        base = rng.randint(0, 256, (40, 48, 3)).astype(np.uint8)
        np.save(tmp_path / ('clip%d.npy' % i), np.stack([np.roll(base, 2 * t, axis=1) for t in range(12 + i)]))
        lines.append(str(tmp_path / ('clip%d.npy' % i)))
    (tmp_path / 'list.txt').write_text('\n'.join(lines) + '\n')
    return str(tmp_path / 'list.txt')


def test_straight_against_split_video_list_host_and_device_pipeline(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    lst = ['--train_video_list_path', _video_list(tmp_path), '--num_threads', '0']
    host = _straight_and_split(tmp_path, capsys, 'host', lst)
    dev = _straight_and_split(tmp_path, capsys, 'dev', lst + ['--device_preprocess'])
    _assert_same_run(host, dev)                                                        # the two clip pipelines stay bit-equal
    assert host['run_state']['ranks'][0]['data']['kind'] == 'sampler'
    assert (host['run_state']['ranks'][0]['data']['epoch'], host['run_state']['ranks'][0]['data']['consumed']) == (1, 1)


# ---------------------------------------------------------------------------------------------------------------- stop request

def test_stop_request_saves_after_the_update_in_flight_and_the_run_continues_exactly(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    syn = ['--synthetic', '4']
    out_a = _train(tmp_path, capsys, 'A', 4, syn)
    before = {s: signal.getsignal(s) for s in (signal.SIGTERM, signal.SIGINT)}
    calls = []
    real = environments.BaseTrainingEnvironment.train_step

    def train_step(self, *a, **k):
        calls.append(1)
        if len(calls) == 2:
            signal.raise_signal(signal.SIGTERM)                                        # during update 2
        return real(self, *a, **k)
    monkeypatch.setattr(environments.BaseTrainingEnvironment, 'train_step', train_step)
    out_1 = _train(tmp_path, capsys, 'B', 4, syn)                                       # returns normally
    monkeypatch.setattr(environments.BaseTrainingEnvironment, 'train_step', real)
    assert len(calls) == 2 and 'model_latest.ckpt holds update 2' in out_1 and 'Done.' not in out_1
    assert out_1.count('Validation (T=%d) done.' % T) == 1                             # after update 1 only: none once the flag is up
    snap = _latest(tmp_path, 'B')
    assert snap['updates'] == 2 and 'run_state' in snap
    assert {s: signal.getsignal(s) for s in before} == before
    out_2 = _train(tmp_path, capsys, 'B', 4, syn)
    assert sorted(_states(out_2)) == [3, 4] and 'Done.' in out_2
    _assert_same_run(_latest(tmp_path, 'A'), _latest(tmp_path, 'B'))
    assert {i: s for i, s in _states(out_a).items() if i > 2} == _states(out_2)
    assert {s: signal.getsignal(s) for s in before} == before

    out_w = _train(tmp_path, capsys, 'W', 4, syn + ['--max_wall_minutes', '0'])
    assert 'model_latest.ckpt holds update 1' in out_w and 'Validation' not in out_w
    snap = _latest(tmp_path, 'W')
    assert snap['updates'] == 1 and 'run_state' in snap
    assert _states(out_w)[1] == _states(out_a)[1]


# ---------------------------------------------------------------------------------------------------------------- --graph_step

def test_graph_step_straight_against_split(tmp_path, capsys, monkeypatch):
    """Straight: updates 1-2 eager, 3 captured and replayed, 4-5 replayed.  Split: 3 + 2, and the second process makes its two updates
    eagerly (the warm-up of a new process) where the straight run replayed its graph: equal bits say a replayed update is an eager one."""
    monkeypatch.chdir(tmp_path)
    extra = ['--synthetic', '4', '--graph_step']
    args = _args(tmp_path, 'g', 5, extra)
    args.remove('--sample_KTF')                                                         # one (K, T, F): the straight run does replay
    import train
    capsys.readouterr()

    def run(name, n):
        a = list(args)
        a[a.index('--name') + 1], a[a.index('--max_iter') + 1] = name, str(n)
        train.main(a)
        return capsys.readouterr().out
    out_a, out_b1, out_b2 = run('gA', 5), run('gB', 3), run('gB', 5)
    print('graph_step straight', _states(out_a), 'split', _states(out_b1), _states(out_b2))
    _assert_same_run(_latest(tmp_path, 'gA'), _latest(tmp_path, 'gB'))
    assert _states(out_a) == {**_states(out_b1), **_states(out_b2)}
