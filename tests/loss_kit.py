"""What the five fused-loss GPU test files (test_gpu_{ssim,image,lap,temporal,census}_loss.py) share: bit views and relative errors, the
tiny model's train.py runs and how their output is read, and the three test bodies that are the same for every loss up to its flags and
keys -- graph replay against eager, straight against split, graph_step; and, for test_loss_terms_cpu.py and test_gpu_loss_terms.py,
loss_G's fold written out.  A plain module, imported the way sepconv_cases.py is."""
import gc
import re

import numpy as np
import torch

DEV = torch.device('cuda:0')


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _rel(a, b):
    """Largest relative error of ``a`` against ``b``; equal entries count as 0 (for finite values that is what the quotient gives)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.where(a == b, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-300))))


def _device(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def check_graph_replay(make_module, sp, sg, second, gt2, want_grads, single=False):
    """Forward and backward captured in one graph on the static leaves ``sp`` (a list; they hold the first inputs) and ``sg``, replayed
    on the inputs ``second`` / ``gt2`` (numpy): losses and gradients equal an eager run's, and the gradients ``want_grads`` (the
    restatement's) bit for bit.  ``single``: the module takes one prediction and returns one loss, else a tuple of each."""
    run = (lambda module, ps, g: [module(ps[0], g)]) if single else (lambda module, ps, g: list(module(tuple(ps), g)))
    total = (lambda losses: losses[0]) if single else sum
    module = make_module()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                     # warm-up outside the capture
        total(run(module, sp, sg)).backward()
    torch.cuda.current_stream().wait_stream(side)
    for p in sp:
        p.grad = None
    torch.cuda.synchronize()
    gc.collect()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        losses = run(module, sp, sg)
        total(losses).backward()
        losses = [x.detach() for x in losses]                                         # nothing with history outlives the capture
    with torch.no_grad():
        for p, a in zip(sp, second):
            p.copy_(torch.from_numpy(np.array(a)))
        sg.copy_(torch.from_numpy(np.array(gt2)))
    graph.replay()
    torch.cuda.synchronize()
    eager_p = [_device(a).requires_grad_() for a in second]
    eager = run(make_module(), eager_p, _device(gt2))
    total(eager).backward()
    for i in range(len(sp)):
        assert float(losses[i]) == float(eager[i].detach())
        assert torch.equal(sp[i].grad.view(torch.int32), eager_p[i].grad.view(torch.int32))
        assert np.array_equal(_bits(sp[i].grad.cpu().numpy()), _bits(want_grads[i]))


# ---------------------------------------------------------------------------------------------------------------- drivers

SPEC = '{"class": "TAIFillInModel", "args": [4, 1, 3, 51], "kwargs": {"num_block": 5, "kf_dim": 2}}'
MCNET = '{"class": "MCNetFillInModel", "args": [4, 1, 3], "kwargs": {}}'          # MCNet_gray at reduced width
K, T, F, SIZE = 3, 2, 3, 32


def _train(tmp_path, capsys, name, max_iter, extra, model=SPEC):
    import train
    capsys.readouterr()
    train.main(['--name', name, '--K', str(K), '--T', str(T), '--F', str(F), '--c_dim', '1', '--image_size', str(SIZE), '--model_key', model,
                '--checkpoints_dir', str(tmp_path / 'ckpt'), '--batch_size', '2', '--max_iter', str(max_iter), '--print_freq', '1',
                '--df_dim', '8', '--synthetic', '4'] + list(extra))
    return capsys.readouterr().out


def _states(out):
    return dict((int(i), s) for i, s in re.findall(r'^iter (\d+) .* state=([0-9a-f]{16})$', out, re.M))


def _terms(out, n, keys, lo, hi):
    """{key: [value per printed update]}; asserts each key is printed on every line, finite and inside (lo, hi)."""
    found = {}
    for key in keys:
        values = [float(v) for v in re.findall(r' %s=(\S+)' % key, out)]
        assert len(values) == n, (key, out)
        assert all(np.isfinite(v) and lo < v < hi for v in values), (key, values)
        found[key] = values
    return found


def _generator(tmp_path, name):
    snap = torch.load(str(tmp_path / 'ckpt' / name / 'model_latest.ckpt'), map_location='cpu', weights_only=False)
    return snap['generator']


def check_straight_against_split(tmp_path, capsys, extra, terms):
    """Four updates in one run against two runs of two (the second resumes): the same state digests, all four different; ``terms(out,
    n)`` is the file's reading of its keys."""
    straight = _train(tmp_path, capsys, 'A', 4, extra)
    first = _train(tmp_path, capsys, 'B', 2, extra)
    second = _train(tmp_path, capsys, 'B', 4, extra)
    assert 'carries no run_state' not in second and 'falling back' not in second
    sa, sb1, sb2 = _states(straight), _states(first), _states(second)
    print('straight', sa, 'split', sb1, sb2)
    assert sorted(sa) == [1, 2, 3, 4] and sorted(sb1) == [1, 2] and sorted(sb2) == [3, 4]
    assert sa == {**sb1, **sb2} and len(set(sa.values())) == 4
    print(terms(straight, 4))


def check_graph_step(tmp_path, capsys, flags, terms, changing=None, replays_differ=False):
    """Updates 1-2 eager, 3 captured and replayed, 4 replayed: the launch is part of the captured update.  The keys ``changing`` (default:
    all) take more than one value; ``replays_differ``: some key differs between the two replays (new inputs and new weights were read)."""
    found = terms(_train(tmp_path, capsys, 'g', 4, ['--graph_step'] + list(flags)), 4)
    print(found)
    assert all(len(set(found[key])) > 1 for key in (changing or found))
    if replays_differ:
        assert any(v[2] != v[3] for v in found.values())


# ---------------------------------------------------------------------------------------------------------------- loss_G's fold

TERM_WEIGHTS = {'ssim_weight': 0.2, 'lap_weight': 0.5, 'temporal_weight': 0.3, 'census_weight': 0.7}          # all different: a mixed-up weight shows


def check_fold(env, image_loss, on, three):
    """After one update of ``env`` (``on``: the keys of TERM_WEIGHTS that are on; ``three``: TAITrainingEnvironment): loss_G's bits are
    those of the fp32 left-to-right fold of the environment's value attributes, written out here addend by addend and not read from the
    environment's own table; no tensor with autograd history stays on the environment outside the step outputs; the printed keys are the
    ones listed here."""
    w = {k: (v if k in on else 0.0) for k, v in TERM_WEIGHTS.items()}
    a, b = env.alpha, env.beta
    g = torch.zeros(1, device=env.loss_G.device)
    if image_loss == 'l2':
        g = g + a * (env.Lp + env.gdl)
        g = g + b * env.L_GAN
    else:
        g = g + a * env.image
        g = g + b * env.L_GAN
        if three:
            g = g + a * (env.image_forward + env.image_backward)
    if w['ssim_weight']:
        g = g + w['ssim_weight'] * env.ssim
    if w['lap_weight']:
        g = g + w['lap_weight'] * env.lap
    if w['temporal_weight']:
        g = g + w['temporal_weight'] * env.temporal
        if three:
            g = g + w['temporal_weight'] * (env.temporal_forward + env.temporal_backward)
    if w['census_weight']:
        g = g + w['census_weight'] * env.census
        if three:
            g = g + w['census_weight'] * (env.census_forward + env.census_backward)
    if three and image_loss == 'l2':
        g = g + a * (env.Lp_forward + env.Lp_backward + env.gdl_forward + env.gdl_backward)
    if three and w['ssim_weight']:
        g = g + w['ssim_weight'] * (env.ssim_forward + env.ssim_backward)
    if three and w['lap_weight']:
        g = g + w['lap_weight'] * (env.lap_forward + env.lap_backward)
    print(image_loss, sorted(on), 'loss_G', float(env.loss_G.detach()), 'fold', float(g.detach()))
    assert g.dtype == env.loss_G.dtype == torch.float32 and g.shape == env.loss_G.shape
    assert torch.equal(g.detach().view(torch.int32), env.loss_G.detach().view(torch.int32))

    def with_history(v):
        return any(t.grad_fn is not None for t in (v.values() if isinstance(v, dict) else [v]) if torch.is_tensor(t))
    alive = sorted(k for k, v in vars(env).items() if with_history(v))
    assert 'loss_G' in alive and set(alive) <= set(env._STEP_OUTPUTS), (alive, env._STEP_OUTPUTS)

    ends = ['', '_forward', '_backward'] if three else ['']
    keys = ['D_fake', 'D_real', 'G_GAN', 'G_loss'] + ['G_' + name + end for name in ('Lp', 'gdl') for end in ends]
    keys += ['G_' + k[:-len('_weight')] + end for k in TERM_WEIGHTS if w[k] for end in ends]
    errors = env.get_current_errors()
    assert sorted(errors) == sorted(keys)
    assert all(np.isfinite(v) for v in errors.values())
