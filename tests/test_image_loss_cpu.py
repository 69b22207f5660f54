"""The L1 / Charbonnier image loss without a GPU (train.py --image_loss; losses.ImageLoss; include/tai_sepconv.h tai_image_loss): the numpy
restatement of the definition (image_loss_ref.py) against float64 autograd of a torch composition (for L2: today's MSELoss + losses.GDL),
the module's CPU path, the flags' refusals, one CPU update per kind, and the header / library."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_loss_ref as ref  # noqa: E402

import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import _native, synthetic  # noqa: E402
from video_frame_inpainting_amd.ablations import BidirectionalSimpleAverageFillInModel  # noqa: E402
from video_frame_inpainting_amd.environments import create_training_environment  # noqa: E402
from video_frame_inpainting_amd.losses import GDL, ImageLoss  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-3
SHAPES = [(15, 41, 17), (4, 128, 128), (2, 3, 2, 33, 20)]

# The restatement rounds x, y (2^-25 each: values around [0, 1]) and d (2^-25 relative) to fp32; the composition it is held against keeps
# the same fp32 inputs exact in float64.
TERM_REL = 2.0 ** -24 * 4                                  # point and gdl, relative
GRAD_REL = {0: 2.0 ** -21, 1: 2.0 ** -21,                  # of the map's maximum magnitude
            2: 3 * 2.0 ** -25 / EPS + 2.0 ** -21}          # rho' = d / sqrt(d^2 + eps^2) has slope 1 / eps at 0: d's rounding is amplified


def _composition(pred32, gt32, kind):
    """float64 torch composition on the same fp32 values -> (point, gdl, grad of point + gdl), numpy float64."""
    p = torch.from_numpy(pred32).double().requires_grad_()
    x, y = (p + 1) / 2, (torch.from_numpy(gt32).double() + 1) / 2
    if kind == 0:
        point = torch.nn.MSELoss()(x, y)
    elif kind == 1:
        point = (x - y).abs().mean()
    else:
        e2 = float(np.float32(EPS) * np.float32(EPS))       # the definition's constant: eps * eps in fp32
        point = torch.sqrt((x - y) * (x - y) + e2).mean()
    gdl = GDL()(x, y)
    (point + gdl).backward()
    return float(point.detach()), float(gdl.detach()), p.grad.numpy()


def _check(got_point, got_gdl, got_grad, point, gdl, grad, kind, what):
    scale = np.abs(grad).max()
    d_grad = np.abs(np.asarray(got_grad, np.float64) - grad).max()
    print('%s: point %.9e (rel %.2e) gdl %.9e (rel %.2e) grad max %.3e diff %.2e of it' % (
        what, point, abs(got_point - point) / max(abs(point), 1e-300), gdl, abs(got_gdl - gdl) / max(abs(gdl), 1e-300), scale,
        d_grad / max(scale, 1e-300)))
    assert abs(got_point - point) <= TERM_REL * abs(point)
    assert abs(got_gdl - gdl) <= TERM_REL * abs(gdl)
    assert d_grad <= GRAD_REL[kind] * scale


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', [0, 1, 2], ids=ref.KIND_NAMES)
def test_restatement_and_cpu_module_match_the_float64_composition(kind, shape):
    for inputs in ref.KINDS:
        pred, gt = ref.make_pair(inputs, shape, 23 + shape[-1])
        point, gdl, grad = _composition(pred, gt, kind)
        want = ref.image_loss_ref(pred, gt, kind, EPS)
        assert want['grad'].dtype == np.float32 and want['grad'].shape == pred.shape
        _check(want['point'], want['gdl'], want['grad64'], point, gdl, grad, kind, 'restatement %s %s' % (inputs, shape))
        assert want['loss'] == want['point'] + want['gdl']
        # the module's CPU path: the same fp32 terms by torch ops, float64 sums, fp32 autograd
        p = torch.from_numpy(pred).requires_grad_()
        module = ImageLoss(ref.KIND_NAMES[kind], EPS)
        loss = module(p, torch.from_numpy(gt))
        assert loss.dtype == torch.float32 and loss.dim() == 0
        loss.backward()
        (m_point, m_gdl), = module.last_terms
        assert not m_point.requires_grad and not m_gdl.requires_grad
        planes = module.plane_terms.numpy()
        assert planes.shape == (1,) + want['plane_terms'].shape and planes.dtype == np.float64
        # the same terms in another order, up to torch's own fp32 square root (a few words differ from numpy's by one ulp)
        np.testing.assert_allclose(planes[0], want['plane_terms'], rtol=1e-12 if kind < 2 else TERM_REL, atol=0)
        P, (H, W) = planes.shape[1], shape[-2:]
        _check(planes[0, :, 0].sum() / (P * H * W), planes[0, :, 1].sum() / (P * (H - 1) * (W - 1)), p.grad.numpy(), point, gdl, grad, kind,
               'module %s %s' % (inputs, shape))
        assert abs(float(loss.detach()) - want['loss']) <= 2.0 ** -23 * abs(want['loss'])     # the fp32 scalar
        if inputs == 'equal':                                                               # sgn(0) = 0: every d, gw, gh is 0
            assert not want['grad'].any() and not p.grad.numpy().any() and want['gdl'] == 0.0
            assert want['point'] == 0.0 if kind < 2 else abs(want['point'] - EPS) <= 2.0 ** -22 * EPS          # rho(0) = sqrt(eps * eps)


def test_grid_sums_do_not_depend_on_their_order_and_every_sign_count_occurs():
    """On grid inputs every term is a multiple of 2^-33 below 2: float64 sums of up to 2^18 of them are exact, whatever the order."""
    for shape in ((15, 41, 17), (4, 128, 128)):
        pred, gt = ref.make_pair('grid', shape, 5)
        rs = np.random.RandomState(1)
        for kind in (0, 1, 2):
            want = ref.image_loss_ref(pred, gt, kind, EPS)
            for terms in (want['rho'], np.abs(want['gw']), np.abs(want['gh'])):
                t = terms.astype(np.float64).ravel()
                assert np.all(t < 2.0) and np.all(t * 2.0 ** 33 == np.round(t * 2.0 ** 33))
                total = t.sum()
                assert total == t[::-1].sum() == t[rs.permutation(t.size)].sum() == float(sum(float(c.sum()) for c in np.array_split(t, 37)))
            assert want['S'].min() == -4 and want['S'].max() == 4
            assert (want['gw'] == 0).mean() > 0.05 and (want['gh'] == 0).mean() > 0.05 and (want['rho'] == want['rho'].min()).mean() > 0.3


def test_three_predictions_a_permuted_view_and_float64():
    preds = [ref.make_pair('uniform', (2, 3, 9, 11), s)[0] for s in (1, 2, 3)]
    gt = ref.make_pair('uniform', (2, 3, 9, 11), 4)[1]
    module = ImageLoss('charbonnier', EPS)
    ts = tuple(torch.from_numpy(p).requires_grad_() for p in preds)
    losses = module(ts, torch.from_numpy(gt))
    assert isinstance(losses, tuple) and len(losses) == 3 and len(module.last_terms) == 3 and module.plane_terms.shape == (3, 6, 2)
    sum(losses).backward()
    for t, p, loss in zip(ts, preds, losses):
        want = ref.image_loss_ref(p, gt, 2, EPS)
        assert abs(float(loss.detach()) - want['loss']) <= 2.0 ** -23 * want['loss']
        assert np.abs(t.grad.numpy() - want['grad64']).max() <= 2.0 ** -21 * np.abs(want['grad64']).max()
    # a permuted view: the loss does not care how planes are ordered, the gradient comes back in the view's shape
    base = torch.from_numpy(preds[0])
    view = base.permute(1, 0, 2, 3).requires_grad_()
    loss = ImageLoss('l1')(view, torch.from_numpy(gt).permute(1, 0, 2, 3))
    loss.backward()
    assert view.grad.shape == view.shape
    want = ref.image_loss_ref(preds[0], gt, 1)
    assert np.abs(view.grad.permute(1, 0, 2, 3).numpy() - want['grad64']).max() <= 2.0 ** -21 * np.abs(want['grad64']).max()
    # float64 tensors: the same definition in float64
    p64 = torch.from_numpy(preds[0]).double().requires_grad_()
    loss64 = ImageLoss('l2')(p64, torch.from_numpy(gt).double())
    assert loss64.dtype == torch.float64
    point, gdl, _ = _composition(preds[0], gt, 0)
    assert abs(float(loss64.detach()) - (point + gdl)) <= 1e-14


def test_the_module_refuses_what_it_cannot_take_and_carries_no_state():
    assert not ImageLoss().state_dict() and not list(ImageLoss().parameters()) and not list(ImageLoss().buffers())
    assert ImageLoss().kind == 'charbonnier' and ImageLoss().eps == 1e-3
    for shape in [(1, 1, 1, 32), (1, 1, 32, 1)]:
        x = torch.zeros(shape)
        with pytest.raises(ValueError):
            ImageLoss()(x, x)
    with pytest.raises(ValueError):
        ImageLoss()(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 9))
    with pytest.raises(ValueError):
        ImageLoss()((torch.zeros(1, 8, 8),) * 4, torch.zeros(1, 8, 8))
    with pytest.raises(ValueError):
        ImageLoss('huber')
    for eps in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            ImageLoss('charbonnier', eps)


# ---------------------------------------------------------------------------------------------------------------- flags, environment

def _main(extra):
    import train
    return train.main(['--name', 'x', '--K', '3', '--T', '2', '--F', '3', '--c_dim', '1', '--image_size', '32', '--batch_size', '2',
                       '--model_key', 'MCNet_gray'] + extra)


def test_the_flags_parse_and_bad_values_are_refused_before_anything_runs(monkeypatch):
    import train
    from video_frame_inpainting_amd.options import TrainOptions
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)         # the option parser's own check; nothing else is reached
    seen = []
    monkeypatch.setattr(train, '_run', lambda opt, stop: seen.append((opt.image_loss, opt.charbonnier_eps)))
    _main([])
    _main(['--image_loss', 'l1'])
    _main(['--image_loss', 'charbonnier', '--charbonnier_eps', '0.01'])
    assert seen == [('l2', 1e-3), ('l1', 1e-3), ('charbonnier', 0.01)]
    monkeypatch.setattr(train, '_run', lambda *a, **k: pytest.fail('the run was started'))
    for extra in (['--image_loss', 'huber'], ['--charbonnier_eps', '0'], ['--charbonnier_eps', 'nan'], ['--charbonnier_eps', '-1'],
                  ['--charbonnier_eps', 'inf'], ['--image_loss', 'charbonnier', '--charbonnier_eps', '0', '--resumable']):
        with pytest.raises(SystemExit) as e:
            _main(extra)
        assert e.value.code not in (0, None), extra
    with pytest.raises(ValueError, match='image_loss'):
        _env('unused', 'unused', image_loss='huber')
    with pytest.raises(ValueError, match='charbonnier_eps'):
        _env('unused', 'unused', image_loss='charbonnier', charbonnier_eps=0.0)


K, T, F = 3, 2, 3
_CLIPS = torch.from_numpy(synthetic.make_clips(2, K + T + F, 1, 32, 32, 77))


def _env(root, name, model='mcnet', **kw):
    torch.manual_seed(0)
    np.random.seed(0)
    net = vfi.MCNetFillInModel(4, 1, 3) if model == 'mcnet' else BidirectionalSimpleAverageFillInModel(4, 1, 3)
    return create_training_environment(net, 1, str(root), name, K, T, F, [32, 32], 1.0, 0.02, 1e-3, 0.5, 4, 2, 3, [0, 0], device='cpu', **kw)


def _update(env):
    env.K, env.T, env.F = K, T, F
    env.train()
    env.set_train_inputs(_CLIPS[:, :K], _CLIPS[:, K + T:], _CLIPS[:, K:K + T])
    env.forward_train()
    env.optimize_parameters()


@pytest.mark.parametrize('kind', ref.KIND_NAMES)
@pytest.mark.parametrize('model', ['mcnet', 'bidirectional'])
def test_one_cpu_update_with_each_kind(tmp_path, model, kind):
    """The separable convolution exists on the GPU only, so the three-prediction environment is driven here by the bidirectional average
    model (the same TAITrainingEnvironment, the same three outputs) and the one-prediction environment by MC-Net."""
    env = _env(tmp_path, kind, model, image_loss=kind)
    assert (env.loss_image is None) == (kind == 'l2')
    _update(env)
    errs = env.get_current_errors()
    keys = ['G_Lp', 'G_gdl'] + (['G_Lp_forward', 'G_gdl_forward', 'G_Lp_backward', 'G_gdl_backward'] if model == 'bidirectional' else [])
    print(kind, {k: errs[k] for k in keys})
    assert all(np.isfinite(errs[k]) and errs[k] > 0 for k in keys)
    assert sorted(errs) == sorted(keys + ['D_fake', 'D_real', 'G_GAN', 'G_loss'])
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in env.generator.parameters() if p.requires_grad)
    gt = _CLIPS[:, K:K + T].numpy()
    for suffix, out in (('', 'pred'), ('_forward', 'pred_forward'), ('_backward', 'pred_backward')):
        if 'G_Lp' + suffix not in keys:
            continue
        want = ref.image_loss_ref(env.gen_output[out].detach().numpy(), gt, ref.KIND_NAMES.index(kind))
        # l2: today's MSELoss + GDL modules in fp32 on time-major copies; l1 / charbonnier: the definition; either way one fp32 scalar
        tol = 2.0 ** -20 if kind == 'l2' else 2.0 ** -23
        assert abs(errs['G_Lp' + suffix] - want['point']) <= tol * want['point']
        assert abs(errs['G_gdl' + suffix] - want['gdl']) <= tol * want['gdl']
    assert not env.get_current_state_dict(1, 0, 0).get('loss_image') and not hasattr(env, '_image_losses')


def test_the_default_builds_no_module_and_l2_is_the_run_without_the_flag(tmp_path):
    plain, l2 = _env(tmp_path, 'plain'), _env(tmp_path, 'l2', image_loss='l2')
    assert plain.loss_image is None and l2.loss_image is None
    _update(plain)
    _update(l2)
    a, b = plain.get_current_errors(), l2.get_current_errors()
    assert sorted(a) == sorted(b) == ['D_fake', 'D_real', 'G_GAN', 'G_Lp', 'G_gdl', 'G_loss']
    assert a['G_Lp'] == b['G_Lp'] and a['G_gdl'] == b['G_gdl']          # the same modules on the same prediction
    assert isinstance(l2.loss_Lp, torch.nn.MSELoss) and isinstance(l2.loss_gdl, GDL)


# ---------------------------------------------------------------------------------------------------------------- header, library

def test_the_header_declares_the_entry_points_and_the_library_exports_them():
    header = open(os.path.join(ROOT, 'include', 'tai_sepconv.h')).read()
    assert {'tai_image_loss', 'tai_image_loss_workspace_bytes'} <= set(_native.declared_symbols())
    flat = re.sub(r'\s*\n \*\s*', ' ', header)
    for line in ('x = (pred + 1) / 2, y = (gt + 1) / 2, in that operation order (util.inverse_transform);',
                 'kind 0 (L2): rho = d * d; rho\' = 2 * d;',
                 'kind 1 (L1): rho = |d|; rho\' = sgn(d), with sgn(0) = 0 and NaN kept;',
                 'kind 2 (Charbonnier): s = sqrt(d * d + e2) with e2 = eps * eps computed once in fp32; rho = s; rho\' = d / s;',
                 'gw(r, c) = (x[r,c] - x[r,c+1]) - (y[r,c] - y[r,c+1]) for 1 <= r <= H-1, 0 <= c <= W-2;',
                 'gh(r, c) = (x[r,c] - x[r-1,c]) - (y[r,c] - y[r-1,c]) for 1 <= r <= H-1, 1 <= c <= W-1;',
                 'grad[r,c] = fp32( (double)rho\'(d) * cp + S * cg )',
                 'cp = 0.5 / ((double)P * H * W)', 'cg = 0.5 / ((double)P * (H-1) * (W-1))'):
        assert re.sub(r'\s+', ' ', line) in re.sub(r'\s+', ' ', flat), line
    assert 'long long tai_image_loss_workspace_bytes(int npred, long long planes, int H, int W);' in header
    L = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(L, 'tai_image_loss') and hasattr(L, 'tai_image_loss_workspace_bytes')
    L.tai_sepconv_version.restype = ctypes.c_int
    assert L.tai_sepconv_version() >= 820
    # the workspace query is host code: two float64 partials per prediction, plane and 16 x 64 tile
    L.tai_image_loss_workspace_bytes.restype = ctypes.c_longlong
    L.tai_image_loss_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    assert L.tai_image_loss_workspace_bytes(3, 160, 128, 128) == 3 * 160 * 8 * 2 * 2 * 8
    assert L.tai_image_loss_workspace_bytes(1, 1, 2, 2) == 16
    for bad in ((0, 1, 8, 8), (4, 1, 8, 8), (1, 0, 8, 8), (1, 1, 1, 8), (1, 1, 8, 1), (1, 1 << 20, 1 << 10, 1 << 10), (1, 1, 1 << 16, 1 << 15),
                (1, 1 << 38, 2, 2), (1, 1 << 31, 2, 2)):
        assert L.tai_image_loss_workspace_bytes(*bad) < 0, bad
