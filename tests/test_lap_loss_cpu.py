"""The Laplacian-pyramid loss without a GPU (train.py --lap_weight; losses.LapLoss; include/tai_sepconv.h tai_lap_loss): the numpy
restatement of the definition (lap_loss_ref.py) against float64 autograd of the module's torch path, the closed forms, the refusals, the
flags, and the header / library."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lap_loss_ref as ref  # noqa: E402

import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import _native, synthetic  # noqa: E402
from video_frame_inpainting_amd.environments import create_training_environment  # noqa: E402
from video_frame_inpainting_amd.losses import ImageLoss, LapLoss  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, W, L): the smallest plane; one reduction; five levels down to 1 x 1; both clamps of a 3-row level on one pixel; odd at every level;
# odd / even mixed; a level that is not square; six levels
SHAPES = [(1, 1, 1), (2, 2, 2), (16, 16, 5), (3, 5, 2), (17, 16, 5), (13, 22, 3), (24, 40, 4), (33, 70, 6)]
_ids = lambda s: 'x'.join(map(str, s))


def _sum_bound(want):
    """Per level: n_l * 2^-53 relative, the worst case of any order of a sum of n_l non-negative terms."""
    return np.array(want['level_pixels'], np.float64) * 2.0 ** -53


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
@pytest.mark.parametrize('kind', ref.KINDS)
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['fp32', 'fp64'])
def test_restatement_matches_autograd_of_the_torch_path(dtype, kind, shape):
    """Both sides evaluate every Laplacian value with the same operations in the same order and differ only in the order of the sums of
    |L_l|; the gradient's adjoint sums are exact in float64 on both sides, so after the fp32 rounding the maps are equal."""
    H, W, L = shape
    pred32, gt32 = ref.make_pair(kind, (2, 3, H, W), 17 + W)
    pred, gt = pred32.astype(dtype), gt32.astype(dtype)
    want = ref.lap_loss_ref(pred, gt, L)
    p = torch.from_numpy(pred).requires_grad_()
    module = LapLoss(L)
    loss = module(p, torch.from_numpy(gt))
    assert loss.dim() == 0 and loss.dtype == p.dtype
    loss.backward()
    assert np.array_equal(p.grad.numpy().astype(np.float32), want['grad'])
    got = module.plane_terms.numpy()
    assert got.shape == (6, L) and got.dtype == np.float64
    rel = np.abs(got - want['plane_terms']) / np.maximum(want['plane_terms'], 1e-300)
    print('%s %s: loss %.15g; plane sums rel %.2e' % (kind, shape, want['loss'], rel.max()))
    assert np.all(rel <= _sum_bound(want)[None, :])
    # the terms and the loss: the same sums again over six planes, one division, L additions
    tol = (6 * max(want['level_pixels']) + 8) * 2.0 ** -53 if dtype is np.float64 else 2.0 ** -23
    assert abs(float(loss.detach()) - want['loss']) <= tol * max(want['loss'], 1e-300)
    assert module.last_terms.shape == (L,) and not module.last_terms.requires_grad
    np.testing.assert_allclose(module.last_terms.numpy().astype(np.float64), want['terms'], rtol=tol, atol=0)


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_equal_frames_give_zero(shape):
    H, W, L = shape
    pred, gt = ref.make_pair('equal', (2, H, W), 5)
    want = ref.lap_loss_ref(pred, gt, L)
    assert want['loss'] == 0.0 and not want['grad'].any() and not want['plane_terms'].any()
    p = torch.from_numpy(pred).requires_grad_()
    loss = LapLoss(L)(p, torch.from_numpy(gt))
    loss.backward()
    assert float(loss.detach()) == 0.0 and not p.grad.numpy().any()


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_a_constant_offset_lives_on_the_top_level_alone(shape):
    """The pyramid reproduces constants exactly: every level below the top is 0, the top is the constant c' (the fp32 difference)."""
    H, W, L = shape
    pred, gt = ref.make_pair('offset', (2, H, W), 9)
    c = np.unique(((pred + np.float32(1)) / np.float32(2) - (gt + np.float32(1)) / np.float32(2)).astype(np.float64))
    assert c.size == 1 and c[0] == 0.125
    want = ref.lap_loss_ref(pred, gt, L)
    module = LapLoss(L)
    module(torch.from_numpy(pred), torch.from_numpy(gt))
    hl, wl = ref.sizes(H, W, L)[-1]
    top = 2.0 ** (L - 1) * abs(c[0]) * hl * wl / (H * W)
    for terms in (want['terms'], module.last_terms.numpy().astype(np.float64)):
        assert not terms[:L - 1].any()
        assert abs(terms[L - 1] - top) <= 2.0 ** -23 * top
    assert abs(want['terms'][L - 1] - top) <= 4 * 2.0 ** -53 * top


@pytest.mark.parametrize('shape', [(1, 1), (3, 5), (17, 16), (24, 40)], ids=_ids)
def test_one_level_is_the_l1_point_term(shape):
    H, W = shape
    for kind in ('noise', 'smooth', 'impulse'):
        pred, gt = ref.make_pair(kind, (2, 3, max(H, 2), max(W, 2)), 3)          # ImageLoss needs H, W >= 2
        p1, p2 = torch.from_numpy(pred).requires_grad_(), torch.from_numpy(pred).requires_grad_()
        g = torch.from_numpy(gt)
        lap = LapLoss(1)
        lap(p1, g).backward()
        image = ImageLoss('l1')
        image(p2, g)
        point = float(image.plane_terms[0, :, 0].sum()) / pred.size              # from its float64 plane sums: last_terms is fp32 here
        want = ref.lap_loss_ref(pred, gt, 1)
        assert abs(want['loss'] - point) <= 1e-12
        assert abs(float(lap.last_terms[0]) - float(image.last_terms[0][0])) <= 2.0 ** -23 * point
        d = ((p2 + 1) / 2 - (g + 1) / 2).detach()
        assert torch.equal(torch.sign(p1.grad), torch.sign(d))
    if min(shape) < 2:
        pred, gt = ref.make_pair('noise', (2, H, W), 3)
        d = ((pred + np.float32(1)) / np.float32(2) - (gt + np.float32(1)) / np.float32(2)).astype(np.float64)
        assert abs(ref.lap_loss_ref(pred, gt, 1)['loss'] - np.abs(d).mean()) <= 1e-12


def test_the_gradient_is_the_slope_of_the_loss():
    """Central differences in float64 at a point without kinks nearby (a smooth plane plus noise well above the step)."""
    pred, gt = ref.make_pair('noise', (1, 13, 22), 2)
    pred, gt = pred.astype(np.float64), gt.astype(np.float64)
    want = ref.lap_loss_ref(pred, gt, 3)
    rs = np.random.RandomState(0)
    for _ in range(12):
        r, c = rs.randint(13), rs.randint(22)
        e = np.zeros_like(pred)
        e[0, r, c] = 1e-7
        slope = (ref.lap_loss_ref(pred + e, gt, 3)['loss'] - ref.lap_loss_ref(pred - e, gt, 3)['loss']) / 2e-7
        assert abs(slope - want['grad64'][0, r, c]) <= 1e-6 * np.abs(want['grad64']).max() + 1e-9


def test_refusals():
    x = torch.zeros(2, 3, 16, 16)
    for levels in (0, 7, -1, 2.0, None):
        with pytest.raises(ValueError):
            LapLoss(levels)
    with pytest.raises(ValueError):
        LapLoss(2)(x, torch.zeros(2, 3, 16, 17))
    with pytest.raises(ValueError):
        LapLoss(2)(torch.zeros(16), torch.zeros(16))
    for shape, levels in (((1, 15, 16), 5), ((1, 16, 15), 5), ((1, 1, 1), 2), ((1, 31, 64), 6), ((0, 16, 16), 2)):
        with pytest.raises(ValueError):
            LapLoss(levels)(torch.zeros(shape), torch.zeros(shape))
    LapLoss(5)(x, x)
    LapLoss(6)(torch.zeros(1, 32, 32), torch.zeros(1, 32, 32))


def test_the_module_carries_no_state():
    assert not LapLoss().state_dict() and not list(LapLoss().parameters()) and LapLoss().levels == 5


# ---------------------------------------------------------------------------------------------------------------- flags

K, T, F = 3, 2, 3
_CLIPS = torch.from_numpy(synthetic.make_clips(2, K + T + F, 1, 32, 32, 77))


def _env(root, name, alpha=1.0, beta=0.02, **kw):
    torch.manual_seed(0)
    np.random.seed(0)
    return create_training_environment(vfi.MCNetFillInModel(4, 1, 3), 1, str(root), name, K, T, F, [32, 32], alpha, beta, 1e-3, 0.5, 4, 2,
                                       3, [0, 0], device='cpu', **kw)


def _update(env):
    env.K, env.T, env.F = K, T, F
    env.train()
    env.set_train_inputs(_CLIPS[:, :K], _CLIPS[:, K + T:], _CLIPS[:, K:K + T])
    env.forward_train()
    env.optimize_parameters()


def test_the_flag_is_off_by_default_and_a_negative_weight_is_refused(monkeypatch):
    import train
    from video_frame_inpainting_amd.options import TrainOptions
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)         # the option parser's own check; nothing else is reached
    base = ['--name', 'x', '--K', '3', '--T', '2', '--F', '3', '--c_dim', '1', '--image_size', '32', '--batch_size', '2',
            '--model_key', 'MCNet_gray']
    opt = TrainOptions().parse(base)
    assert opt.lap_weight == 0.0 and opt.lap_levels == 5
    monkeypatch.setattr(train, '_run', lambda *a, **k: pytest.fail('the run was started'))
    for extra in ([], ['--resumable']):
        with pytest.raises(SystemExit) as e:
            train.main(base + ['--lap_weight', '-1'] + extra)
        assert '--lap_weight' in str(e.value) and e.value.code not in (0, None)
        with pytest.raises(SystemExit) as e:
            train.main(base + ['--lap_weight', '0.5', '--lap_levels', '7'] + extra)
        assert '--lap_levels' in str(e.value) and e.value.code not in (0, None)
    with pytest.raises(ValueError, match='lap_weight'):
        _env('unused', 'unused', lap_weight=-1.0)


def test_the_term_alone_is_the_pyramid_distance_of_the_prediction(tmp_path):
    env = _env(tmp_path, 'lap', alpha=0.0, beta=0.0, lap_weight=1.0, lap_levels=4)
    _update(env)
    pred = env.gen_output['pred'].detach().numpy()
    want = ref.lap_loss_ref(pred, _CLIPS[:, K:K + T].numpy(), 4)
    assert 0.0 < want['loss'] < 8.0
    assert abs(float(env.loss_G.item()) - want['loss']) <= 2.0 ** -23 * want['loss']           # the fp32 scalar: one rounding
    errs = env.get_current_errors()
    assert errs['G_lap'] == float(env.lap.item()) and abs(errs['G_lap'] - want['loss']) <= 2.0 ** -23 * want['loss']
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in env.generator.parameters() if p.requires_grad)
    assert any(float(p.grad.abs().max()) > 0 for p in env.generator.parameters())


def test_weight_zero_builds_no_module_and_prints_no_key(tmp_path):
    env = _env(tmp_path, 'plain')
    _update(env)
    assert sorted(env.get_current_errors()) == ['D_fake', 'D_real', 'G_GAN', 'G_Lp', 'G_gdl', 'G_loss']
    assert env.loss_lap is None and not hasattr(env, 'lap')
    zero = _env(tmp_path, 'zero', lap_weight=0.0)
    _update(zero)
    assert zero.loss_lap is None and zero.get_current_errors() == env.get_current_errors()
    for a, b in zip(env.generator.parameters(), zero.generator.parameters()):
        assert torch.equal(a, b)
    state = env.get_current_state_dict(1, 0, 0)
    with_term = _env(tmp_path, 'with', lap_weight=0.5)
    assert isinstance(with_term.loss_lap, LapLoss) and with_term.loss_lap.levels == 5
    assert sorted(with_term.get_current_state_dict(1, 0, 0)) == sorted(state)
    assert list(with_term.generator.state_dict()) == list(env.generator.state_dict())


# ---------------------------------------------------------------------------------------------------------------- header, library

def test_the_header_declares_the_entry_points_and_the_library_exports_them():
    header = open(os.path.join(ROOT, 'include', 'tai_sepconv.h')).read()
    assert {'tai_lap_loss', 'tai_lap_loss_workspace_bytes'} <= set(_native.declared_symbols())
    assert 'long long tai_lap_loss_workspace_bytes(long long planes, int H, int W, int levels);' in header
    for line in ('k = (1, 4, 6, 4, 1) / 16', 'L_l = G_l - U(G_{l+1}) for l < L-1', 'grad = fp32((t_0 * 0.5) / count)',
                 's_l = 2^l * sign(L_l)'):
        assert line in header, line
    L = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(L, 'tai_lap_loss') and hasattr(L, 'tai_lap_loss_workspace_bytes')
    L.tai_sepconv_version.restype = ctypes.c_int
    assert L.tai_sepconv_version() >= 830
    # the workspace query is host code
    q = L.tai_lap_loss_workspace_bytes
    q.restype = ctypes.c_longlong
    q.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    assert q(160, 128, 128, 5) == 8 and q(1, 1, 1, 1) == 8                      # the pyramid fits LDS: nothing but a token
    third = 128 * 128 + 64 * 64 + 32 * 32 + 16 * 16                             # levels 1..4 of a 256 x 256 plane
    assert q(144, 256, 256, 5) == 144 * third * 8
    assert q(600, 256, 256, 5) == 512 * third * 8                               # the grid is capped at 512 workgroups
    for bad in ((0, 8, 8, 1), (-1, 8, 8, 1), (1, 8, 8, 0), (1, 8, 8, 7), (1, 15, 16, 5), (1, 16, 15, 5), (1, 0, 8, 1), (1, 8, 0, 1),
                (1 << 31, 1, 1, 1), (1 << 11, 1 << 10, 1 << 10, 1), (1, 1 << 16, 1 << 15, 1), (1 << 40, 2, 2, 1)):
        assert q(*bad) < 0, bad
    assert q((1 << 31) - 1, 1, 1, 1) > 0
