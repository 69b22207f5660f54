"""tests/kink_sides.py judged without a GPU: a stand-in "product" -- the discriminator's layer in fp32 torch, rounded at every stage
(conv2d, per-window factor, bias, LeakyReLU) -- on seeded weights and clips at the discriminator geometries of the GPU tests passes
check_layer on every layer; planted defects fail it."""
import pytest
import torch
import torch.nn.functional as F

from video_frame_inpainting_amd import synthetic
from video_frame_inpainting_amd.sn_discriminator import SNDiscriminator, max_singular_value

import kink_sides as ks  # noqa: E402

IP, WINDOW, B = 3, 3, 2
# name -> (df_dim, c_dim, H, W, K, T, F, windows kept).  Full width: the first, middle and last window, as the GPU tests keep them
GEOMETRIES = {'df8 128x128': (8, 1, 128, 128, 5, 5, 5, None),
              'df8 64x96': (8, 1, 64, 96, 4, 2, 3, None),
              'df64 128x128': (64, 1, 128, 128, 5, 5, 5, ks.ends_and_middle),
              'df64 colour 160x208': (64, 3, 160, 208, 4, 3, 4, ks.ends_and_middle)}     # planes 80 x 104 ... 10 x 13: odd, HW % 4 != 0
_STAND_IN = {}


def stand_in_layer(x, w0, bias, inv_scale, nw, windows, slope=0.2):
    """One LayerCall of the stand-in: fp32, every stage rounded."""
    per_window = x.shape[0] // len(windows)
    s = inv_scale[list(windows)].repeat_interleave(per_window).view(-1, 1, 1, 1)
    y = F.leaky_relu(F.conv2d(x, w0, None, (2, 2), (1, 1)) * s + bias.view(1, -1, 1, 1), slope)
    return ks.LayerCall(x, w0, bias, inv_scale, nw, (2, 2), (1, 1), slope, y, list(windows))


def stand_in(name):
    """The 4 LayerCalls of one discriminator evaluation at a geometry, computed once: weights of synthetic.seeded_init, the per-window
    factors of the product's CPU power iteration (nw renormalisations in a row), a clip of synthetic.make_clips."""
    if name not in _STAND_IN:
        df_dim, c_dim, H, W, K, T, Fn, keep = GEOMETRIES[name]
        disc = synthetic.seeded_init(SNDiscriminator((H, W), c_dim, WINDOW, df_dim, IP), 22)
        g = torch.Generator().manual_seed(23)
        clips = torch.from_numpy(synthetic.make_clips(B, K + T + Fn, c_dim, H, W, synthetic.SEEDS['cfg3']))
        nw = K + T + Fn - WINDOW + 1
        windows = list(range(nw)) if keep is None else keep(nw)
        x = torch.cat([clips[:, t0:t0 + WINDOW].reshape(B, WINDOW * c_dim, H, W) for t0 in windows], 0)
        recs = []
        with torch.no_grad():
            for layer in disc.conv_layers:
                if not hasattr(layer, 'Ip'):
                    continue
                w0 = layer.weight.detach().clone()
                u = torch.randn(1, w0.size(0), generator=g)
                wt, sigmas = w0.clone(), []
                for _ in range(nw):
                    sigma, u = max_singular_value(wt.view(wt.size(0), -1), u, IP)
                    wt = wt / sigma
                    sigmas.append(sigma.view(()))
                inv_scale = torch.cumprod(torch.stack(sigmas), 0).reciprocal()
                recs.append(stand_in_layer(x, w0, layer.bias.detach().clone(), inv_scale, nw, windows))
                x = recs[-1].y
        _STAND_IN[name] = recs
    return _STAND_IN[name]


@pytest.mark.parametrize('name', sorted(GEOMETRIES))
def test_clean_stand_in_passes_every_layer(name):
    """(i)-(iii) on all 4 layers; the share of elements where either kink side is a legitimate fp32 answer stays at or below 1e-3
    (measured: <= 5.5e-4), the stand-in's worst error is < 0.01 B and whatever sign differs from float64's does so inside B."""
    for li, rec in enumerate(stand_in(name)):
        res = ks.check_layer(rec)
        print('%s layer %d: %s' % (name, li, ks.format_layer(res)))
        assert res['ambiguous'] <= ks.AMBIGUOUS_SHARE * res['numel']
        assert res['worst'] < 0.05


# ---- planted defects: each on one layer call; -> the defective output (fp32)
def _one_window_factor_off(rec, i):
    inv = rec.inv_scale.clone()
    inv[rec.windows[i]] *= 1 + 1e-4
    return stand_in_layer(rec.x, rec.w0, rec.bias, inv, rec.nw, rec.windows).y


def _one_channel_bias_dropped(rec, k):
    bias = rec.bias.clone()
    bias[k] = 0
    return stand_in_layer(rec.x, rec.w0, bias, rec.inv_scale, rec.nw, rec.windows).y


def _neighbouring_windows_swapped(rec, i):
    assert rec.windows[i + 1] == rec.windows[i] + 1
    y = rec.y.clone()
    y[i * B:(i + 1) * B], y[(i + 1) * B:(i + 2) * B] = rec.y[(i + 1) * B:(i + 2) * B], rec.y[i * B:(i + 1) * B]
    return y


def _last_column_replicate_padded(rec, n, k):
    xp = F.pad(F.pad(rec.x[n:n + 1], (1, 0, 1, 1)), (0, 1, 0, 0), mode='replicate')         # zeros above, below and left; the last column repeated
    s = rec.inv_scale[rec.windows[n // B]]
    col = F.leaky_relu(F.conv2d(xp, rec.w0[k:k + 1], None, (2, 2), 0) * s + rec.bias[k], rec.slope)[0, 0, :, -1]
    y = rec.y.clone()
    y[n, k, :, -1] = col
    return y


def _one_channel_slope_twice(rec, k):
    y = rec.y.clone()
    y[:, k] = torch.where(y[:, k] < 0, y[:, k] * rec.slope, y[:, k])
    return y


def _one_element_other_sign(rec, _):
    z, _, _, bound = ks.layer_reference(rec)
    far = torch.where(z.abs() > 10 * bound, z.abs(), torch.full_like(z, float('inf')))
    at = torch.unravel_index(far.argmin(), far.shape)          # the element nearest the kink that is NOT ambiguous
    y = rec.y.clone()
    y[at] = -y[at]
    return y


# defect -> (geometry, layer, function, place).  Places: where check_layer's margin is SMALLEST among a few candidates looked at on the
# CPU (the factor: only the first layer's tiles have magnitude sums small enough for 1e-4 of an output to exceed B at all)
DEFECTS = {'one window\'s inv_scale x (1 + 1e-4)': ('df8 64x96', 0, _one_window_factor_off, (6,)),
           'bias of one output channel dropped': ('df8 128x128', 1, _one_channel_bias_dropped, (9,)),
           'images of two neighbouring windows swapped': ('df8 64x96', 2, _neighbouring_windows_swapped, (4,)),
           'last output column of one plane with replicate padding': ('df64 colour 160x208', 3, _last_column_replicate_padded, (5, 0)),
           'one channel\'s negative side x slope twice': ('df64 128x128', 3, _one_channel_slope_twice, (356,)),
           'one element with |z| > 10 B given the other sign': ('df8 128x128', 0, _one_element_other_sign, (None,))}


@pytest.mark.parametrize('defect', sorted(DEFECTS))
def test_planted_defect_fails_check_layer(defect):
    """Each defect on one layer call of the clean stand-in fails check_layer.

    The figures next to it are the defect's largest error in units of B and in units of 2e-5 * max |ref| of the whole tensor (the bound of
    the kernel-level tests of this layer, tests/test_gpu_training.py and tests/test_gpu_wino_ragged.py).  They are printed, not
    asserted to be below 1: on these operands (clip frames in [-1, 1], spectrally normalised weights) max |y| is 0.3-1.7 while
    1 + the tile's magnitude sum is 1.03-7, so B is the LARGER of the two bounds everywhere but in a few first-layer tiles, and a search
    over every window, channel and plane of all 16 layer calls found no placement of any of the six defects that check_layer catches and
    the whole-tensor bound lets through (its smallest figure there: 2.8).  What the whole-step tests lacked was not a sharper bound on the
    discriminator's activations but any per-element bound at all."""
    name, li, plant, place = DEFECTS[defect]
    rec = stand_in(name)[li]
    ks.check_layer(rec)
    bad = rec._replace(y=plant(rec, *place))
    _, y, _, bound = ks.layer_reference(rec)
    err = (bad.y.double() - y).abs()
    print('%s (%s, layer %d): %.3g B, %.3g x 2e-5 max|ref|' % (defect, name, li, float((err / bound).max()),
                                                              float(err.max()) / (2e-5 * float(y.abs().max()))))
    with pytest.raises(AssertionError, match=r'^\((i|ii)\) '):
        ks.check_layer(bad)


def test_sign_on_the_wrong_side_fails_on_its_own_and_nan_counts_as_infinite():
    """(ii) is a condition of its own: an output within B of y but on the other side of the kink than a z with |z| > B (possible up to
    |z| = B / slope) fails; a NaN fails (i)."""
    rec = stand_in('df8 64x96')[3]
    z, y, _, bound = ks.layer_reference(rec)
    inside = (z < -1.5 * bound) & (z > -4 * bound)             # y = 0.2 z is within 0.8 B of zero: +1e-30 is within B of y
    assert bool(inside.any())
    at = tuple(int(i) for i in inside.nonzero()[0])
    bad = rec.y.clone()
    bad[at] = 1e-30
    with pytest.raises(AssertionError, match=r'^\(ii\) 1 outputs'):
        ks.check_layer(rec._replace(y=bad))
    bad = rec.y.clone()
    bad[0, 0, 0, 0] = float('nan')
    with pytest.raises(AssertionError, match=r'^\(i\) .*inf'):
        ks.check_layer(rec._replace(y=bad))


def test_a_layer_of_ambiguous_elements_fails_non_vacuity():
    """(iii): outputs at rounding distance from the kink everywhere (a layer whose input is 1e-6 of the clip) agree with float64 in value
    and may differ in sign anywhere -- the check refuses to certify such sides."""
    rec = stand_in('df8 64x96')[0]
    quiet = stand_in_layer(rec.x * 1e-6, rec.w0, torch.zeros_like(rec.bias), rec.inv_scale, rec.nw, rec.windows)
    with pytest.raises(AssertionError, match=r'^\(iii\) '):
        ks.check_layer(quiet)


def test_tile_mag_on_planes_that_are_no_multiple_of_the_tile():
    mag = torch.arange(10 * 13, dtype=torch.float64).view(1, 1, 10, 13)
    got = ks.wc.tile_mag(mag)
    assert got.shape == mag.shape
    for y0 in range(0, 10, 4):
        for x0 in range(0, 13, 4):
            assert bool((got[..., y0:y0 + 4, x0:x0 + 4] == mag[..., y0:y0 + 4, x0:x0 + 4].max()).all())
    whole = torch.rand(2, 3, 8, 12, dtype=torch.float64)
    assert torch.equal(ks.wc.tile_mag(whole), F.interpolate(F.max_pool2d(whole, 4), scale_factor=4, mode='nearest'))     # as before


def test_discriminator_spy_keeps_the_selected_windows_and_every_side(monkeypatch):
    """DiscriminatorSpy around a CPU stand-in of _WindowScaledConvLReLU.apply: the arguments as passed, the images of ``keep``'s windows
    in order, the sides of every window; masks_of_call cuts them per window and layer."""
    from video_frame_inpainting_amd import sn_discriminator as snd
    rec = stand_in('df8 64x96')[0]

    def apply(x, weight, w0, bias, inv_scale, nw, stride, padding, slope):
        return stand_in_layer(x, w0, bias, inv_scale, nw, list(range(nw)), slope).y
    monkeypatch.setattr(snd._WindowScaledConvLReLU, 'apply', staticmethod(apply))
    spy = ks.DiscriminatorSpy(monkeypatch, keep=ks.ends_and_middle)
    for _ in range(4):
        y = snd._WindowScaledConvLReLU.apply(rec.x, None, rec.w0, rec.bias, rec.inv_scale, rec.nw, (2, 2), (1, 1), 0.2)
    assert torch.equal(y, rec.y) and len(spy.calls) == len(spy.layers) == 4
    kept = spy.calls[2]
    assert kept.windows == [0, 3, 6] and kept.nw == 7 and kept.stride == (2, 2) and kept.padding == (1, 1) and kept.slope == 0.2
    rows = [0, 1, 6, 7, 12, 13]
    assert torch.equal(kept.x, rec.x[rows]) and torch.equal(kept.y, rec.y[rows]) and torch.equal(kept.inv_scale, rec.inv_scale)
    assert torch.equal(kept.w0, rec.w0) and torch.equal(kept.bias, rec.bias)
    full = ks.check_layer(rec)
    part = ks.check_layer(kept)
    assert part['numel'] * 7 == full['numel'] * 3 and part['worst'] <= full['worst']
    masks = spy.masks_of_call(0, B)
    assert len(masks) == 4 * 7
    assert torch.equal(masks[(5, 'conv_layers.4')], rec.y[10:12] > 0)


def test_oracle_sides_are_counted_against_the_imposed_ones_per_evaluation_and_layer():
    """OracleSides around train_oracle.discriminator_leg: its sides, restacked as the product stacks them (windows along the batch), differ
    from themselves nowhere; one flipped element is counted at its evaluation and layer; report_lines gives one line per call."""
    from oracle import train_oracle
    K, T, Fn, H = 3, 2, 3, 32
    nw = K + T + Fn - WINDOW + 1
    disc = synthetic.seeded_init(SNDiscriminator((H, H), 1, WINDOW, 4, IP), 22)
    g = torch.Generator().manual_seed(23)
    u = {name: torch.randn(1, m.weight.size(0), generator=g) for name, m in disc.named_modules() if hasattr(m, 'Ip')}
    state = train_oracle.DiscriminatorState(disc.state_dict(), u, IP, WINDOW)
    clips = torch.from_numpy(synthetic.make_clips(B, K + T + Fn, 1, H, H, synthetic.SEEDS['cfg3']))
    P, GT, Fo = synthetic.split_clip(clips, K, T, Fn)
    with ks.OracleSides() as own:
        train_oracle.discriminator_leg(state, torch.cat([P, 0.9 * GT, Fo], 1), P, GT, Fo)
    assert train_oracle.F.conv2d is F.conv2d and len(own.layers) == 2 * nw * 4

    class Product(object):
        layers = [None] * 4 + [torch.cat([own.layers[(ev * nw + t0) * 4 + li] for t0 in range(nw)], 0) for ev in (0, 1) for li in range(4)]
        calls = []
    assert set(own.differences(Product, B).values()) == {0}
    Product.layers[4 * 2 + 1][2 * B + 1, 0, 3, 3] ^= True              # evaluation 2, layer 1, window 2
    diffs = own.differences(Product, B)
    assert diffs.pop((2, 1)) == 1 and set(diffs.values()) == {0}
    Product.calls = stand_in('df8 64x96') * 3
    lines = ks.report_lines(Product, [ks.check_layer(rec) for rec in Product.calls], own.differences(Product, B))
    assert len(lines) == 12 and lines[0].startswith('D evaluation 0 conv_layers.0') and lines[0].endswith(' -')
    assert lines[9].startswith('D evaluation 2 conv_layers.2') and lines[9].endswith(' 1') and 'all 7' in lines[9]


@pytest.mark.parametrize('shape', ks.LAYER_SHAPES)
def test_layer_alone_cases_are_not_vacuous_and_see_a_neighbouring_windows_factor(shape):
    """The operands of tests/test_gpu_kink_sides.py without a GPU: the stand-in passes (i)-(iii) on them (so (iii) cannot fail there for the
    seed's sake), and every image scaled with the NEXT window's factor -- 1e-4 away at 13 windows -- fails."""
    nw = shape[0]
    x, w, b, inv, _ = ks.layer_case(shape)
    rec = stand_in_layer(x, w, b, inv, nw, list(range(nw)))
    res = ks.check_layer(rec)
    print('%s: %s' % (shape, ks.format_layer(res)))
    shifted = stand_in_layer(x, w, b, torch.cat([inv[1:], inv[-1:]]), nw, list(range(nw)))
    with pytest.raises(AssertionError, match=r'^\(i\) '):
        ks.check_layer(rec._replace(y=shifted.y))
