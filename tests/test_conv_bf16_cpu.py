"""The opt-in bf16 convolution mode without a GPU: the switch, the layer rule on the models' layer lists, the C ABI's three entry
points (header and library), and the rounding helper the emulating oracle and the GPU tests share (tests/bf16_emulation.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import video_frame_inpainting_amd as vfi
from video_frame_inpainting_amd import _native, conv_ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bf16_emulation import bf16_ok, bf16_round  # noqa: E402

ENTRY_POINTS = ('tai_conv_bf16_weight_elems', 'tai_conv_bf16_pack_weights', 'tai_conv_bf16_forward')


@pytest.fixture(autouse=True)
def _restore_precision():
    prev = conv_ops.get_conv_precision()
    yield
    conv_ops.set_conv_precision(prev)


def test_switch_default_round_trip_and_bad_names():
    assert conv_ops.get_conv_precision() == 'fp32'
    assert conv_ops.set_conv_precision('bf16') == 'fp32'
    assert conv_ops.get_conv_precision() == 'bf16'
    assert conv_ops.set_conv_precision('fp32') == 'bf16'
    assert conv_ops.get_conv_precision() == 'fp32'
    for bad in ('fp16', 'bf16x3', 'BF16', None, 1):
        with pytest.raises(ValueError):
            conv_ops.set_conv_precision(bad)
    assert conv_ops.get_conv_precision() == 'fp32'


def _convs(model):
    """(name, C in, K out, k, padding, stride) of every convolution of the generator, as the forward sees it"""
    out = []
    for name, m in model.named_modules():
        if isinstance(m, nn.ConvTranspose2d):
            out.append((name, m.weight.shape[0], m.weight.shape[1], m.kernel_size[0], m.padding[0], m.stride[0]))
        elif isinstance(m, nn.Conv2d):
            out.append((name, m.weight.shape[1], m.weight.shape[0], m.kernel_size[0], m.padding[0], m.stride[0]))
    return out


# the layers the rule leaves in fp32: one input channel (MotionEnc's first layer, gray ContentEnc's first), c_dim outputs (DecCnn's
# last), TAI_color's 3-channel layers
KEPT = {
    'TAI_gray': {'generator.motion_enc.dyn_conv1.0', 'generator.content_enc.cont_conv1.0', 'generator.dec_cnn.dec1.2'},
    'TAI_color': {'generator.motion_enc.dyn_conv1.0', 'generator.content_enc.cont_conv1.0', 'generator.dec_cnn.dec1.2'},
    'MCNet_gray': {'generator.motion_enc.dyn_conv1.0', 'generator.content_enc.cont_conv1.0', 'generator.dec_cnn.dec1.2'},
}


@pytest.mark.parametrize('key', sorted(KEPT))
def test_rule_takes_exactly_the_named_layers(key):
    convs = _convs(vfi.create_model(key))
    assert len(convs) > 20
    taken = {n for n, C, K, k, p, s in convs if s == 1 and conv_ops._bf16_ok(C, K, k, p)}
    assert {n for n, *_ in convs} - taken == KEPT[key]
    # the 5x5 / 7x7 MotionEnc layers, the transposed DecCnn layers and the kernel network's 51- and 65-channel layers are in
    names = {n: (C, K, k) for n, C, K, k, p, s in convs}
    assert 'generator.motion_enc.dyn_conv2.1' in taken and names['generator.motion_enc.dyn_conv3.1'][2] == 7
    assert 'generator.motion_enc.dyn_conv3.1' in taken
    assert any('dec_cnn.dec3' in n for n in taken)
    if key.startswith('TAI'):
        assert any(C in (51, 65) for n, C, K, k, p, s in convs if n in taken)
    # the test's own restatement agrees with the product's rule, and neither depends on N (no N in the signature at all)
    for n, C, K, k, p, s in convs:
        assert bf16_ok(C, K, k, p) == conv_ops._bf16_ok(C, K, k, p)


def test_rule_does_not_depend_on_the_batch(monkeypatch):
    """The route asks the rule with the weight's shape only: the same layers go to the bf16 kernel at N = 1 and N = 160."""
    seen = {}
    for N in (1, 160):
        asked = []
        monkeypatch.setattr(conv_ops, '_bf16_ok', lambda Ci, Co, k, p, _a=asked: _a.append((Ci, Co, k, p)) or bf16_ok(Ci, Co, k, p))
        conv_ops.set_conv_precision('bf16')
        for C, K, k in ((64, 128, 3), (1, 64, 5), (51, 51, 3), (128, 256, 7), (64, 3, 3)):
            asked.clear()
            conv_ops._bf16_route(C, K, k, k, k // 2)
            seen.setdefault((C, K, k), set()).add((N, tuple(asked), conv_ops._bf16_route(C, K, k, k, k // 2)))
    for key, v in seen.items():
        assert len({r for _, _, r in v}) == 1, key


def test_rule_edges():
    ok = conv_ops._bf16_ok
    assert ok(16, 16, 3, 1) and ok(16, 16, 5, 2) and ok(16, 16, 7, 3)
    assert not ok(15, 16, 3, 1) and not ok(16, 15, 3, 1) and not ok(1, 64, 5, 2) and not ok(64, 1, 3, 1) and not ok(3, 64, 3, 1)
    assert not ok(64, 64, 3, 0) and not ok(64, 64, 5, 1) and not ok(64, 64, 4, 2) and not ok(64, 64, 1, 0)


def test_header_declares_and_library_exports_the_entry_points():
    declared = set(_native.declared_symbols())
    assert set(ENTRY_POINTS) <= declared
    L = ctypes.CDLL(_native.build())
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name


def test_weight_elems_and_refusals_without_a_gpu():
    L = _native.lib()
    # ceil(K / 64) x ceil(C / 16) chunks x ceil(k^2 / 2) tap pairs x 64 x 32 bf16
    assert L.tai_conv_bf16_weight_elems(64, 64, 3) == 1 * 4 * 5 * 2048
    assert L.tai_conv_bf16_weight_elems(51, 65, 7) == 1 * 5 * 25 * 2048
    assert L.tai_conv_bf16_weight_elems(256, 512, 5) == 4 * 32 * 13 * 2048
    assert L.tai_conv_bf16_weight_elems(64, 1, 5) < 0 and L.tai_conv_bf16_weight_elems(64, 64, 4) < 0
    xs = (ctypes.c_void_p * 1)(16)
    for args in ((1, 64, 64, 8, 8, 4, 0), (1, 8, 64, 8, 8, 3, 0), (1, 64, 64, 8, 8, 3, 3), (0, 64, 64, 8, 8, 3, 0)):
        N, C, K, H, W, k, act = args
        rc = L.tai_conv_bf16_forward(xs, 1, 16, 16, 16, None, None, None, N, C, K, H, W, k, act, None)
        assert rc == -1, args
        assert L.tai_sepconv_last_error()
    # pool / unpool need even planes; y2 needs addx
    assert L.tai_conv_bf16_forward(xs, 1, 16, 16, 16, 16, None, None, 1, 64, 64, 9, 8, 3, 1, None) == -1
    assert L.tai_conv_bf16_forward(xs, 1, 16, 16, 16, None, None, 16, 1, 64, 64, 8, 8, 3, 0, None) == -1


def test_rounding_helper_equals_torch_bit_for_bit():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(200000, generator=g) * torch.exp(torch.randn(200000, generator=g) * 20)
    specials = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0x7fa12345, 0x7f800000, 0xff800000, 0x00000001, 0x80000000,
                         0x3f808000, 0x3f818000, 0x7f7fffff, 0x00008000, 0x3f80ffff], dtype=np.uint32).view(np.float32)
    x = torch.cat([torch.from_numpy(specials), x])
    got = bf16_round(x).numpy().view(np.uint64)
    want = x.bfloat16().double().numpy().view(np.uint64)
    assert np.array_equal(got, want)
    assert np.isnan(bf16_round(x[:4]).numpy()).all()
