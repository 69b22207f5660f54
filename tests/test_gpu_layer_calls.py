"""Every layer call of a generator training step on the MI355X against float64 on its own operands (tests/layer_calls.py): the shapes,
channel counts, needs_input_grad subsets and weight orientations the MODEL hands the autograd Functions -- planes of 2 x 3 to 64 x 96, the
17-channel input, 2- and 4-part inputs, a part and first layers without an input gradient, transposed weights ending in tanh on one
channel -- with the product's own kink sides, at the per-kernel bounds.  Each case is one forward + backward and its judgement; the
census, the worst ratio per route and the calls still on ATen go to stdout (and, with LAYER_CALL_REPORT set, to that file:
profiles/layer_call_parity.txt)."""
import time

import pytest
import torch

from video_frame_inpainting_amd import conv_ops, tai

import layer_calls as lc  # noqa: E402

pytestmark = pytest.mark.gpu
IN_TREE = {'autograd_3x3', 'autograd_parts', 'autograd_kxk', 'autograd_thin_in', 'autograd_thin_out'}


def _thresholds_of_a_full_batch(monkeypatch):
    """every layer takes the in-tree route it takes at 32 clips per GPU, at B = 2 (tests/test_gpu_wino_conv.py does the same)"""
    for name in ('WINO_MIN_WORKGROUPS', 'WINO43_MIN_WORKGROUPS', 'WINO43_SPLIT_MIN_WORKGROUPS'):
        monkeypatch.setattr(conv_ops, name, 1)


def _step_and_verdict(monkeypatch, title, spec, B, K, Fn, T, H, W):
    model = lc.make_model(spec, 'cuda')
    rec = lc.StepRecorder(monkeypatch, model)
    torch.cuda.synchronize()
    t0 = time.time()
    grads = lc.run_step(model, B, K, Fn, T, H, W)
    torch.cuda.synchronize()
    seconds = time.time() - t0
    verdict = lc.Verdict(rec, model, grads)
    lc.emit(verdict.report(title, seconds))
    return rec, verdict


def _counts(rec):
    return tuple(len(rec.of(k)) for k in ('conv', 'act_pool', 'lstm', 'unpool', 'upsample', 'pad', 'sepconv'))


def _assert_clean(rec, verdict):
    assert rec.bypassed == [] and rec.fused_motion_enc == 0
    assert all(c.g is not None for c in rec.of('conv'))                 # every hook fired: no call is skipped by the judge
    assert verdict.failures == [], '\n'.join(verdict.failures)


def test_gray_5_block_fused_directions_on_the_in_tree_routes(monkeypatch):
    _thresholds_of_a_full_batch(monkeypatch)
    rec, verdict = _step_and_verdict(monkeypatch, 'gray 5-block 64x96 B 2 K 3 F 3 T 2, thresholds 1, default tiles', lc.GRAY5, 2, 3, 3, 2, 64, 96)
    assert _counts(rec) == (104, 15, 3, 6, 8, 2, 2)
    assert IN_TREE <= set(verdict.routes()), verdict.routes()
    _assert_clean(rec, verdict)


def test_gray_5_block_on_the_2x2_tile(monkeypatch):
    """F(2x2, 3x3) for everything under autograd and the F(2x2, 3x3)-domain weight gradient"""
    _thresholds_of_a_full_batch(monkeypatch)
    monkeypatch.setattr(conv_ops, 'WINO43_UNDER_AUTOGRAD', False)
    prev = conv_ops.set_weight_gradient_tile(2)
    try:
        rec, verdict = _step_and_verdict(monkeypatch, 'gray 5-block 64x96 B 2 K 3 F 3 T 2, thresholds 1, 2x2 tiles', lc.GRAY5, 2, 3, 3, 2, 64, 96)
    finally:
        conv_ops.set_weight_gradient_tile(prev)
    assert _counts(rec) == (104, 15, 3, 6, 8, 2, 2)
    assert IN_TREE <= set(verdict.routes()), verdict.routes()
    _assert_clean(rec, verdict)


def test_gray_5_block_directions_apart_default_thresholds_reproducible_backward(monkeypatch):
    """K != F: two generator passes at B = 2, the mix of in-tree kernels and aten.convolution_backward fall-backs a 2-clip batch really
    runs, with the fixed-order replicate-pad backward of --resumable"""
    prev = tai.set_reproducible_backward(True)
    try:
        rec, verdict = _step_and_verdict(monkeypatch, 'gray 5-block 64x96 B 2 K 3 F 2 T 3, default thresholds, reproducible backward',
                                         lc.GRAY5, 2, 3, 2, 3, 64, 96)
    finally:
        tai.set_reproducible_backward(prev)
    assert all(c.fixed_order for c in rec.of('pad')) and _counts(rec) == (216, 39, 7, 18, 8, 2, 2)
    _assert_clean(rec, verdict)


def test_colour_4_block_on_the_in_tree_routes(monkeypatch):
    """c_dim 3: the 3-channel first and last layers on the min_ci = 2 route"""
    _thresholds_of_a_full_batch(monkeypatch)
    rec, verdict = _step_and_verdict(monkeypatch, 'colour 4-block 32x48 B 2 K 3 F 3 T 2, thresholds 1', lc.COLOUR4, 2, 3, 3, 2, 32, 48)
    assert _counts(rec) == (97, 15, 3, 6, 7, 2, 2)
    three = [c for c in rec.of('conv') if c.name in ('generator.content_enc.cont_conv1.0', 'generator.dec_cnn.dec1.2')]
    assert three and all(c.route == 'autograd_3x3' for c in three), [(c.name, c.route) for c in three]
    _assert_clean(rec, verdict)
