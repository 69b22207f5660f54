"""The derived-weight cache without a GPU: ``conv_ops._cached``'s contract under a counting ``make`` for every weight writer that can
run on the host (tests/derived_cases.py: WRITERS), the fused step's host path, the weight average on a stub environment, the replica
broadcast, and the condition on the GPU matrix's inputs: every write of every row moves the float64 reference by at least
DISCRIMINATING bounds, so that a form of the weights of before the write cannot pass the comparison."""
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import derived_cases as dc  # noqa: E402

from video_frame_inpainting_amd import conv_ops, fused_step  # noqa: E402


class _Counted(object):
    """``make`` of one tag of one weight: a copy of the weight as it is now, and how often it was asked for"""

    def __init__(self, weight, tag):
        self.weight, self.tag, self.calls = weight, tag, 0

    def make(self):
        self.calls += 1
        return self.weight.detach().clone()

    def get(self):
        return conv_ops._cached(self.weight, self.tag, self.make)

    def assert_current(self, calls, what):
        got = self.get()
        assert self.calls == calls, '%s: make ran %d times, not %d' % (what, self.calls, calls)
        assert torch.equal(got, self.weight.detach()), '%s: the derived form is not that of the current weight' % what
        assert self.get() is got and self.calls == calls, '%s: a second call rebuilt' % what


def _layer(seed=7):
    return dc.init_module(nn.Conv2d(4, 6, 3, padding=1), seed)


def _case(module, tmp_path=None):
    return dc.Case(None, module, 'cpu', tmp_path)


def test_two_calls_with_nothing_changed_build_once():
    m = _layer()
    c = _Counted(m.weight, 'a')
    first = c.get()
    assert c.get() is first and c.calls == 1
    assert torch.equal(first, m.weight.detach())


@pytest.mark.parametrize('writer', [w for w in dc.WRITERS if w.number in (1, 5, 6, 7, 8, 9, 10)], ids=lambda w: w.name)
def test_each_writer_causes_exactly_one_rebuild(writer):
    m = _layer()
    c, other = _Counted(m.weight, 'a'), _Counted(m.bias, 'a')
    c.assert_current(1, 'before')
    other.assert_current(1, 'before (bias)')
    before = m.weight.detach().clone()
    state = {'calls': 1, 'phase': 0}

    def check(label):
        state['calls'] += writer.rebuilds[state['phase']]
        state['phase'] += 1
        assert not torch.equal(m.weight.detach(), before), '%s: the writer wrote nothing' % label
        c.assert_current(state['calls'], label)
        other.assert_current(state['calls'], label + ' (bias)')
    writer.fn(_case(m), check)
    assert state['phase'] == len(writer.rebuilds)


def test_two_tags_on_one_weight_are_independent():
    m = _layer()
    a, b = _Counted(m.weight, 'a'), _Counted(m.weight, ('b', 1))
    a.assert_current(1, 'a')
    assert b.calls == 0
    b.assert_current(1, 'b')
    assert a.calls == 1
    with torch.no_grad():
        m.weight.mul_(2.0)
    a.assert_current(2, 'a after a write')
    assert b.calls == 1                                # asking for one tag does not rebuild the other ...
    b.assert_current(2, 'b after a write')             # ... which is still rebuilt when it is asked for
    assert a.calls == 2
    del m.weight._tai_derived['a']
    b.assert_current(2, 'b after a was dropped')
    a.assert_current(3, 'a after it was dropped')


@pytest.mark.parametrize('writer', [dc.WRITER['fused_step'], dc.WRITER['fused_step_skipped']], ids=lambda w: w.name)
def test_the_fused_step_host_path_leaves_no_derived_form_valid(writer):
    """host_step writes through numpy views: no version counter moves.  After the step the form is rebuilt from the current weight --
    after a skipped one too (the device path's host does not know the verdict; the two paths behave alike)."""
    m = _layer()
    forms = [_Counted(p, 'a') for p in m.parameters()]
    for c in forms:
        c.assert_current(1, 'before')
    kept = _Counted(_layer(8).weight, 'a')             # another module's weight: its form stays
    kept.assert_current(1, 'other module')

    def check(label):
        for c in forms:
            c.assert_current(2, label)
        kept.assert_current(1, label + ' (other module)')
    writer.fn(_case(m), check)


def test_averaged_weights_on_a_stub_environment():
    m = _layer()
    forms = {n: _Counted(p, 'a') for n, p in m.named_parameters()}
    for c in forms.values():
        c.assert_current(1, 'before')
    weights = {n: p.detach().clone() for n, p in m.named_parameters()}
    ema = {n: v.reshape(-1) for n, v in dc.new_values(m, 41).items()}
    with fused_step.averaged_weights(dc.stub_env(m, ema)):
        for n, c in forms.items():
            c.assert_current(2, 'inside')
            assert torch.equal(c.get().reshape(-1), ema[n])
    for n, c in forms.items():
        c.assert_current(3, 'after')
        assert torch.equal(c.get(), weights[n])
    # no average kept: the block exchanges nothing and drops nothing
    with fused_step.averaged_weights(dc.stub_env(m, {})):
        for c in forms.values():
            c.assert_current(3, 'inside, without an average')


def test_broadcast_in_a_group_of_one_writes_nothing_and_keeps_the_forms(tmp_path):
    m = _layer()
    c = _Counted(m.weight, 'a')
    c.assert_current(1, 'before')
    before = m.weight.detach().clone()
    dc.write_broadcast(_case(m, tmp_path), lambda label: c.assert_current(1, label))
    assert torch.equal(m.weight.detach(), before)


def _broadcast_worker(rank, world, path):
    import torch.distributed as dist
    from video_frame_inpainting_amd import parallel
    dist.init_process_group('gloo', store=dist.FileStore(os.path.join(path, 'store'), world), rank=rank, world_size=world)
    try:
        m = _layer(100 + rank)                          # the replicas start different
        c = _Counted(m.weight, 'a')
        c.assert_current(1, 'rank %d before' % rank)
        parallel.broadcast_module_state(m)
        assert torch.equal(m.weight.detach(), _layer(100).weight.detach())
        c.assert_current(2, 'rank %d after the broadcast' % rank)       # rebuilt once, from the received weight
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_broadcast_into_a_second_rank_rebuilds_its_forms(tmp_path):
    """Writer 12 where it does write: rank 1 receives rank 0's weights (gloo, two ranks on a FileStore)."""
    import torch.multiprocessing as mp
    mp.spawn(_broadcast_worker, args=(2, str(tmp_path)), nprocs=2, join=True)


# ---- the GPU matrix's inputs ---------------------------------------------------------------------------------------------------------

RATIOS = {}


@pytest.mark.parametrize('pair', dc.pairs(on_gpu=False), ids=dc.pair_id)
def test_every_write_of_the_matrix_is_discriminating(pair, tmp_path):
    """max |ref(new w) - ref(old w)| >= DISCRIMINATING x bound x max |ref(new w)| on every output that is computed from a derived form,
    from the float64 reference alone: a condition on the rows' inputs, not a measurement of the kernels.  Where a phase of a writer
    leaves the weights alone the reference must not move at all."""
    form, writer = pair
    module, inp = form.module('cpu'), form.inputs()
    state = {'ref': form.ref(module, inp), 'phase': 0}

    def check(label):
        new = form.ref(module, inp)
        writes = writer.writes[state['phase']]
        for i, (a, b) in enumerate(zip(state['ref'], new)):
            scale = dc.max_abs(b)
            assert scale > 0, (label, i)
            if not writes:
                assert torch.equal(a, b), (label, i)
            elif form.reads_form[i]:
                ratio = dc.max_abs(b - a) / (form.bound * scale)
                RATIOS.setdefault(form.name, []).append(ratio)
                assert ratio >= dc.DISCRIMINATING, '%s, %s, output %d: the write moves the reference by %.3g bounds only' % (
                    form.name, label, i, ratio)
        state['ref'], state['phase'] = new, state['phase'] + 1
    writer.fn(dc.Case(form, module, 'cpu', tmp_path), check)
    assert state['phase'] == len(writer.writes)


def test_report_the_discriminating_ratios():
    """pytest -s: per form, the smallest ratio over its writers and outputs (the condition itself is asserted above)"""
    for name in dc.FORM_IDS:
        if name in RATIOS:
            print('%-28s smallest max|ref(new) - ref(old)| / (bound max|ref(new)|) over %3d writes: %.3g' % (
                name, len(RATIOS[name]), min(RATIOS[name])))


def test_the_matrix_covers_every_tag_conv_ops_builds():
    """The first element of every tag handed to _cached in the package's sources appears in FORMS."""
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'video-frame-inpainting_amd')
    text = open(os.path.join(root, 'conv_ops.py')).read() + open(os.path.join(root, 'mcnet.py')).read()
    in_source = set(re.findall(r"_cached\([^,]+, \('(\w+)'", text)) | {'wino', 'wino43', 'wino_kxk', 'wino43_kxk'}
    assert {'bf16', 'direct', 'input_half', 'wino_input_grad_part'} <= in_source, in_source
    in_forms = {tag[0] for f in dc.FORMS for tags in f.tags.values() for tag in tags}
    assert in_source == in_forms, (sorted(in_source), sorted(in_forms))
