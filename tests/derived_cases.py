"""The derived-weight cache of conv_ops (``_cached``: Winograd-domain images, their k x k block forms, per-part input-gradient
images, packed bf16 weights, the flipped ``direct`` layout, the ConvLSTM's ``input_half``) as a matrix: FORMS, one row per cache tag
and caller, and WRITERS, one per mechanism that changes a layer's weights.  tests/test_gpu_derived_weights.py runs forms x writers on
the GPU, tests/test_derived_weights_cpu.py checks the conditions on the inputs and the cache's contract without one.

A form holds the smallest layer and input that make conv_ops build its tags (``routes``: the dispatch thresholds it needs, set the
way the other tests set them), the call that uses them, the tags expected in ``weight._tai_derived`` afterwards (asserted, so that a
silent reroute fails) and a plain float64 CPU reference of the same operation from the CURRENT weights.  Under autograd the outputs
are y, the input gradient(s), the weight gradient and the bias gradient of sum(y * g) for a fixed g; the input gradient reads the
OTHER orientation's form, the weight and bias gradients read none (``reads_form``).

A writer is ``writer(case, check)``: it changes the weights of ``case.module`` to new values through one mechanism, calls
``check(label)`` after each of its phases and returns nothing.  Weights are drawn N(0, 0.05^2) and the Adam / fused writers step with
lr 0.05, so Adam's first step moves every element by about lr.

Bounds are the ones the suite already asserts per route: 1e-4 of the reference's maximum for the fp32 Winograd, thin and MIOpen routes
(tests/test_gpu_model.py::test_derived_weights_follow_in_place_weight_writes) and for the bf16x3 arithmetic
(tests/test_gpu_wino_split.py), 1e-5 against the float64 convolution of the bf16-rounded operands for the bf16 kernel
(tests/bf16_cases.py, tests/test_gpu_conv_bf16_kernel.py).
"""
import collections
import contextlib
import os
import sys
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_cases as bc  # noqa: E402

from video_frame_inpainting_amd import conv_ops, fused_step, grad_guard, util  # noqa: E402
from video_frame_inpainting_amd.mcnet import ConvLstmCell  # noqa: E402

FP32_BOUND = 1e-4
BF16_BOUND = 1e-5
LR = 0.05
W_STD, B_STD = 0.05, 0.1
DISCRIMINATING = 100            # a write moves the reference by at least this many bounds
RELU_MARGIN = 1e-5              # under autograd no pre-activation of a ReLU row is nearer to 0 (the fp32 mask is then the fp64 one)

F22 = {'WINO_MIN_WORKGROUPS': 0}                                     # every 3x3 layer the F(2x2, 3x3) kernel takes is given to it
F43 = {'WINO_MIN_WORKGROUPS': 0, 'WINO43_MIN_WORKGROUPS': 0}         # ... and F(4x4, 3x3) wherever its channel rule allows
DEFAULTS = {}                                                        # the default thresholds: these shapes stay below them


def _activate(y, act):
    return torch.relu(y) if act == 'relu' else (torch.tanh(y) if act == 'tanh' else y)


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def init_module(module, seed):
    """weights N(0, W_STD^2), biases N(0, B_STD^2), written before anything is cached"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (W_STD if p.dim() > 1 else B_STD))
    return module


def new_values(module, seed):
    """name -> a CPU tensor of other values of the same distribution"""
    g = torch.Generator().manual_seed(seed)
    return collections.OrderedDict((n, torch.randn(p.shape, generator=g) * (W_STD if p.dim() > 1 else B_STD))
                                   for n, p in module.named_parameters())


class Form(object):
    """One row of FORMS.  ``tags``: parameter name -> the tags its ``_tai_derived`` must hold after ``call``.  ``reads_form``: per
    output, whether it is computed from a derived form (the discriminating-write condition is asked of those).  ``exact``: a fresh
    Parameter gives the same bits (every in-tree kernel; False on the MIOpen route, which is compared inside the bound).  ``f22``: the
    tags carry the F(2x2, 3x3) arithmetic (writer 11 applies).  ``trained``: the call is one a training or validation run makes."""

    def __init__(self, name, make, inputs, call, ref, tags, routes, reads_form, bound=FP32_BOUND, exact=True, f22=False, precision='fp32',
                 trained=True):
        self.name, self.make, self.inputs, self.call, self.ref = name, make, inputs, call, ref
        self.tags, self.routes, self.reads_form, self.bound, self.exact, self.f22 = tags, routes, reads_form, bound, exact, f22
        self.precision, self.trained = precision, trained

    def module(self, device='cpu', seed=7):
        return init_module(self.make(), seed).to(device)

    def fresh(self, module):
        """The same layer on fresh Parameters cloned from ``module``'s current weights: no ``_tai_derived`` anywhere."""
        other = self.make().to(next(module.parameters()).device)
        for q, p in zip(other.parameters(), module.parameters()):
            q.data = p.detach().clone()
        assert not any(hasattr(q, '_tai_derived') for q in other.parameters())
        return other

    @contextlib.contextmanager
    def routed(self, monkeypatch):
        """The dispatch thresholds and the convolution precision of this row; the precision is put back on the way out."""
        for k, v in self.routes.items():
            monkeypatch.setattr(conv_ops, k, v)
        prev = conv_ops.set_conv_precision(self.precision)
        try:
            yield self
        finally:
            conv_ops.set_conv_precision(prev)

    def current_tags(self):
        """``tags`` under the Winograd arithmetic in force: the F(2x2, 3x3) tags end in it"""
        arith = conv_ops._WINO_ARITH[0]
        follow = lambda tag: tag[:-1] + (arith,) if tag[0] in ('wino', 'wino_kxk', 'wino_input_grad_part') else tag
        return {name: [follow(tag) for tag in tags] for name, tags in self.tags.items()}

    def assert_tags(self, module):
        named = dict(module.named_parameters())
        for name, tags in self.current_tags().items():
            have = getattr(named[name], '_tai_derived', {})
            for tag in tags:
                assert tag in have, '%s: %s holds %s, not %s: the call took another route' % (self.name, name, sorted(have, key=repr), tag)

    def derived(self, module):
        """[(parameter name, tag, the cached object)] of the row's tags"""
        named = dict(module.named_parameters())
        return [(name, tag, named[name]._tai_derived[tag][1]) for name, tags in self.current_tags().items() for tag in tags]


Case = collections.namedtuple('Case', 'form module device tmp_path')


def to_device(inputs, device):
    return {k: ([t.to(device) for t in v] if isinstance(v, list) else v.to(device)) for k, v in inputs.items()}


# ---- one convolution layer -------------------------------------------------------------------------------------------------

def _conv_form(name, make, x_shape, act, mode, tags, routes, nparts=1, **kw):
    """``make`` -> nn.Conv2d / nn.ConvTranspose2d (stride 1, padding k // 2); x [N, C, H, W], given as ``nparts`` channel parts"""
    transposed = isinstance(make(), nn.ConvTranspose2d)
    bf16 = kw.get('precision') == 'bf16'

    def inputs():
        m = make()
        Co = m.weight.shape[1] if transposed else m.weight.shape[0]
        N, C, H, W = x_shape
        return {'x': [_randn(11 + i, N, C // nparts, H, W) for i in range(nparts)], 'g': _randn(19, N, Co, H, W)}

    def call(module, inp):
        w, b, pad = module.weight, module.bias, module.padding[0]
        if mode == 'no_grad':
            with torch.no_grad():
                x = inp['x'] if nparts > 1 else inp['x'][0]
                return (conv_ops.conv_bias_act(x, w, b, pad, act, transposed=transposed),)
        xs = [p.detach().clone().requires_grad_(True) for p in inp['x']]
        y = conv_ops.conv_bias_act(xs if nparts > 1 else xs[0], w, b, pad, act, transposed=transposed)
        grads = torch.autograd.grad(y, xs + [w, b], inp['g'])
        return (y.detach(),) + tuple(grads)

    def ref(module, inp):
        w = module.weight.detach().cpu()
        b = module.bias.detach().cpu().double()
        xs = [p.detach().cpu() for p in inp['x']]
        if bf16:                                   # the bf16 kernel's definition: bf16-rounded operands, exact products (bf16_cases.conv64)
            w, xs = bc.bf16_round(w), [bc.bf16_round(p) for p in xs]
        w = w.double().requires_grad_(mode != 'no_grad')
        b.requires_grad_(mode != 'no_grad')
        xs = [p.double().requires_grad_(mode != 'no_grad') for p in xs]
        fn = F.conv_transpose2d if transposed else F.conv2d
        pre = fn(torch.cat(xs, 1), w, b, padding=module.padding[0])
        y = _activate(pre, act)
        if mode == 'no_grad':
            return (y,)
        if act == 'relu':
            assert float(pre.detach().abs().min()) > RELU_MARGIN, '%s: a pre-activation within %g of 0' % (name, RELU_MARGIN)
        grads = torch.autograd.grad(y, xs + [w, b], inp['g'].detach().cpu().double())
        return (y.detach(),) + tuple(grads)

    reads = (True,) if mode == 'no_grad' else (True,) + (True,) * nparts + (False, False)
    return Form('%s-%s' % (name, mode), make, inputs, call, ref, {'weight': tags}, routes, reads, **kw)


def _input_grad_part_tags(tile, nparts=2):
    return [('wino_input_grad_part', False, i, nparts, tile, 0) for i in range(nparts)]


def _marked(layer):
    conv_ops.mark_outside_recurrence(layer)        # F(4x4, 3x3) below 64 channels, as the kernel network's layers (tai.py)
    return layer


# ---- MotionEnc's chain on the 4 x 4 tile (the no-grad caller of the wino43_kxk form) --------------------------------------------------

def _chain_make():
    return nn.Sequential(nn.Conv2d(1, 16, 5, padding=2), nn.Conv2d(16, 32, 5, padding=2), nn.Conv2d(32, 64, 7, padding=3))


def _chain_call(module, inp):
    with torch.no_grad():
        r = conv_ops.motion_enc_chain(inp['x'], module[0], module[1], module[2])
    assert r is not None, 'motion_enc_chain refused the shape'
    return (r[0],) + tuple(r[1])


def _chain_ref(module, inp):
    x, outs = inp['x'].detach().cpu().double(), []
    for conv in module:
        y = torch.relu(F.conv2d(x, conv.weight.detach().cpu().double(), conv.bias.detach().cpu().double(), padding=conv.padding[0]))
        outs.append(y)
        x = F.max_pool2d(y, 2)
    return (x,) + tuple(outs)


# ---- the ConvLSTM's first step -----------------------------------------------------------------------------------------------------

LSTM_F = 16


def _lstm_call(module, inp):
    with torch.no_grad():
        new_h, (new_c, _) = module(inp['x'], (inp['c'], inp['h']), state_is_zero=True)
    return (new_h, new_c)


def _lstm_ref(module, inp):
    w, b = module.conv.weight.detach().cpu().double(), module.conv.bias.detach().cpu().double()
    x, c = inp['x'].detach().cpu().double(), inp['c'].detach().cpu().double()
    gates = F.conv2d(x, w[:, :LSTM_F], b, padding=1)          # h == 0: its half of the reduction contributes nothing
    i, j, f, o = torch.chunk(gates, 4, dim=1)
    new_c = c * torch.sigmoid(f + module.forget_bias) + torch.sigmoid(i) * torch.tanh(j)
    return (torch.tanh(new_c) * torch.sigmoid(o), new_c)


def _both(name, make, x_shape, tag_f, tag_b, routes, act_no_grad='relu', act_autograd='tanh', **kw):
    """the no-grad row (the forward's form) and the autograd row (both orientations' forms)"""
    return [_conv_form(name, make, x_shape, act_no_grad, 'no_grad', [tag_f], routes, **kw),
            _conv_form(name, make, x_shape, act_autograd, 'autograd', [tag_f, tag_b], routes, **kw)]


X16, X64 = (2, 16, 8, 8), (2, 64, 8, 8)

FORMS = (
    _both('wino', lambda: nn.Conv2d(16, 16, 3, padding=1), X16, ('wino', False, 0), ('wino', True, 0), F22, f22=True)
    + _both('wino-T', lambda: nn.ConvTranspose2d(16, 16, 3, padding=1), X16, ('wino', True, 0), ('wino', False, 0), F22, f22=True)
    + _both('wino43', lambda: nn.Conv2d(64, 64, 3, padding=1), X64, ('wino43', False), ('wino43', True), F43)
    + _both('wino43-T', lambda: nn.ConvTranspose2d(64, 64, 3, padding=1), X64, ('wino43', True), ('wino43', False), F43)
    # the 5x5 layer as 2 x 2 blocks of 3 x 3 taps: _kxk_as_wino / _WinoConvKxK on F(2x2, 3x3) (the 4 x 4 tile's threshold left alone) ...
    + _both('wino_kxk', lambda: nn.Conv2d(16, 16, 5, padding=2), X16, ('wino_kxk', False, 0), ('wino_kxk', True, 0), F22,
            act_autograd='relu', f22=True)
    + [
        # ... and on the 4 x 4 tile: _WinoConvKxK -> _kxk_as_blocks under autograd, motion_enc_chain without (its 5x5 at 8 x 8 and its
        # 7x7 at 4 x 4: the smallest planes _wino43_blocks_ok takes, H % 4 == 0, from a 16 x 16 difference frame)
        _conv_form('wino43_kxk', lambda: nn.Conv2d(16, 16, 5, padding=2), X16, 'relu', 'autograd',
                   [('wino43_kxk', False), ('wino43_kxk', True)], F43),
        Form('wino43_kxk-chain-no_grad', _chain_make, lambda: {'x': _randn(13, 2, 1, 16, 16)}, _chain_call, _chain_ref,
             {'1.weight': [('wino43_kxk', False)], '2.weight': [('wino43_kxk', False)]}, F43, (True, False, True, True)),
        # two channel parts read where they lie: the forward's form and one input-gradient image per part, on either tile
        _conv_form('wino_parts', lambda: nn.Conv2d(16, 16, 3, padding=1), X16, 'tanh', 'autograd',
                   [('wino', False, 0)] + _input_grad_part_tags(2), F22, nparts=2, f22=True),
        _conv_form('wino43_parts', lambda: _marked(nn.Conv2d(64, 64, 3, padding=1)), X64, 'tanh', 'autograd',
                   [('wino43', False)] + _input_grad_part_tags(4), F43, nparts=2),
        # the opt-in bf16 kernel on the smallest shape of tests/bf16_cases.py (3 x 16 x 1 x 1 into 16 channels, k = 3), either weight form
        _conv_form('bf16', lambda: nn.Conv2d(16, 16, 3, padding=1), (3, 16, 1, 1), 'relu', 'no_grad', [('bf16', False)], DEFAULTS,
                   bound=BF16_BOUND, precision='bf16', trained=False),
        _conv_form('bf16-T', lambda: nn.ConvTranspose2d(16, 16, 3, padding=1), (3, 16, 1, 1), 'relu', 'no_grad', [('bf16', True)], DEFAULTS,
                   bound=BF16_BOUND, precision='bf16', trained=False),
        # the flipped layout: a transposed layer MIOpen convolves, the one-output-channel layer (either mode), the one-input-channel one
        _conv_form('direct-miopen-T', lambda: nn.ConvTranspose2d(16, 16, 3, padding=1), X16, 'relu', 'no_grad', [('direct', True)], DEFAULTS,
                   exact=False),
        _conv_form('direct-thin_out', lambda: nn.Conv2d(16, 1, 3, padding=1), X16, 'tanh', 'no_grad', [('direct', False)], DEFAULTS),
        _conv_form('direct-thin_out', lambda: nn.Conv2d(16, 1, 3, padding=1), X16, 'tanh', 'autograd', [('direct', False)], DEFAULTS),
        _conv_form('direct-thin_out-T', lambda: nn.ConvTranspose2d(16, 1, 3, padding=1), X16, 'tanh', 'autograd', [('direct', True)], DEFAULTS),
        _conv_form('direct-thin_in', lambda: nn.Conv2d(1, 16, 5, padding=2), (2, 1, 8, 8), 'relu', 'no_grad', [('direct', False)], DEFAULTS),
        # the ConvLSTM's first step: the input half of the gates' weight (h == 0), itself convolved on the Winograd kernel
        Form('input_half-no_grad', lambda: ConvLstmCell(3, LSTM_F),
             lambda: {'x': _randn(14, 2, LSTM_F, 8, 8), 'c': _randn(15, 2, LSTM_F, 8, 8), 'h': torch.zeros(2, LSTM_F, 8, 8)},
             _lstm_call, _lstm_ref, {'conv.weight': [('input_half', LSTM_F)]}, F22, (True, True)),
    ]
)
FORM_IDS = [f.name for f in FORMS]
assert len(set(FORM_IDS)) == len(FORM_IDS)


# ---- the writers -------------------------------------------------------------------------------------------------------------------

def plant_gradients(module, seed=31):
    g = torch.Generator().manual_seed(seed)
    for p in module.parameters():
        p.grad = torch.randn(p.shape, generator=g).to(p.device)


def _adam(module):
    return torch.optim.Adam(module.parameters(), lr=LR, betas=(0.5, 0.999))


def write_adam(case, check):
    """1: torch.optim.Adam.step() -- moves the version counters"""
    plant_gradients(case.module)
    _adam(case.module).step()
    check('after Adam.step()')


def _fused(case, guard=None):
    fs = fused_step.FusedStep(case.device, 10, guard=guard)
    fs.attach('G', case.module, _adam(case.module))
    return fs


def write_fused_step(case, check):
    """2: FusedStep.step -- tai_fused_step through raw pointers on the device, host_step through numpy views on the host"""
    before = [p.detach().clone() for p in case.module.parameters()]
    versions = [p._version for p in case.module.parameters()]
    plant_gradients(case.module)
    fs = _fused(case)
    fs.step('G', True)
    fs.read(wait=True)
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, case.module.parameters())), 'the fused step moved nothing'
    check('after FusedStep.step (version counters %s)' % ('moved' if versions != [p._version for p in case.module.parameters()] else 'did not move'))


def write_fused_step_skipped(case, check):
    """3: FusedStep.step with a planted NaN gradient and a guard: the verdict is "skipped", the weights stay"""
    before = [p.detach().clone() for p in case.module.parameters()]
    plant_gradients(case.module)
    next(iter(case.module.parameters())).grad.view(-1)[:2] = float('nan')
    guard = grad_guard.GradGuard(patience=5)
    fs = _fused(case, guard)
    fs.step('G', True)
    fs.read(wait=True)
    assert guard.verdict['G'] == grad_guard.SKIPPED and guard.skipped['G'] == 1
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, case.module.parameters())), 'a skipped step wrote the weights'
    check('after a skipped FusedStep.step')


def stub_env(module, ema):
    """What fused_step.averaged_weights reads of an environment"""
    return types.SimpleNamespace(generator=module, fused=types.SimpleNamespace(ema=ema, ema_decay=0.9))


def write_averaged_weights(case, check):
    """4: averaged_weights: p.data exchanged with other values on the way in, and back on the way out"""
    ema = collections.OrderedDict((n, v.to(case.device).reshape(-1)) for n, v in new_values(case.module, 41).items())
    with fused_step.averaged_weights(stub_env(case.module, ema)):
        check('inside averaged_weights')
    check('after averaged_weights')


def write_load_state_dict(case, check):
    """5"""
    case.module.load_state_dict(new_values(case.module, 42))
    check('after load_state_dict')


def write_weights_init(case, check):
    """6: the package's own re-initialisation (Xavier-normal weights, zero biases)"""
    torch.manual_seed(43)
    case.module.apply(util.weights_init)
    check('after weights_init')


def _data_copy(case, seed):
    for p, v in zip(case.module.parameters(), new_values(case.module, seed).values()):
        p.data.copy_(v)


def write_data_copy_invalidate_module(case, check):
    """7: a write through .data moves neither the counter nor the pointer; the writer says so for its module"""
    _data_copy(case, 44)
    conv_ops.invalidate_derived(case.module)
    check('after p.data.copy_ and invalidate_derived(module)')


def write_data_copy_invalidate_all(case, check):
    """8: ... or for every weight"""
    _data_copy(case, 45)
    conv_ops.invalidate_derived()
    check('after p.data.copy_ and invalidate_derived()')


def write_no_grad_copy(case, check):
    """9"""
    with torch.no_grad():
        for p, v in zip(case.module.parameters(), new_values(case.module, 46).values()):
            p.copy_(v)
    check('after p.copy_ under no_grad')


def write_data_assign(case, check):
    """10: p.data = other: the storage moves"""
    for p, v in zip(case.module.parameters(), new_values(case.module, 47).values()):
        p.data = v.to(p.device)
    check('after p.data = other')


def write_arithmetic_switch(case, check):
    """11: not a weight write, but the F(2x2, 3x3) tags carry the arithmetic: to bf16x3, a weight write there, and back -- the fp32
    image cached before the switch is then one of an earlier weight"""
    prev = conv_ops.set_winograd_arithmetic('bf16x3')
    try:
        check('under bf16x3')
        with torch.no_grad():
            for p, v in zip(case.module.parameters(), new_values(case.module, 48).values()):
                p.copy_(v)
        check('under bf16x3 after a write')
    finally:
        conv_ops.set_winograd_arithmetic(prev)
    check('back on fp32')


def write_broadcast(case, check):
    """12, CPU only: parallel.broadcast_module_state in a single-rank gloo group on a FileStore under tmp_path.  With one rank there is
    nobody to receive from: the call writes nothing, and the forms stay valid (and right)."""
    import torch.distributed as dist
    from video_frame_inpainting_amd import parallel
    store = dist.FileStore(os.path.join(str(case.tmp_path), 'store'), 1)
    dist.init_process_group('gloo', store=store, rank=0, world_size=1)
    try:
        parallel.broadcast_module_state(case.module)
    finally:
        dist.destroy_process_group()
    check('after broadcast_module_state in a group of one')


Writer = collections.namedtuple('Writer', 'number name fn writes rebuilds')
# writes: per check, whether the weights differ from those at the check before (the discriminating-write condition is asked there);
# rebuilds: per check, how many times a counting ``make`` runs at that check (the _cached contract)
WRITERS = [
    Writer(1, 'adam', write_adam, (True,), (1,)),
    Writer(2, 'fused_step', write_fused_step, (True,), (1,)),
    Writer(3, 'fused_step_skipped', write_fused_step_skipped, (False,), (1,)),
    Writer(4, 'averaged_weights', write_averaged_weights, (True, True), (1, 1)),
    Writer(5, 'load_state_dict', write_load_state_dict, (True,), (1,)),
    Writer(6, 'weights_init', write_weights_init, (True,), (1,)),
    Writer(7, 'data_copy_invalidate_module', write_data_copy_invalidate_module, (True,), (1,)),
    Writer(8, 'data_copy_invalidate_all', write_data_copy_invalidate_all, (True,), (1,)),
    Writer(9, 'no_grad_copy', write_no_grad_copy, (True,), (1,)),
    Writer(10, 'data_assign', write_data_assign, (True,), (1,)),
    Writer(11, 'arithmetic_switch', write_arithmetic_switch, (False, True, False), None),
    Writer(12, 'broadcast_one_rank', write_broadcast, (False,), (0,)),
]
WRITER = {w.name: w for w in WRITERS}


def pairs(on_gpu):
    """The (form, writer) pairs that make sense.  Writers 1 and 5-10 on every form; 2-4 (the fused step, a skipped one, the weight
    average) on every form a training or validation run reaches (the bf16 kernel is inference only); 11 on the forms whose tags carry
    the F(2x2, 3x3) arithmetic; 12 without a GPU only."""
    out = []
    for f in FORMS:
        for w in WRITERS:
            if w.number in (2, 3, 4) and not f.trained:
                continue
            if w.number == 11 and not f.f22:
                continue
            if w.number == 12 and on_gpu:
                continue
            out.append((f, w))
    return out


def pair_id(pair):
    return '%s-%s' % (pair[0].name, pair[1].name)


def max_abs(t):
    return float(t.detach().abs().max())
