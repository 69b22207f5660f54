"""Which launches a layer gets: conv_bias_act, conv_bias_act_maxpool, conv_bias_unpool_add and motion_enc_chain driven without a device
over a table of layers, and the sequence of C-ABI entries, ATen fallbacks and autograd Functions each call reaches compared, by equality,
with tests/golden/conv_routes.json.  The golden table was recorded by this harness (``python tests/test_conv_routes_cpu.py OUT.json CHECKOUT``, CHECKOUT a built
checkout of that commit) at commit 395d83e, the parent of the change that introduced conv_ops.conv_route; it states
what the dispatch did before that change and is not regenerated from the code it checks.

Stand-ins: the tensors are a torch.Tensor subclass on the ``meta`` device that says is_cuda (data_ptr() of a meta tensor is 0); the
library is a proxy that records the name of every tai_* entry called and returns 0, and hands the host-only queries (*_floats, *_elems,
*_splits, *_workspace_*) to the real library; F.conv2d, torch.cat and the ``apply`` of the autograd Functions record their names and
return a stand-in of the right shape."""
import contextlib
import functools
import json
import os
import re
import sys
import weakref
from types import SimpleNamespace

import torch

if __name__ == '__main__':            # recording: OUT.json [checkout whose package is driven; default: this one]
    sys.path.insert(0, sys.argv[2] if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from video_frame_inpainting_amd import _native, conv_ops  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_routes.json')

# (N, Ci, Co, H, W, k); the last one with its weight marked by mark_outside_recurrence
LAYERS = [(32, 1, 64, 128, 128, 5), (32, 64, 64, 128, 128, 3), (32, 64, 128, 64, 64, 5), (32, 128, 256, 32, 32, 7), (32, 256, 256, 32, 32, 3),
          (32, 3, 64, 128, 128, 3), (32, 64, 1, 128, 128, 3), (32, 64, 3, 128, 128, 3), (160, 512, 512, 4, 4, 3), (2, 64, 64, 8, 8, 3),
          (16, 64, 64, 15, 20, 3), (32, 16, 16, 64, 64, 3), (32, 512, 256, 16, 16, 3), (32, 64, 64, 30, 40, 3)]
MARKED = (64, 256, 128, 16, 16, 3)
SWITCHES = ('default', 'ragged_off', 'parts_off', 'bf16x3')
FUNCTIONS = ('_WinoConv3x3', '_WinoConv3x3Parts', '_WinoConvKxK', '_ThinInConv', '_ThinOutConv', '_ActPool2x2')
# every one of these occurs in at least one recorded signature: the table is not vacuous
MUST_OCCUR = ('tai_conv_bf16_forward', 'tai_conv3x3_wino_forward', 'tai_conv3x3_wino_forward_ex', 'tai_conv3x3_wino_forward_parts',
              'tai_conv3x3_wino_forward_maxpool', 'tai_conv3x3_wino_forward_window', 'tai_conv_shift_stack',
              'tai_conv3x3_wino43_forward_ws', 'tai_conv_cin1_forward', 'tai_conv_cin1_forward_maxpool', 'tai_conv_cout1_3x3_forward',
              'tai_bias_act_inplace', 'tai_unpool2x_add', 'tai_conv_cin1_forward_maxpool_window', 'tai_conv3x3_wino43_forward_blocks',
              'F.conv2d', 'torch.cat') + FUNCTIONS
_HOST_ONLY = re.compile(r'_(floats|elems|splits)$|_workspace_')


class Fake(torch.Tensor):
    is_cuda = property(lambda self: True)


def fake(*shape, grad=False):
    t = torch.empty(shape, device='meta').as_subclass(Fake)
    return t.requires_grad_(grad)


def _plain(t):
    return torch.empty(t.shape, device='meta')


class Harness(object):
    """Installs the stand-ins (``with Harness() as h``) and records into ``h.calls`` / ``h.routes``."""

    def __init__(self):
        self.calls, self.routes, self._undo = [], [], []

    def _set(self, obj, name, value):
        self._undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def __enter__(self):
        real, calls = _native.lib(), self.calls

        class Proxy(object):
            def __getattr__(self, name):
                if _HOST_ONLY.search(name):
                    return getattr(real, name)

                def entry(*args):
                    calls.append(name)
                    return 0
                return entry
        proxy = Proxy()
        self._set(_native, 'lib', lambda: proxy)
        self._set(_native, 'check', lambda rc, what: None)
        self._set(torch.cuda, 'device', lambda d: contextlib.nullcontext())
        self._set(torch.cuda, 'current_stream', lambda d=None: SimpleNamespace(cuda_stream=None))
        self._set(weakref, 'finalize', lambda *a, **k: None)

        def out(n, c, h, w):
            return fake(n, c, h, w).requires_grad_(torch.is_grad_enabled())
        shapes = {
            '_WinoConv3x3': lambda x, w, b, act, tr: out(x.shape[0], w.shape[1 if tr else 0], x.shape[2], x.shape[3]),
            '_WinoConv3x3Parts': lambda w, b, act, tr, *parts: out(parts[0].shape[0], w.shape[1 if tr else 0], parts[0].shape[2], parts[0].shape[3]),
            '_WinoConvKxK': lambda x, w, b, act: out(x.shape[0], w.shape[0], x.shape[2], x.shape[3]),
            '_ThinInConv': lambda x, w, b, act: out(x.shape[0], w.shape[0], x.shape[2], x.shape[3]),
            '_ThinOutConv': lambda x, w, b, act, tr: out(x.shape[0], 1, x.shape[2], x.shape[3]),
            '_ActPool2x2': lambda z, relu: (out(*z.shape), out(z.shape[0], z.shape[1], z.shape[2] // 2, z.shape[3] // 2)),
        }

        def recording(name, shape):
            def apply(*args):
                calls.append(name)
                return shape(*args)
            return staticmethod(apply)
        for name in FUNCTIONS:
            self._set(getattr(conv_ops, name), 'apply', recording(name, shapes[name]))
        conv2d, cat = conv_ops.F.conv2d, torch.cat

        def fake_conv2d(x, w, b=None, stride=1, padding=0):
            calls.append('F.conv2d')
            return conv2d(_plain(x), _plain(w), None, stride=stride, padding=padding).as_subclass(Fake)

        def fake_cat(ts, dim=0):
            calls.append('torch.cat')
            return cat([_plain(t) for t in ts], dim=dim).as_subclass(Fake)
        self._set(conv_ops.F, 'conv2d', fake_conv2d)
        self._set(torch, 'cat', fake_cat)
        route = getattr(conv_ops, 'conv_route', None)
        if route is not None:
            def recording_route(*a, **k):
                name = route(*a, **k)
                self.routes.append(name)
                return name
            self._set(conv_ops, 'conv_route', recording_route)
        self._saved = (conv_ops._CONV_PREC[0], conv_ops._WINO_TILE[0], conv_ops._WINO_ARITH[0], conv_ops.RAGGED_ROUTES[0],
                       conv_ops.PARTS_UNDER_AUTOGRAD, dict(conv_ops._HALO_PLANES))
        return self

    def __exit__(self, *exc):
        for obj, name, value in reversed(self._undo):
            setattr(obj, name, value)
        (conv_ops._CONV_PREC[0], conv_ops._WINO_TILE[0], conv_ops._WINO_ARITH[0], conv_ops.RAGGED_ROUTES[0],
         conv_ops.PARTS_UNDER_AUTOGRAD, planes) = self._saved
        conv_ops._HALO_PLANES.clear()
        conv_ops._HALO_PLANES.update(planes)

    def run(self, fn):
        """-> (signature, route names) of one call"""
        del self.calls[:], self.routes[:]
        fn()
        return '+'.join(self.calls), tuple(self.routes)


def _switch(name):
    conv_ops.RAGGED_ROUTES[0] = name != 'ragged_off'
    conv_ops.PARTS_UNDER_AUTOGRAD = name != 'parts_off'
    conv_ops._WINO_ARITH[0] = 1 if name == 'bf16x3' else 0      # what set_winograd_arithmetic leaves on the Python side


def layer_cases(layer, marked=False):
    """The calls made for one layer under one (switch, precision, tile) setting, in a fixed order: [(id, thunk)]."""
    N, Ci, Co, H, W, k = layer
    cases = []
    for grad in (False, True):
        for transposed in (False, True):
            for act in (None, 'relu', 'tanh'):
                for nparts in (1, 2, 4):
                    if Ci % nparts:
                        continue

                    def args(grad=grad, transposed=transposed, nparts=nparts):
                        w = fake(Ci, Co, k, k, grad=grad) if transposed else fake(Co, Ci, k, k, grad=grad)
                        if marked:
                            conv_ops.mark_outside_recurrence(SimpleNamespace(parameters=lambda: [w]))
                        xs = [fake(N, Ci // nparts, H, W) for _ in range(nparts)]
                        return (xs if nparts > 1 else xs[0]), w, fake(Co, grad=grad)

                    def call(fn, grad=grad):
                        def thunk():
                            with (torch.enable_grad() if grad else torch.no_grad()):
                                fn()
                        return thunk
                    tag = 'grad%d/T%d/%s/parts%d/' % (grad, transposed, act, nparts)
                    cases.append((tag + 'conv', call(
                        lambda args=args, act=act, transposed=transposed: conv_ops.conv_bias_act(*args(), k // 2, act, transposed=transposed))))
                    cases.append((tag + 'conv_out', call(
                        lambda args=args, act=act, transposed=transposed: conv_ops.conv_bias_act(*args(), k // 2, act, transposed=transposed,
                                                                                                 out=fake(N, Co, H, W)))))
                    if not transposed:
                        cases.append((tag + 'pool', call(lambda args=args, act=act: conv_ops.conv_bias_act_maxpool(*args(), k // 2, act))))
                    if not transposed and act is None and H % 2 == 0 and W % 2 == 0:
                        for keep in (True, False):
                            cases.append((tag + 'unpool_add/keep%d' % keep, call(
                                lambda args=args, keep=keep: conv_ops.conv_bias_unpool_add(*args(), k // 2, fake(N, Co, H // 2, W // 2),
                                                                                           keep_plain=keep))))
    return cases


def chain_cases():
    """motion_enc_chain: MotionEnc at 32 x 128 x 128, gf 64 (the 4 x 4 tile's displaced blocks / the F(2x2) general entry), and a width and
    a grad mode it refuses."""
    def conv(co, ci, k, grad=False):
        return SimpleNamespace(weight=fake(co, ci, k, k, grad=grad), bias=fake(co, grad=grad), padding=(k // 2, k // 2))
    cases = []
    for g, grad in ((64, False), (16, False), (8, False), (64, True)):
        def thunk(g=g, grad=grad):
            with (torch.enable_grad() if grad else torch.no_grad()):
                conv_ops.motion_enc_chain(fake(32, 1, 128, 128), conv(g, 1, 5, grad), conv(2 * g, g, 5, grad), conv(4 * g, 2 * g, 7, grad))
        cases.append(('gf%d/grad%d' % (g, grad), thunk))
    return cases


def groups():
    """[(group id, [(case id, thunk)])]: a group is one (layer, switch, precision, tile) setting, applied before its calls run."""
    out = []
    for switch in SWITCHES:
        for prec in ('fp32', 'bf16'):
            for tile in (4, 2):
                def setting(switch=switch, prec=prec, tile=tile):
                    _switch(switch)
                    conv_ops._CONV_PREC[0], conv_ops._WINO_TILE[0] = prec, tile
                for layer in LAYERS + [MARKED]:
                    marked = layer is MARKED
                    gid = '%s/%s/tile%d/%s%s' % (switch, prec, tile, 'x'.join(map(str, layer)), '/marked' if marked else '')
                    out.append((gid, setting, layer_cases(layer, marked)))
                out.append(('%s/%s/tile%d/motion_enc_chain' % (switch, prec, tile), setting, chain_cases()))
    return out


@functools.lru_cache(maxsize=None)
def record():
    """-> ({group id: [signature per case]}, {(case kind, route names): set of signatures})"""
    table, by_route = {}, {}
    with Harness() as h:
        for gid, setting, cases in groups():
            setting()
            row = []
            for cid, thunk in cases:
                sig, routes = h.run(thunk)
                row.append(sig)
                if routes:
                    by_route.setdefault((cid.split('/')[-1], routes), set()).add(sig)
            table[gid] = row
    return table, by_route


def _load():
    with open(GOLDEN) as f:
        doc = json.load(f)
    return {gid: [doc['signatures'][i] for i in row] for gid, row in doc['table'].items()}


def test_every_layer_takes_the_recorded_launches():
    golden = _load()
    table, _ = record()
    assert sorted(table) == sorted(golden)
    ids = {gid: [cid for cid, _ in cases] for gid, _, cases in groups()}
    wrong = [(gid, ids[gid][i], golden[gid][i], sig) for gid, row in table.items() if row != golden[gid]
             for i, sig in enumerate(row) if len(row) != len(golden[gid]) or sig != golden[gid][i]]
    assert not wrong, '%d cases differ; the first (group, case, recorded, now): %s' % (len(wrong), wrong[:5])


def test_the_recorded_table_is_not_vacuous():
    golden = _load()
    names = set(n for row in golden.values() for sig in row for n in sig.split('+'))
    assert not [n for n in MUST_OCCUR if n not in names]
    assert len(set(sig for row in golden.values() for sig in row)) >= 43


def test_a_route_name_is_one_sequence_of_launches():
    """The names conv_route returned during a call (a call that falls back to another entry point asks more than once) determine the
    launches of that call: the relation from route names to recorded signatures is a function."""
    _, by_route = record()
    assert len(by_route) > 20
    assert not {k: sorted(v) for k, v in by_route.items() if len(v) != 1}
    assert set(name for _, routes in by_route for name in routes) <= set(conv_ops.ROUTES)


if __name__ == '__main__':
    table, _ = record()
    sigs = sorted(set(sig for row in table.values() for sig in row))
    index = {s: i for i, s in enumerate(sigs)}
    with open(sys.argv[1], 'w') as f:
        json.dump({'signatures': sigs, 'table': {gid: [index[s] for s in row] for gid, row in sorted(table.items())}}, f,
                  separators=(',', ':'))
        f.write('\n')
    print('%d groups, %d cases, %d distinct signatures' % (len(table), sum(len(r) for r in table.values()), len(sigs)))
