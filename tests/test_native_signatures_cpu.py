"""The ctypes signatures _native.lib() sets are those of include/tai_sepconv.h: derived from the prototypes, never restated by hand."""
import ctypes
import re

import pytest

from video_frame_inpainting_amd import _native

P = V = ctypes.c_void_p
I, LL, Fl = ctypes.c_int, ctypes.c_longlong, ctypes.c_float


def _prototypes():
    return dict((name, params) for name, params in re.findall(r'\b(tai_\w+)\s*\(([^)]*)\)\s*;', _native._header_text()))


def test_every_declared_symbol_has_the_signature_of_its_prototype():
    L, protos = _native.lib(), _prototypes()
    assert sorted(protos) == _native.declared_symbols() and len(protos) >= 86
    for name, params in protos.items():
        entry = getattr(L, name)
        n = 0 if params.strip() in ('', 'void') else params.count(',') + 1
        assert entry.argtypes is not None and len(entry.argtypes) == n, name
        assert entry.restype in (I, LL, ctypes.c_char_p), name


def test_literal_pins():
    L = _native.lib()
    assert L.tai_unpool2x_add.argtypes == [P, P, P, LL, I, I, V]
    assert L.tai_image_loss.argtypes == [P, I, P, I, Fl, P, P, P, P, LL, I, I, V]
    assert L.tai_step_verdict.argtypes == [P, P, I, ctypes.c_double, I, I, LL, LL, P, V]
    assert len(L.tai_conv3x3_wino43_forward_blocks.argtypes) == 21
    assert L.tai_sepconv_last_error.argtypes == [] and L.tai_sepconv_last_error.restype is ctypes.c_char_p
    assert L.tai_unpool2x_add.restype is I and L.tai_conv3x3_wino_weight_floats.restype is LL


def test_the_parser_on_prototypes_given_as_text():
    sigs = _native.signatures('const char* tai_a(void);\nlong long tai_b(int, long long n, const float* const* xs,\n double d, float);')
    assert sigs == {'tai_a': (ctypes.c_char_p, []), 'tai_b': (LL, [I, LL, P, ctypes.c_double, Fl])}


@pytest.mark.parametrize('proto', ['int tai_x(unsigned n, float* y);', 'size_t tai_x(int n);', 'int tai_x(float y[4]);',
                                   'int tai_x(long n);'])
def test_an_unknown_type_raises_and_names_the_prototype(proto):
    with pytest.raises(_native.NativeLibraryError, match=r'tai_x\('):
        _native.signatures(proto)
