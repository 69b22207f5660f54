"""Loader (and in-tree builder) of the C-ABI HIP library ``libtai_sepconv.so``.

The library is the product's only compute backend for the separable convolution: there is no CPU or
eager-PyTorch fallback.  ``lib()`` raises if the shared object is missing or lacks a symbol that
``include/tai_sepconv.h`` declares.
"""
import ctypes
import os
import re
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
LIB_PATH = os.path.join(_PKG, 'libtai_sepconv.so')
HEADER = os.path.join(_ROOT, 'include', 'tai_sepconv.h')
CSRC = os.path.join(_PKG, 'csrc')
MAIN_SOURCE = os.path.join(CSRC, 'sepconv_capi.hip')          # the one translation unit; it #includes every *.inc
GENERATED = os.path.join(CSRC, 'sepconv_fwd_rowloop.inc')     # written by tools/gen_fwd_asm.py
GENERATORS = (('gen_fwd_asm.py', GENERATED),                  # (generator under tools/, the include it writes)
              ('gen_wino43_asm.py', os.path.join(CSRC, 'wino43_chunkloop.inc')))


def sources(csrc=None):
    """Every source file under csrc/ (*.hip, *.inc): the staleness check and the source hash cover whatever the translation
    unit includes, listed or not.  Editor backups and the generator's transient '<name>.tmp.<pid>' are not sources."""
    csrc = csrc or CSRC
    return sorted(os.path.join(csrc, f) for f in os.listdir(csrc)
                  if f.endswith(('.hip', '.inc')) and not f.startswith('.') and '.tmp.' not in f)


def source_hash(csrc=None, header=None):
    """SHA-256 over (file name, length, bytes) of every source under csrc/ and of include/tai_sepconv.h, in sorted order: what
    build() compiles into the library (tai_sepconv_source_hash()) and what lib() recomputes from the tree before it trusts a
    binary.  Contents only -- no mtimes, no paths -- so the hash survives the copy to the GPU box."""
    import hashlib
    h = hashlib.sha256()
    for path in sources(csrc) + [header or HEADER]:
        try:
            with open(path, 'rb') as f:
                data = f.read()
        except FileNotFoundError:        # vanished between listdir and open (a concurrent generator run): not a source
            continue
        h.update(os.path.basename(path).encode() + b'\0' + str(len(data)).encode() + b'\0')
        h.update(data)
    return h.hexdigest()


_lib = None


class NativeLibraryError(RuntimeError):
    pass


def _header_text():
    """include/tai_sepconv.h without comments and preprocessor lines: what is left is the prototypes."""
    text = open(HEADER).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'//[^\n]*', '', text)
    return re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)


def declared_symbols():
    """Function names declared in include/tai_sepconv.h."""
    return sorted(set(re.findall(r'\b(tai_\w+)\s*\(', _header_text())))


_CTYPES = {'int': ctypes.c_int, 'long long': ctypes.c_longlong, 'float': ctypes.c_float, 'double': ctypes.c_double}
_TYPE_WORDS = ('const', 'void', 'char', 'int', 'long', 'float', 'double', 'unsigned', 'signed', 'short')


def _ctype(decl, proto):
    """ctypes type of a C type as the header writes it.  Every pointer is a c_void_p (data pointers, the stream, ``const float* const*``)
    except ``const char*``, which only the getters return.  A type that is not listed is an error naming the prototype, never a guess."""
    words = re.sub(r'\bconst\b', ' ', decl.replace('*', ' * ')).split()
    if '*' in words:
        return ctypes.c_char_p if words == ['char', '*'] else ctypes.c_void_p
    if ' '.join(words) not in _CTYPES:
        raise NativeLibraryError('include/tai_sepconv.h: no ctypes type for `%s` in `%s`' % (decl.strip(), proto))
    return _CTYPES[' '.join(words)]


def signatures(text=None):
    """{name: (restype, argtypes)} of every prototype in the header (or in ``text``, prototypes given as a string)."""
    sigs = {}
    for ret, name, params in re.findall(r'([\w \t\*]+?)\b(tai_\w+)\s*\(([^)]*)\)\s*;', _header_text() if text is None else text):
        proto = '%s %s(%s)' % (ret.strip(), name, ' '.join(params.split()))
        params = [] if params.strip() in ('', 'void') else [p.strip() for p in params.split(',')]
        # `float* y`, `long long planes`, `int`: the last word is the parameter's name unless it is part of the type
        last = [re.search(r'\w+$', p) for p in params]
        types = [p if m is None or m.group() in _TYPE_WORDS else p[:m.start()] for p, m in zip(params, last)]
        sigs[name] = (_ctype(ret, proto), [_ctype(t, proto) for t in types])
    return sigs


TIMING_LIB_PATH = os.path.join(_ROOT, 'build', 'libtai_sepconv_timing.so')


def build(force=False, verbose=False, timing=False):
    """hipcc --offload-arch=gfx950 -> video-frame-inpainting_amd/libtai_sepconv.so (cross-compiles without a GPU).
    ``timing=True`` builds build/libtai_sepconv_timing.so instead: the same sources with -DTAI_TIMING_VARIANTS, i.e. with
    the timing experiments (forward variants >= 100, Winograd timeline skip levels) that the shipped library leaves out;
    only tools/ links or loads it."""
    out = TIMING_LIB_PATH if timing else LIB_PATH
    regenerate()
    want = source_hash()
    if not force and os.path.exists(out) and embedded_source_hash(out) == want:
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # the old binary goes first: a compile that fails must leave NOTHING to load (round 3's one GPU fault was a stale library
    # that survived a failed rebuild); the new one is written beside the target and renamed over it only when hipcc succeeded
    if os.path.exists(out):
        os.remove(out)
    # compiled in a directory of its own with -save-temps=obj: the device assembly of THIS compile is checked before the library is
    # installed (_isa_check: properties of the generated code that a different hipcc could break with no source change)
    import shutil
    work = os.path.join(_ROOT, 'build', 'obj.%s.%d' % ('timing' if timing else 'lib', os.getpid()))
    os.makedirs(work, exist_ok=True)
    tmp = os.path.join(work, os.path.basename(out))
    cmd = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-fno-slp-vectorize', '-w', '-save-temps=obj',
           '-I' + os.path.join(_ROOT, 'include'), '-DTAI_SOURCE_HASH="%s"' % want, '-o', tmp, MAIN_SOURCE] + \
          (['-DTAI_TIMING_VARIANTS'] if timing else [])
    if verbose:
        print(' '.join(cmd))
    try:
        subprocess.check_call(cmd)
        if source_hash() != want:
            raise NativeLibraryError('csrc/ changed while %s was compiling: build again' % os.path.basename(out))
        asm = os.path.join(work, 'sepconv_capi-hip-amdgcn-amd-amdhsa-gfx950.s')
        from . import _isa_check
        violations = _isa_check.check(open(asm).read()) + _isa_check.check_fused_step(open(asm).read())
        if violations:
            raise NativeLibraryError('the device code hipcc generated for %s breaks an invariant the kernels rely on; the library is NOT '
                                     'installed:\n  %s' % (os.path.basename(out), '\n  '.join(violations[:20])))
        if not timing:          # kept for tools/isa_fn.py and a look at what the compiler did
            os.replace(asm, os.path.join(_ROOT, 'build', 'sepconv_capi-hip-amdgcn-amd-amdhsa-gfx950.s'))
        os.replace(tmp, out)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return out


def embedded_source_hash(path):
    """The hash a built library carries, read from the FILE (the marker 'TAI_SOURCE_HASH=' in front of it): nothing is mapped, so
    a binary about to be refused never runs a constructor, and dlopen's by-name cache cannot answer for a file that was rebuilt
    since.  None if the file is missing or carries no hash (any library from before this check)."""
    try:
        with open(path, 'rb') as f:
            data = f.read()
    except OSError:
        return None
    m = re.search(rb'TAI_SOURCE_HASH=([0-9a-f]{64})\0', data)
    return m.group(1).decode() if m else None


def verify(path, csrc=None, header=None):
    """Raise NativeLibraryError unless the library at `path` was compiled from exactly the sources in the tree."""
    have, want = embedded_source_hash(path), source_hash(csrc, header)
    if have != want:
        raise NativeLibraryError(
            '%s was not built from the sources next to it (library: %s, tree: %s): a stale binary must not run -- rebuild with '
            '`python -c "import __graft_entry__ as g; g.build()"`' % (path, have, want))


def regenerate():
    """Re-run the asm generators whose script is newer than its output.  A generator writes a temporary file and renames
    it over the target, so a concurrent hipcc never reads a half-written include."""
    for name, out in GENERATORS:
        gen = os.path.join(_ROOT, 'tools', name)
        if os.path.exists(gen) and (not os.path.exists(out) or os.path.getmtime(gen) > os.path.getmtime(out)):
            subprocess.check_call(['python3', gen], stdout=subprocess.DEVNULL)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    path = LIB_PATH
    if os.environ.get('TAI_NATIVE_TIMING_LIB') == '1':     # tools/ only: the build with the timing experiments compiled in
        path = TIMING_LIB_PATH
    if not os.path.exists(path):
        raise NativeLibraryError(
            '%s is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(there is no fallback path for the separable convolution)' % path)
    import torch  # noqa: F401  -- load torch's HIP runtime first so this library binds to the same libamdhip64
    verify(path)
    L = ctypes.CDLL(path)
    missing = [s for s in declared_symbols() if not hasattr(L, s)]
    if missing:
        raise NativeLibraryError('%s does not export %s' % (path, missing))
    for name, (restype, argtypes) in signatures().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    _lib = L
    return L


def check(rc, what):
    if rc != 0:
        raise RuntimeError('%s failed (%d): %s' % (what, rc, lib().tai_sepconv_last_error().decode()))


def launch(name, device, *args):
    """Call the entry ``name`` on ``device``'s current stream and raise unless it returns 0: the entries whose last parameter is the
    stream.  Tensors among ``args`` go as their data pointer and None as a null pointer; ints, floats and ctypes pointer arrays pass
    through.  (The entries without a stream -- *_floats, *_workspace_bytes, *_splits, set_*, get_* -- are called on lib() directly.)"""
    import torch
    with torch.cuda.device(device):
        check(getattr(lib(), name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args],
                                   torch.cuda.current_stream(device).cuda_stream), name)
