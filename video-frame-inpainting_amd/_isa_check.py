"""Invariants of the GENERATED device code that the library's correctness depends on and that a different compiler could break
without any source change: checked on the assembly of the very compile that produces the library (_native.build keeps
it with -save-temps=obj) and refused if violated; tests/test_wino_isa.py runs the same checks and feeds them doctored text.

wino43::conv3x3_gen and conv3x3_wrw_gen (the F(4x4, 3x3) kernel and its weight-gradient form): the chunk loop is one asm statement with fixed registers v0-v99 and
   a[0:143]; the compiler must give the kernel no scratch, no spill, and registers for two waves per SIMD (<= 256 in all): a
   spill would be vector-memory traffic the statement's own s_waitcnt vmcnt counting does not expect.
   (Round 4's compiler-scheduled forms of that kernel, whose asm loads depended on the compiler not touching their destination registers
   before a wait it could not see, are gone: every load of the kernel is inside the statement now.)

fstep::step_segments (the fused optimizer step, csrc/fused_step.hip.inc): its arithmetic is a written definition of single IEEE fp32
   operations.  Contraction is switched off in the source; what the compiler may still add are the fused multiply-adds INSIDE its
   correctly rounded division (five each) and square root (two each, the next-up / next-down residual test behind v_sqrt_f32).  So the
   number of fp32 fma / fmac / mad instructions must be exactly 5 x divisions + 2 x square roots -- one more would be a contracted
   a * b + c of the definition -- every square root must be the refined form, and there is no scratch.
   fstep::step_segments_decay (the same step with the weight-decay line, tai_fused_step_decay): the same rule under its own name
   (check_fused_step_decay, part of check()): its decay line must stay a multiplication and a subtraction.
"""
import re

_KERNEL = re.compile(r'^(_Z\w+):', re.M)


def kernels(asm, prefix):
    """{mangled name: (body lines, descriptor text)} of the kernels whose mangled name starts with ``prefix``."""
    out = {}
    for m in _KERNEL.finditer(asm):
        name = m.group(1)
        if not name.startswith(prefix) or name in out:
            continue
        end = asm.find('.end_amdhsa_kernel', m.start())
        if end < 0:
            continue
        body = asm[m.start():end]
        cut = body.find('.amdhsa_kernel')
        out[name] = (body[:cut].splitlines(), body[cut:])
    return out


def _regs(text):
    """vector registers an operand string mentions"""
    found = set(int(n) for n in re.findall(r'\bv(\d+)\b', text))
    for a, b in re.findall(r'\bv\[(\d+):(\d+)\]', text):
        found.update(range(int(a), int(b) + 1))
    return found


def check(asm):
    """-> list of violations (empty: the library may be installed)."""
    bad = []
    gen = kernels(asm, '_ZN6wino4311conv3x3_gen')
    if not gen:
        bad.append('no wino43::conv3x3_gen kernel in the assembly')
    wrw = kernels(asm, '_ZN6wino4315conv3x3_wrw_gen')       # the weight-gradient form of the same statement: the same rules
    if not wrw:
        bad.append('no wino43::conv3x3_wrw_gen kernel in the assembly')
    gen.update(wrw)
    for name, (lines, desc) in gen.items():
        get = lambda key: int(re.search(r'\.amdhsa_%s\s+(\d+)' % key, desc).group(1))
        if get('private_segment_fixed_size') != 0 or any(re.search(r'\bscratch_(load|store)', l) for l in lines):
            bad.append('%s: scratch memory in use (spills next to the asm chunk loop)' % name)
        if get('next_free_vgpr') > 256:
            bad.append('%s: %d registers: two waves per SIMD do not fit' % (name, get('next_free_vgpr')))
        if get('next_free_vgpr') - get('accum_offset') < 144:
            bad.append('%s: fewer than 144 accumulator registers' % name)
        n = sum(1 for l in lines if 'v_mfma_f32_16x16x4_f32' in l)
        var = re.match(r'_ZN6wino4311conv3x3_genILin?\d+ELin?\d+ELi(\d+)E', name)
        if var and var.group(1) != '0':      # <ACT, EPI, VAR != 0>: a timing ablation of the tools build (parts of the loop left out on purpose)
            continue
        # chunk bodies of 36 MFMAs: per role one with the next chunk's loads / DMA and the plain one; the weight-gradient form's third role
        # transforms between the MFMA groups and has a third body (a next chunk, none behind it)
        want = 252 if name in wrw else 216
        if n != want:
            bad.append('%s: %d MFMAs in the chunk loops, expected %d' % (name, n, want))
    return bad + check_fused_step_decay(asm)


def check_fused_step(asm):
    """-> list of violations of the fused optimizer step's kernels (see the module's docstring)."""
    found = kernels(asm, '_ZN5fstep13step_segments')
    bad = []
    if len(found) != 2:
        bad.append('expected two fstep::step_segments kernels (plain and non-temporal loads), found %d' % len(found))
    return bad + _step_arithmetic(found)


def check_fused_step_decay(asm):
    """-> list of violations of fstep::step_segments_decay (tai_fused_step_decay): the same rule under its own name."""
    found = kernels(asm, '_ZN5fstep19step_segments_decay')
    bad = []
    if len(found) != 1:
        bad.append('expected one fstep::step_segments_decay kernel, found %d' % len(found))
    return bad + _step_arithmetic(found)


def _step_arithmetic(found):
    bad = []
    for name, (lines, desc) in found.items():
        ops = [l.split()[0] for l in lines if l.startswith('\t') and l.split() and l.split()[0].startswith(('v_', 'scratch_'))]
        count = lambda *prefixes: sum(1 for o in ops if o.startswith(prefixes))
        if int(re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', desc).group(1)) != 0 or count('scratch_'):
            bad.append('%s: scratch memory in use' % name)
        fused = count('v_fma_f32', 'v_fmac_f32', 'v_mad_f32', 'v_mac_f32', 'v_pk_fma_f32', 'v_fma_mix', 'v_fmaak_f32', 'v_fmamk_f32')
        divisions, roots = count('v_div_fixup_f32'), count('v_sqrt_f32')
        if divisions == 0 or roots == 0 or count('v_div_fmas_f32') != divisions:
            bad.append('%s: no IEEE division / square root sequence found (%d v_div_fixup_f32, %d v_sqrt_f32)' % (name, divisions, roots))
        if fused != 5 * divisions + 2 * roots:
            bad.append('%s: %d fused multiply-adds for %d divisions and %d square roots (5 and 2 each expected): the arithmetic of the '
                       'definition was contracted, or the division / square root is not the correctly rounded form' % (name, fused, divisions, roots))
        if count('v_rsq_f32', 'v_rcp_iflag'):
            bad.append('%s: an approximate reciprocal square root in the step arithmetic' % name)
    return bad
