#!/usr/bin/env python3
"""Compare the kernels of two device assembly files, symbol by symbol:  python tools/device_code_diff.py A.s B.s

For a change that may not touch device code (host-side refactors of the launchers): A.s and B.s are the
`sepconv_capi-hip-amdgcn-amd-amdhsa-gfx950.s` of two builds (_native.build() keeps the shipped build's under build/; hipcc
-save-temps gives any other).  A kernel is its function body ('; -- Begin function' ... '; -- End function') plus its
'.amdhsa_kernel ... .end_amdhsa_kernel' descriptor.  Function-local labels carry the ordinal at which the compiler emitted the
function (.LBB<n>_<m>, .Lfunc_end<n>, inline assembly's %=), which moves when the host code names the kernels in another order, so
labels are compared by their order of definition inside the kernel.  Comment-only lines (first non-blank character ';': 'implicit-def'
notes, loop nests, the resource summary that the descriptor repeats) and the comment behind a label (the IR block's name, numbered
by the compiler's value counter) are dropped before comparing: they move with inlining while the instructions stay put.  Exit status 0 when both files hold the same kernel symbols with identical text, 1 otherwise."""
import re
import sys


def kernels(path):
    text = open(path).read()
    bodies = {}
    for m in re.finditer(r'; -- Begin function (\S+)\n(.*?); -- End function', text, re.S):
        bodies[m.group(1)] = m.group(2)
    out = {}
    for m in re.finditer(r'\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', text, re.S):
        name = m.group(1)
        if name not in bodies:
            sys.exit('%s: kernel descriptor without a function body: %s' % (path, name))
        code = bodies[name] + '\n.amdhsa_kernel\n' + m.group(2)
        code = re.sub(r'^[ \t]*;.*\n', '', code, flags=re.M)
        code = re.sub(r'^([A-Za-z_.$][\w.$]*:)[ \t]*;.*$', r'\1', code, flags=re.M)
        # labels are renamed by their order of definition inside the kernel: the compiler's (.LBB<n>_<m>, .Lfunc_end<n>) and inline
        # assembly's (NAME_%=) carry an ordinal that moves when the host code names the kernels in another order
        order = {}
        for label in re.findall(r'^([A-Za-z_.$][\w.$]*):', code, re.M):
            order.setdefault(label, 'label%d' % len(order))
        code = re.sub(r'[A-Za-z_.$][\w.$]*', lambda t: order.get(t.group(), t.group()), code)
        code = re.sub(r'\bBB\d+_(\d+)', r'BB#_\1', code)             # (the loop comments name blocks without the .L)
        out[name] = re.sub(r'[ \t]+;', ' ;', code)                    # (comments are aligned behind the label, whose length varies)
    return out


def main(a_path, b_path):
    a, b = kernels(a_path), kernels(b_path)
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    print('%s: %d kernels; %s: %d kernels' % (a_path, len(a), b_path, len(b)))
    for title, names in (('only in the first', only_a), ('only in the second', only_b), ('text differs', differ)):
        for name in names:
            print('  %s: %s' % (title, name))
    same = not (only_a or only_b or differ)
    print('identical' if same else 'DIFFERENT')
    return 0 if same else 1


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
