"""tools/isa_diff.py on hand-written assembly (no compiler): what counts as the same code,
and that a kernel missing from the new tree is an error."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tools'))
import isa_diff  # noqa: E402

# the order hipcc emits: the kernel descriptor sits inside the .type ... .size range
KERNEL = '''
\t.protected\t{name}
\t.type\t{name},@function
{name}:                                 ; @{name}
; %bb.0:
\ts_load_dword s{reg}, s[0:1], 0x0      ; a comment
.LBB{n}_1:
\ts_cbranch_scc1 .LBB{n}_1
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_kernarg_size {kernarg}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{n}:
\t.size\t{name}, .Lfunc_end{n}-{name}
'''
FUNC = '''
\t.type\t{name},@function
{name}:
\tv_mov_b32_e32 v0, {imm}
\ts_setpc_b64 s[30:31]
.Lfunc_end{n}:
\t.size\t{name}, .Lfunc_end{n}-{name}
'''


def kernel(name, n=0, reg=2, kernarg=8):
    return KERNEL.format(name=name, n=n, reg=reg, kernarg=kernarg)


def run(old, new):
    lines = []
    bad = isa_diff.compare(isa_diff.symbols(old), isa_diff.symbols(new), 'O', 'N', lines.append)
    return bad, lines


def test_moved_and_renumbered_code_is_same():
    old = {'a.hip': kernel('k1', 0) + kernel('k2', 1) + FUNC.format(name='f', n=2, imm=1)}
    new = {'b.hip': kernel('k2', 0) + FUNC.format(name='f', n=1, imm=1),
           'c.hip': FUNC.format(name='f', n=0, imm=1) + kernel('k1', 1)}
    assert isa_diff.symbols(old)[1] == {'k1', 'k2'}
    bad, lines = run(old, new)
    assert bad == 0
    assert sorted(l.split()[0] for l in lines) == ['SAME'] * 3


def test_changed_code_or_descriptor_is_diff():
    old = {'a.hip': kernel('k1') + kernel('k2') + FUNC.format(name='f', n=2, imm=1)}
    assert run(old, {'a.hip': kernel('k1', reg=3) + kernel('k2') + FUNC.format(name='f', n=2, imm=1)})[0] == 1
    assert run(old, {'a.hip': kernel('k1') + kernel('k2', kernarg=16) + FUNC.format(name='f', n=2, imm=1)})[0] == 1
    # a function that two files hold must be the same in both
    assert run(old, {'a.hip': kernel('k1') + kernel('k2') + FUNC.format(name='f', n=2, imm=1),
                     'b.hip': FUNC.format(name='f', n=0, imm=2)})[0] == 1


def test_missing_kernel_is_an_error_missing_function_is_not():
    old = {'a.hip': kernel('k1') + kernel('k2', 1) + FUNC.format(name='f', n=2, imm=1)}
    bad, lines = run(old, {'a.hip': kernel('k1') + FUNC.format(name='f', n=1, imm=1)})
    assert bad == 1 and 'ONLY IN O  k2  (a.hip)' in lines
    bad, lines = run(old, {'a.hip': kernel('k1') + kernel('k2', 1)})  # f was inlined away
    assert bad == 0 and 'ONLY IN O  f  (a.hip)' in lines
    bad, lines = run(old, {'a.hip': old['a.hip'] + kernel('k3', 3)})  # a new kernel is fine
    assert bad == 0 and 'ONLY IN N  k3  (a.hip)' in lines
