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


FAKE_BUILD = '''import os
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(HERE, 'csrc')
HIPCC = 'hipcc'
CFLAGS = ['-O3', '-I', os.path.join(REPO, 'include')]
FILE_FLAGS = {file_flags!r}
VARIANTS = {variants!r}
'''


def test_each_tree_is_compiled_with_its_own_builds_flags(tmp_path):
    """Code that left a.hip for b.hip: the old tree flags a.hip, the new one both, and each
    tree's command lines carry its own build.py's per-file flags, variant defines and paths."""
    trees = {}
    for tree, file_flags, variants in (('old', {'a.hip': ['-fno-x']}, {'stamps': ['-DOLD_STAMPS']}),
                                       ('new', {'a.hip': ['-fno-x'], 'b.hip': ['-fno-x']},
                                        {'stamps': ['-DNEW_STAMPS']})):
        pkg = tmp_path / tree / 'openpifpaf_amd'
        (pkg / 'csrc').mkdir(parents=True)
        (pkg / 'build.py').write_text(FAKE_BUILD.format(file_flags=file_flags, variants=variants))
        trees[tree] = isa_diff.tree_build(str(tmp_path / tree))
    old, new = trees['old'], trees['new']
    assert old is not new and old.FILE_FLAGS != new.FILE_FLAGS
    for name, old_has, new_has in (('a.hip', True, True), ('b.hip', False, True), ('c.hip', False, False)):
        co = isa_diff.command(old, name, '', 'o.s')
        cn = isa_diff.command(new, name, '', 'n.s')
        assert ('-fno-x' in co, '-fno-x' in cn) == (old_has, new_has)
        # each tree's own source and include directory
        assert str(tmp_path / 'old' / 'openpifpaf_amd' / 'csrc' / name) in co
        assert str(tmp_path / 'new' / 'openpifpaf_amd' / 'csrc' / name) in cn
        assert str(tmp_path / 'old' / 'include') in co and str(tmp_path / 'new' / 'include') in cn
        assert str(tmp_path / 'new') not in ' '.join(co) and str(tmp_path / 'old') not in ' '.join(cn)
    so, sn = isa_diff.command(old, 'b.hip', 'stamps', 'o.s'), isa_diff.command(new, 'b.hip', 'stamps', 'n.s')
    assert '-DOLD_STAMPS' in so and '-DNEW_STAMPS' not in so
    assert '-DNEW_STAMPS' in sn and '-DOLD_STAMPS' not in sn and '-fno-x' in sn and '-fno-x' not in so


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
