"""Does a refactor change the generated gfx950 code?  Compares two source trees by symbol:
    python tools/isa_diff.py PARENT_TREE NEW_TREE [variant]
Each tree is a repository root (a `git archive` of the parent commit, and the working tree).
Every csrc/*.hip of each is compiled to device assembly with the flags of that tree's own
openpifpaf_amd/build.py (its per-file flags and its variant's defines, e.g. `stamps`: code
that moved to another file is built as each tree's build would build it); the assembly is
split by function symbol, comments go, the numbers in local labels are replaced, and each
symbol is compared ACROSS the files of a tree (code may have moved to another file).  hipcc emits a kernel's .amdhsa_kernel block
(registers, LDS, scratch) inside the function's .type ... .size range, so it is compared with
the code, and it marks the symbol as a kernel.  Needs no GPU.  Exits 1 on any DIFF or on a
kernel missing from NEW_TREE."""
import concurrent.futures
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

LABEL = re.compile(r'(\.L[A-Za-z_]+?)\d+')


def tree_build(tree):
    """The tree's own openpifpaf_amd/build.py as a module, loaded by path: each tree is
    compiled with the flags its own build gives it (CFLAGS with its include directory,
    FILE_FLAGS by file name, VARIANTS)."""
    path = os.path.join(tree, 'openpifpaf_amd', 'build.py')
    spec = importlib.util.spec_from_file_location('isa_diff_tree_build', path)  # not registered
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def command(b, name, variant, out):
    """The hipcc line for the device assembly of csrc/`name` under the tree's build module b"""
    return ([b.HIPCC] + b.CFLAGS + b.FILE_FLAGS.get(name, []) + b.VARIANTS.get(variant, []) +
            ['--cuda-device-only', '-S', os.path.join(b.CSRC, name), '-o', out])


def assembly(tree, variant, tmp):
    """{file name: device assembly text} of the tree's csrc/*.hip"""
    b = tree_build(tree)

    def one(name):
        out = os.path.join(tmp, name[:-4] + '.s')
        cmd = command(b, name, variant, out)
        res = subprocess.run(cmd, capture_output=True, text=True, check=False)
        if res.returncode != 0:
            raise RuntimeError('hipcc failed: {}\n{}'.format(' '.join(cmd), res.stderr))
        with open(out) as f:
            return name, f.read()

    names = sorted(f for f in os.listdir(b.CSRC) if f.endswith('.hip'))
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        return dict(ex.map(one, names))


def symbols(asm):
    """({symbol: [(file, normalised text), ...]}, the set of kernel symbols) of
    {file name: assembly text}"""
    syms, kernels = {}, set()
    for name, text in asm.items():
        cur, body = None, []
        for line in text.splitlines():
            line = line.split(';', 1)[0].rstrip()
            if not line.strip():
                continue
            line = LABEL.sub(r'\1N', line)
            tok = line.split()
            if tok[0] == '.amdhsa_kernel':
                kernels.add(tok[1])
            if cur is None:
                if tok[0] == '.type' and tok[1].endswith(',@function'):
                    cur, body = tok[1][:-len(',@function')], []
            elif tok[0] == '.size':
                syms.setdefault(cur, []).append((name, '\n'.join(body)))
                cur = None
            else:
                body.append(line)
    return syms, kernels


def compare(old, new, old_name='OLD', new_name='NEW', out=print):
    """Report every symbol of two symbols() results; the number of DIFFs and of kernels
    missing from `new`"""
    (old, old_kernels), (new, _) = old, new
    bad = 0
    for sym in sorted(set(old) | set(new)):
        where = ','.join(sorted({f for f, _ in new.get(sym, old.get(sym))}))
        if sym not in new or sym not in old:
            out('ONLY IN {}  {}  ({})'.format(old_name if sym in old else new_name, sym, where))
            bad += sym in old_kernels and sym not in new
            continue
        a, c = {t for _, t in old[sym]}, {t for _, t in new[sym]}
        if a == c:
            out('SAME  {}  ({})'.format(sym, where))
            continue
        bad += 1
        out('DIFF  {}  ({})'.format(sym, where))
        x, y = sorted(a - c or a)[0].splitlines(), sorted(c - a or c)[0].splitlines()
        shown = 0
        for i in range(max(len(x), len(y))):
            lx, ly = (x[i] if i < len(x) else '<end>'), (y[i] if i < len(y) else '<end>')
            if lx != ly and shown < 6:
                out('    line {}:\n      - {}\n      + {}'.format(i + 1, lx.strip(), ly.strip()))
                shown += 1
        out('    ({} -> {} lines)'.format(len(x), len(y)))
    return bad


def main():
    old_tree, new_tree = sys.argv[1], sys.argv[2]
    variant = sys.argv[3] if len(sys.argv) > 3 else ''
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new:
        old = symbols(assembly(old_tree, variant, t_old))
        new = symbols(assembly(new_tree, variant, t_new))
    sys.exit(1 if compare(old, new, old_tree, new_tree) else 0)


if __name__ == '__main__':
    main()
