"""pp_fields_from_conv_ragged_heads without a GPU: the exports and their ctypes signatures,
pp_conv_head against the header, the table arithmetic, and every argument error (all checked
before any copy or launch).  Pointers are dummies that are never dereferenced; accepted
arguments are probed with n_img = 0, which passes every check and launches nothing."""
import ctypes
import os
import re
import subprocess

import pytest

from openpifpaf_amd import _abi, _lib, constants

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
HEADER = os.path.join(REPO, 'include', 'pifpaf_amd.h')
EINVAL, ESHAPE, ENOMEM = -1, -2, -5
CIF, CAF, CIFDET = 0, 1, 2
NAME = 'pp_fields_from_conv_ragged_heads'
SIZE, OFFSET = 'pp_ragged_conv_heads_tables_size', 'pp_ragged_conv_heads_extents_offset'
FLIP = 'pp_conv_head_set_flip'
MAX_ENTRIES = 48  # 3 * PP_MAX_SCALES


@pytest.fixture(scope='module')
def lib():
    from openpifpaf_amd import build
    build.build(verbose=False)
    return _lib.load()


def test_symbols_declared_and_exported(lib):
    text = open(HEADER).read()
    assert re.search(r'#define\s+PP_ABI_VERSION\s+4\b', text)
    assert re.search(r'#define\s+PP_MAX_SCALES\s+16\b', text)
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name, ret, n_args in ((NAME, 'int', 12), (SIZE, 'size_t', 2), (OFFSET, 'size_t', 2),
                              (FLIP, 'int', 4)):
        assert re.search(r'\b' + ret + r'\s+' + name + r'\s*\(', text), name
        assert name in _lib.EXPORTED
        assert hasattr(lib, name)
        assert len(_lib._SIGNATURES[name][0]) == n_args
        decl = re.search(name + r'\s*\((.*?)\)\s*;', text, flags=re.S).group(1)
        assert len(decl.split(',')) == n_args
    assert _lib._SIGNATURES[NAME][1] is ctypes.c_int
    assert _lib._SIGNATURES[SIZE][1] is ctypes.c_size_t
    assert _lib._SIGNATURES[OFFSET][1] is ctypes.c_size_t
    assert _lib._SIGNATURES[NAME][0][10] is ctypes.c_size_t


FIELDS = ['d_container', 'layout', 'n_fields', 'H', 'W', 'out_fields', 'out_field0', 'ext_row',
          'mirror', 'has_src', 'reserved', 'swap_mask', 'src_field']


def test_conv_head_layout_matches_header(tmp_path):
    src = tmp_path / 'conv_head.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pifpaf_amd.h"\n'
                   'int main(void) {\n  printf("%zu", sizeof(pp_conv_head));\n' +
                   ''.join('  printf(" %zu", offsetof(pp_conv_head, {}));\n'.format(f)
                           for f in FIELDS) + '  return 0;\n}\n')
    exe = tmp_path / 'conv_head'
    subprocess.check_call(['gcc', '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert [name for name, _ in _abi.ConvHead._fields_] == FIELDS
    assert vals == [ctypes.sizeof(_abi.ConvHead)] + [getattr(_abi.ConvHead, f).offset
                                                     for f in FIELDS]
    d = _abi.CONV_HEAD_DTYPE
    assert vals == [d.itemsize] + [d.fields[f][1] for f in FIELDS]
    assert vals[0] == 120 and vals[0] % 8 == 0 and d.fields['src_field'][0].shape == (64,)


def test_table_layout(lib):
    size, offset = getattr(lib, SIZE), getattr(lib, OFFSET)
    for n, e in ((0, 4), (-1, 4), (-(1 << 31), 4), (3, 0), (3, -1), (3, MAX_ENTRIES + 1)):
        assert size(n, e) == 0 and offset(n, e) == 0
    for n in (1, 2, 3, 255, 65535):
        for e in (1, 2, 3, 20, MAX_ENTRIES):
            # pointers, strides, the entries, the conv extents; then the field extents
            assert offset(n, e) == n * e * (8 + 16) + 120 * e + n * e * 8
            assert offset(n, e) % 8 == 0
            assert size(n, e) == offset(n, e) + 8 * n * e


def _head(container=4096, layout=CAF, n_fields=19, H=5, W=7, out_fields=None, out_field0=0,
          ext_row=-1, mirror=0, has_src=0, swap_mask=0, src=()):
    head = _abi.ConvHead(container, layout, n_fields, H, W,
                         n_fields if out_fields is None else out_fields, out_field0, ext_row,
                         mirror, has_src, 0, swap_mask)
    for i, v in enumerate(src):
        head.src_field[i] = v
    return head


def _two(**kw):
    """A CIF and a CAF head with their own containers and extent rows; kw changes the CAF one."""
    return [_head(container=1 << 20, layout=CIF, n_fields=17, ext_row=0),
            _head(**dict(dict(container=2 << 20, ext_row=1), **kw))]


def _call(lib, heads=None, n_rows=None, extents=((3, 4), (2, 2)), strides=None, ptrs=None,
          n_img=None, dtype=0, quad=1, tables=4096, tables_bytes=None, n_entries=None,
          per_entry_extents=None):
    """Two images of 3x4 and 2x2 conv pixels (fields 5x7 and 3x3 at quad 1) per entry into 5x7
    containers, unless told otherwise."""
    heads = _two() if heads is None else heads
    e = len(heads)
    n = len(extents) if n_img is None else n_img
    m = max(len(extents), 1)
    rows = per_entry_extents if per_entry_extents is not None else [extents] * e
    arr = (_abi.ConvHead * e)(*heads)
    ptrs = (ctypes.c_void_p * (e * m))(*(ptrs if ptrs is not None else [256] * (e * m)))
    ext = (ctypes.c_int32 * (2 * e * m))(*[v for rows_e in rows for row in rows_e for v in row])
    st = None if strides is None else (ctypes.c_int64 * (2 * e * m))(
        *[v for _ in range(e) for row in strides for v in row])
    n_entries = e if n_entries is None else n_entries
    if n_rows is None:
        n_rows = sum(h.ext_row >= 0 for h in heads)
    if tables_bytes is None:
        tables_bytes = lib.pp_ragged_conv_heads_tables_size(max(n, 0), e)
    return getattr(lib, NAME)(arr, n_entries, n_rows, ptrs, ext, st, n, dtype, quad,
                              ctypes.c_void_p(tables), ctypes.c_size_t(tables_bytes), None)


def _error(lib, code, *words, **kw):
    assert _call(lib, **kw) == code
    msg = lib.pp_last_error()
    assert NAME.encode() in msg, msg
    for word in words:
        assert word in msg, msg


def test_accepted(lib):
    assert _call(lib, n_img=0) == 0
    assert _call(lib, n_img=0, extents=(), tables_bytes=0) == 0
    for dtype in (0, 1, 2):
        assert _call(lib, n_img=0, dtype=dtype, strides=((12, 4), (4, 2))) == 0
    # 48 entries, each with its own container and row
    heads = [_head(container=(m + 1) << 20, ext_row=m) for m in range(MAX_ENTRIES)]
    assert _call(lib, heads=heads, n_img=0) == 0


def test_null_arguments(lib):
    fn = getattr(lib, NAME)
    dummy = ctypes.c_void_p(4096)
    arr = (_abi.ConvHead * 1)(_head(ext_row=0))
    ptrs = (ctypes.c_void_p * 1)(256)
    ext = (ctypes.c_int32 * 2)(3, 4)
    for heads, convs, extents, tables in ((None, ptrs, ext, dummy), (arr, None, ext, dummy),
                                          (arr, ptrs, None, dummy), (arr, ptrs, ext, None)):
        assert fn(heads, 1, 1, convs, extents, None, 1, 0, 1, tables, ctypes.c_size_t(4096),
                  None) == EINVAL
        msg = lib.pp_last_error()
        assert NAME.encode() in msg and b'NULL' in msg, msg


@pytest.mark.parametrize('kw,code,word', [
    (dict(n_entries=0), ESHAPE, b'shape'),
    (dict(n_entries=-1), ESHAPE, b'shape'),
    (dict(n_entries=MAX_ENTRIES + 1), ESHAPE, b'PP_MAX_SCALES'),
    (dict(n_rows=0), ESHAPE, b'shape'),
    (dict(n_rows=3), ESHAPE, b'shape'),
    (dict(n_img=-1), ESHAPE, b'shape'),
    (dict(quad=5), ESHAPE, b'shape'),
    (dict(quad=-1), ESHAPE, b'shape'),
    (dict(dtype=3), EINVAL, b'dtype'),
    (dict(dtype=-1), EINVAL, b'dtype'),
    (dict(heads=_two(container=0)), EINVAL, b'NULL'),
    (dict(heads=_two(n_fields=0)), ESHAPE, b'shape'),
    (dict(heads=_two(H=0)), ESHAPE, b'shape'),
    (dict(heads=_two(W=-1)), ESHAPE, b'shape'),
    (dict(heads=_two(layout=CIFDET, n_fields=3)), EINVAL, b'layout'),
    (dict(heads=_two(layout=-1)), EINVAL, b'layout'),
    (dict(heads=_two(n_fields=65, has_src=1)), ESHAPE, b'64'),
    (dict(heads=_two(n_fields=65, swap_mask=1)), ESHAPE, b'64'),
    (dict(heads=_two(layout=CIF, n_fields=17, swap_mask=2)), EINVAL, b'swap_ends'),
    (dict(heads=_two(out_field0=-1)), ESHAPE, b'out_field'),
    (dict(heads=_two(out_fields=44, out_field0=26)), ESHAPE, b'out_field'),
    (dict(heads=_two(out_fields=18)), ESHAPE, b'out_field'),
    (dict(heads=_two(has_src=1, src=[0] * 18 + [19])), EINVAL, b'src_field'),
    (dict(heads=_two(has_src=1, src=[255] + [0] * 18)), EINVAL, b'src_field'),
    (dict(heads=_two(H=1 << 16, W=1 << 15)), ESHAPE, b'int32'),
    (dict(heads=_two(container=(2 << 20) + 2)), EINVAL, b'misaligned'),
    (dict(heads=_two(H=1 << 15, W=1 << 15, n_fields=1)
          + [_head(container=(m + 3) << 40, H=1 << 15, W=1 << 15, n_fields=64)
             for m in range(8)]), ESHAPE, b'workgroups'),
    # extent rows
    (dict(heads=_two(ext_row=-2)), EINVAL, b'ext_row'),
    (dict(heads=_two(ext_row=2)), EINVAL, b'ext_row'),
    (dict(heads=_two(ext_row=0), n_rows=1), EINVAL, b'two'),
    (dict(heads=_two(ext_row=0), n_rows=2), EINVAL, b'two'),
    (dict(heads=_two(ext_row=-1), n_rows=2), EINVAL, b'no entry'),
    # container ranges
    (dict(heads=_two() + [_head(container=2 << 20, out_fields=44, out_field0=19, n_fields=25)]),
     EINVAL, b'one container'),
    (dict(heads=[_head(container=1 << 20, ext_row=0, out_fields=44),
                 _head(container=1 << 20, out_fields=44, out_field0=18, n_fields=25)]),
     EINVAL, b'overlap'),
    (dict(heads=[_head(container=1 << 20, ext_row=0, out_fields=44),
                 _head(container=1 << 20, out_fields=44, out_field0=0, n_fields=25)]),
     EINVAL, b'overlap'),
    (dict(heads=[_head(container=1 << 20, ext_row=0, out_fields=44),
                 _head(container=1 << 20, out_fields=44, out_field0=19, n_fields=25, W=8)]),
     EINVAL, b'one container'),
    (dict(heads=[_head(container=1 << 20, ext_row=0, layout=CIF, n_fields=17),
                 _head(container=(1 << 20) + 64, ext_row=1)]), EINVAL, b'overlap'),
])
def test_argument_errors(lib, kw, code, word):
    _error(lib, code, word, **kw)
    # ... and before the empty batch returns
    if 'n_img' not in kw:
        _error(lib, code, word, n_img=0, **kw)


def test_shared_container(lib):
    """CAF and dense CAF side by side: one of them names the row."""
    parts = [_head(container=1 << 20, layout=CIF, n_fields=17, ext_row=0),
             _head(container=2 << 20, out_fields=44, ext_row=1),
             _head(container=2 << 20, out_fields=44, out_field0=19, n_fields=25)]
    assert _call(lib, heads=parts, n_img=0) == 0
    same = [(3, 4), (2, 2)]
    assert _call(lib, heads=parts, n_img=0, per_entry_extents=[same, same, same]) == 0
    _error(lib, ESHAPE, b'one container', b'conv extent', heads=parts,
           per_entry_extents=[same, same, [(3, 4), (2, 1)]])
    _error(lib, ESHAPE, b'one container', heads=parts,
           per_entry_extents=[same, [(3, 3), (2, 2)], same])
    # entries of different containers have their own sizes
    assert _call(lib, heads=parts, n_img=0,
                 per_entry_extents=[[(1, 1), (3, 2)], same, same]) == 0


def test_per_image_errors(lib):
    _error(lib, EINVAL, b'NULL', ptrs=[256, 256, 256, 0])
    _error(lib, EINVAL, b'misaligned', ptrs=[256, 258, 256, 256])      # float32 at 2 bytes
    assert _call(lib, ptrs=[256, 258, 256, 256], dtype=1, n_img=0) == 0  # a half is aligned to 2
    _error(lib, EINVAL, b'misaligned', ptrs=[256, 256, 257, 256], dtype=2)
    for bad in ((0, 2), (2, 0), (2, -1)):
        _error(lib, ESHAPE, b'extent', extents=((3, 4), bad))
    # fields of 5 x 7 fit H x W = 5 x 7 exactly; one row or one column less does not
    _error(lib, ESHAPE, b'extent', b'container', heads=_two(H=4))
    _error(lib, ESHAPE, b'extent', b'container', heads=_two(W=6))
    _error(lib, ESHAPE, b'extent', b'container', quad=0, extents=((6, 7), (2, 2)))
    _error(lib, ESHAPE, b'extent', b'container', quad=0, extents=((5, 8), (2, 2)))
    assert _call(lib, quad=0, extents=((5, 7), (1, 1)), n_img=0) == 0
    _error(lib, ESHAPE, b'65535', extents=((1, 1),) * 65536, quad=0)
    # strides
    assert _call(lib, strides=((12, 4), (4, 2)), n_img=0) == 0
    _error(lib, EINVAL, b'negative', strides=((-12, 4), (4, 2)))
    _error(lib, EINVAL, b'negative', strides=((12, 4), (4, -2)))
    # the row stride of an image of one row says nothing, its channel stride does
    assert _call(lib, extents=((1, 4), (2, 2)), strides=((4, -7), (4, 2)), n_img=0) == 0
    _error(lib, EINVAL, b'negative', extents=((1, 4), (1, 1)), strides=((4, -7), (-1, 0)))
    assert _call(lib, strides=((10 ** 15, 10 ** 12), (4, 2)), n_img=0) == 0


def test_table_buffer_errors(lib):
    need = lib.pp_ragged_conv_heads_tables_size(2, 2)
    _error(lib, ENOMEM, b'table', b'small', tables_bytes=need - 1)
    _error(lib, EINVAL, b'misaligned', tables=4096 + 4)
    assert _call(lib, tables=4096 + 4, tables_bytes=0, n_img=0) == 0


def test_set_flip(lib):
    from openpifpaf_amd import heads
    fn = getattr(lib, FLIP)
    flip = heads.caf_hflip(constants.COCO_KEYPOINTS, constants.COCO_PERSON_SKELETON)
    src, swap = flip.tables(19)
    head = _head()
    assert fn(ctypes.byref(head), 1, src, swap) == 0
    assert head.mirror == 1 and head.has_src == 1
    assert list(head.src_field)[:19] == list(flip.src_field) and not any(head.src_field[19:])
    assert head.swap_mask == sum(1 << f for f, s in enumerate(flip.swap_ends) if s)
    assert head.swap_mask != 0
    assert _call(lib, heads=[_head(container=1 << 20, layout=CIF, n_fields=17, ext_row=0),
                             _abi.ConvHead.from_buffer_copy(head)], n_rows=1, n_img=0) == 0
    # without tables: the mirror alone; and back to no flip at all
    assert fn(ctypes.byref(head), 1, None, None) == 0
    assert (head.mirror, head.has_src, head.swap_mask) == (1, 0, 0) and not any(head.src_field)
    assert fn(ctypes.byref(head), 0, None, None) == 0 and head.mirror == 0
    # the checks of pp_fields_from_conv_ex on the tables
    bad = (ctypes.c_int32 * 19)(*([0] * 18 + [19]))
    assert fn(ctypes.byref(head), 1, bad, None) == EINVAL
    assert b'src_field' in lib.pp_last_error()
    cif = _head(layout=CIF, n_fields=17)
    assert fn(ctypes.byref(cif), 1, None, (ctypes.c_uint8 * 17)()) == EINVAL
    assert b'swap_ends' in lib.pp_last_error()
    wide = _head(n_fields=65)
    assert fn(ctypes.byref(wide), 1, (ctypes.c_int32 * 65)(), None) == ESHAPE
    assert fn(ctypes.byref(wide), 1, None, None) == 0  # the limit is the tables'
    assert fn(None, 1, None, None) == EINVAL
    assert fn(ctypes.byref(_head(n_fields=0)), 1, None, None) == ESHAPE
