"""pp_fields_from_conv_ragged_interleaved without a GPU: the export, every argument error (all
checked before any copy or launch, with the codes and the order of
pp_fields_from_conv_ragged) and the table layout it shares with that symbol.  Pointers are
dummies that are never dereferenced; accepted arguments are probed with n_img = 0, which
passes every check and launches nothing."""
import ctypes
import os
import re

import pytest

from openpifpaf_amd import _lib, constants

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
EINVAL, ESHAPE, ENOMEM = -1, -2, -5
CIF, CAF, CIFDET = 0, 1, 2
NAME = 'pp_fields_from_conv_ragged_interleaved'
PLANAR = 'pp_fields_from_conv_ragged'


@pytest.fixture(scope='module')
def lib():
    from openpifpaf_amd import build
    build.build(verbose=False)
    return _lib.load()


def test_symbol_declared_and_exported(lib):
    text = open(os.path.join(REPO, 'include', 'pifpaf_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'\bint\s+' + NAME + r'\s*\(', text)
    assert NAME in _lib.EXPORTED and hasattr(lib, NAME)
    # the arguments of the planar symbol, one for one
    assert _lib._SIGNATURES[NAME] == _lib._SIGNATURES[PLANAR]
    decl = {n: re.search(r'\b' + n + r'\s*\((.*?)\)\s*;', text, flags=re.S).group(1)
            for n in (NAME, PLANAR)}
    assert len(decl[NAME].split(',')) == 19
    assert re.sub(r'\s+', ' ', decl[NAME]).strip() == re.sub(r'\s+', ' ', decl[PLANAR]).strip()
    # a symbol was added and none changed
    assert lib.pp_version() == 4
    assert re.search(r'#define\s+PP_ABI_VERSION\s+4\b', text)


def _call(lib, dtype=0, n_fields=19, layout=CAF, quad=1, src=None, swap=None, out_fields=None,
          out_field0=0, mirror=0, extents=((3, 4), (2, 2)), strides=None, ptrs=None, n_img=None,
          H=5, W=7, container=256, tables=4096, tables_bytes=None, name=NAME):
    """Two images of 3x4 and 2x2 conv pixels (fields 5x7 and 3x3 at quad 1) into a 5x7
    container, unless told otherwise."""
    n = len(extents) if n_img is None else n_img
    m = max(len(extents), 1)
    ptrs = (ctypes.c_void_p * m)(*(ptrs if ptrs is not None else [256] * m))
    ext = (ctypes.c_int32 * (2 * m))(*[v for row in extents for v in row])
    st = None if strides is None else (ctypes.c_int64 * (2 * m))(*[v for row in strides
                                                                    for v in row])
    src = None if src is None else (ctypes.c_int32 * len(src))(*src)
    swap = None if swap is None else (ctypes.c_uint8 * len(swap))(*swap)
    if tables_bytes is None:
        tables_bytes = lib.pp_ragged_conv_tables_size(max(n, 0))
    return getattr(lib, name)(
        ptrs, dtype, ext, st, n, n_fields, layout, quad, mirror, src, swap, H, W,
        ctypes.c_void_p(container), n_fields if out_fields is None else out_fields, out_field0,
        ctypes.c_void_p(tables), ctypes.c_size_t(tables_bytes), None)


def _error(lib, code, *words, planar=True, **kw):
    assert _call(lib, **kw) == code
    msg = lib.pp_last_error()
    assert NAME.encode() in msg, msg
    for word in words:
        assert word in msg, msg
    # the planar symbol answers the same arguments with the same code (its stride table has
    # another meaning)
    if planar and 'strides' not in kw:
        assert _call(lib, name=PLANAR, **kw) == code


@pytest.mark.parametrize('kw,code,word', [
    (dict(dtype=3), EINVAL, b'dtype'),
    (dict(dtype=-1), EINVAL, b'dtype'),
    (dict(layout=3), EINVAL, b'layout'),
    (dict(src=[0] * 18 + [19]), EINVAL, b'src_field'),
    (dict(src=[-1] + [0] * 18), EINVAL, b'src_field'),
    (dict(layout=CIF, n_fields=17, swap=[0] * 17), EINVAL, b'swap_ends'),
    (dict(layout=CIFDET, n_fields=3, swap=[1, 0, 0]), EINVAL, b'swap_ends'),
    (dict(n_fields=65, src=list(range(65))), ESHAPE, b'64'),
    (dict(n_fields=65, swap=[0] * 65), ESHAPE, b'64'),
    (dict(out_field0=-1), ESHAPE, b'out_field'),
    (dict(out_fields=44, out_field0=26), ESHAPE, b'out_field'),
    (dict(out_fields=18), ESHAPE, b'out_field'),
    (dict(H=0), ESHAPE, b'shape'),
    (dict(W=0), ESHAPE, b'shape'),
    (dict(quad=5), ESHAPE, b'shape'),
    (dict(quad=-1), ESHAPE, b'shape'),
    (dict(n_img=-1), ESHAPE, b'shape'),
    (dict(n_fields=0), ESHAPE, b'shape'),
])
def test_ex_argument_errors(lib, kw, code, word):
    _error(lib, code, word, **kw)
    # ... and before the empty batch returns
    if 'n_img' not in kw:
        _error(lib, code, word, n_img=0, **kw)


def test_null_arguments(lib):
    fn = getattr(lib, NAME)
    dummy = ctypes.c_void_p(256)
    ptrs = (ctypes.c_void_p * 1)(256)
    ext = (ctypes.c_int32 * 2)(3, 4)
    for convs, extents, out, tables in ((None, ext, dummy, dummy), (ptrs, None, dummy, dummy),
                                        (ptrs, ext, None, dummy), (ptrs, ext, dummy, None)):
        assert fn(convs, 0, extents, None, 1, 17, CIF, 1, 0, None, None, 5, 7, out, 17, 0,
                  tables, ctypes.c_size_t(4096), None) == EINVAL
        msg = lib.pp_last_error()
        assert NAME.encode() in msg and b'NULL' in msg, msg


def test_ragged_errors(lib):
    _error(lib, EINVAL, b'NULL', ptrs=[256, 0])
    _error(lib, EINVAL, b'misaligned', ptrs=[256, 258])           # float32 at 2 bytes
    # a half is aligned to 2 bytes, no more: channel slices start at any element
    assert _call(lib, ptrs=[256, 258], dtype=1, n_img=0) == 0
    assert _call(lib, ptrs=[256 + 6, 256 + 14], dtype=2, n_img=0) == 0
    assert _call(lib, ptrs=[256 + 4, 256 + 12], dtype=0, n_img=0) == 0
    _error(lib, EINVAL, b'misaligned', ptrs=[256, 257], dtype=2)
    _error(lib, ESHAPE, b'extent', extents=((3, 4), (0, 2)))
    _error(lib, ESHAPE, b'extent', extents=((3, 4), (2, 0)))
    _error(lib, ESHAPE, b'extent', extents=((3, 4), (2, -1)))
    # fields of 5 x 7 fit H x W = 5 x 7 exactly; one row or one column less does not
    _error(lib, ESHAPE, b'extent', b'container', H=4)
    _error(lib, ESHAPE, b'extent', b'container', W=6)
    _error(lib, ESHAPE, b'extent', b'container', quad=0, extents=((6, 7), (2, 2)))
    _error(lib, ESHAPE, b'extent', b'container', quad=0, extents=((5, 8), (2, 2)))
    assert _call(lib, quad=0, extents=((5, 7), (1, 1)), n_img=0) == 0
    _error(lib, ESHAPE, b'int32', H=1 << 16, W=1 << 15)
    _error(lib, ESHAPE, b'65535', extents=((1, 1),) * 65536, quad=0)
    # the order of the planar symbol: the int32 limit before the grid limit, the grid limit
    # before the per-image checks
    _error(lib, ESHAPE, b'int32', H=1 << 16, W=1 << 15, extents=((1, 1),) * 65536, quad=0)
    _error(lib, ESHAPE, b'65535', extents=((1, 1),) * 65535 + ((0, 0),), quad=0)


def test_chunk_grid_limit(lib):
    """At quad 4 a chunk holds 2 pre-dequad channels, so 65535 chunks are 131070 of them:
    CifDet with 18724 categories (131068) is inside, 18725 (131075) is not.  The limit is
    checked after the field-range and before the per-image checks."""
    assert _call(lib, layout=CIFDET, n_fields=18724, quad=4, H=33, W=33, n_img=0) == 0
    _error(lib, ESHAPE, b'chunk', planar=False, layout=CIFDET, n_fields=18725, quad=4, H=33,
           W=33)
    assert _call(lib, name=PLANAR, layout=CIFDET, n_fields=18725, quad=4, H=33, W=33,
                 n_img=0) == 0
    _error(lib, ESHAPE, b'chunk', planar=False, layout=CIFDET, n_fields=18725, quad=4, H=33,
           W=33, ptrs=[256, 0])


def test_table_buffer_errors(lib):
    need = lib.pp_ragged_conv_tables_size(2)
    _error(lib, ENOMEM, b'table', b'small', tables_bytes=need - 1)
    _error(lib, EINVAL, b'misaligned', tables=4096 + 4)
    _error(lib, EINVAL, b'misaligned', container=256 + 2)
    # the per-image checks come before the table checks
    _error(lib, EINVAL, b'NULL', ptrs=[256, 0], tables_bytes=need - 1)
    # the container needs 4-byte alignment only; what passes these checks would launch, so
    # the accepted side is probed with the empty batch
    assert _call(lib, container=256 + 4, tables=4096 + 4, tables_bytes=0, n_img=0) == 0


def test_negative_strides(lib):
    """conv_strides rows are (row, column) strides; the channel stride is 1 by definition."""
    dense = ((4 * 684, 684), (2 * 684, 684))
    assert _call(lib, strides=dense, n_img=0) == 0
    _error(lib, EINVAL, b'negative', strides=((-2736, 684), (1368, 684)))
    _error(lib, EINVAL, b'negative', strides=((2736, 684), (-1368, 684)))
    _error(lib, EINVAL, b'negative', strides=((2736, -684), (1368, 684)))
    _error(lib, EINVAL, b'negative', strides=((2736, 684), (1368, -684)))
    # the row stride of an image of one row says nothing, nor the column stride of one column
    assert _call(lib, extents=((1, 4), (2, 2)), strides=((-7, 684), (1368, 684)), n_img=0) == 0
    assert _call(lib, extents=((3, 1), (2, 2)), strides=((684, -7), (1368, 684)), n_img=0) == 0
    assert _call(lib, extents=((1, 4), (1, 1)), strides=((-7, 684), (-1 << 40, -1)),
                 n_img=0) == 0
    # ... but the other one of such an image does
    _error(lib, EINVAL, b'negative', extents=((1, 4), (2, 2)), strides=((-7, -684), (1368, 684)))
    _error(lib, EINVAL, b'negative', extents=((3, 1), (2, 2)), strides=((-684, -7), (1368, 684)))
    # 64-bit strides are taken, and strides that overlap or are 0 (an expanded view)
    assert _call(lib, strides=((10 ** 15, 10 ** 12), (0, 0)), n_img=0) == 0


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_empty_batch(lib, dtype):
    """n_img = 0 returns 0 with the hflip tables and an output field range, with and without
    strides, whatever the table buffer."""
    from openpifpaf_amd import heads
    flip = heads.caf_hflip(constants.COCO_KEYPOINTS, constants.COCO_PERSON_SKELETON)
    for strides in (None, ((2736, 684), (1368, 684))):
        assert _call(lib, dtype=dtype, n_img=0, src=flip.src_field, swap=flip.swap_ends,
                     mirror=1, out_fields=44, out_field0=25, strides=strides) == 0
    assert _call(lib, dtype=dtype, n_img=0, extents=(), tables_bytes=0) == 0
    # 65 fields without tables are fine (the limit is the tables')
    assert _call(lib, dtype=dtype, n_img=0, n_fields=65, layout=CIFDET, mirror=1) == 0
    for quad in (0, 1, 2, 3, 4):
        side = 2 ** quad * 2 + 1
        assert _call(lib, dtype=dtype, n_img=0, quad=quad, H=side, W=side,
                     extents=((3, 3), (1, 1))) == 0


def test_table_layout_is_the_planar_symbols(lib):
    """The staged layout has the planar symbol's size: an 8-byte pointer, two 8-byte strides,
    the conv extents and the field extents per image; the same two functions size it."""
    size, offset = lib.pp_ragged_conv_tables_size, lib.pp_ragged_conv_extents_offset
    for n in (1, 2, 3, 255, 256, 65535):
        assert offset(n) == n * (8 + 16 + 8) and size(n) == offset(n) + 8 * n
    need = size(2)
    assert _call(lib, tables_bytes=need, n_img=0) == 0
    assert _call(lib, tables_bytes=need - 1) == ENOMEM
    assert _call(lib, name=PLANAR, tables_bytes=need - 1) == ENOMEM
