"""pp_fields_from_conv_ragged without a GPU: the three exports, every argument error (all
checked before any copy or launch) and the table layout.  Pointers are dummies that are never
dereferenced; accepted arguments are probed with n_img = 0, which passes every check and
launches nothing."""
import ctypes
import os
import re

import pytest

from openpifpaf_amd import _lib, constants

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
EINVAL, ESHAPE, ENOMEM = -1, -2, -5
CIF, CAF, CIFDET = 0, 1, 2
NAME = 'pp_fields_from_conv_ragged'
SIZE, OFFSET = 'pp_ragged_conv_tables_size', 'pp_ragged_conv_extents_offset'


@pytest.fixture(scope='module')
def lib():
    from openpifpaf_amd import build
    build.build(verbose=False)
    return _lib.load()


def test_symbols_declared_and_exported(lib):
    text = open(os.path.join(REPO, 'include', 'pifpaf_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name, ret, n_args in ((NAME, 'int', 19), (SIZE, 'size_t', 1), (OFFSET, 'size_t', 1)):
        assert re.search(r'\b' + ret + r'\s+' + name + r'\s*\(', text), name
        assert name in _lib.EXPORTED
        assert hasattr(lib, name)
        assert len(_lib._SIGNATURES[name][0]) == n_args
    decl = re.search(NAME + r'\s*\((.*?)\)\s*;', text, flags=re.S).group(1)
    assert len(decl.split(',')) == 19


def _call(lib, dtype=0, n_fields=19, layout=CAF, quad=1, src=None, swap=None, out_fields=None,
          out_field0=0, mirror=0, extents=((3, 4), (2, 2)), strides=None, ptrs=None, n_img=None,
          H=5, W=7, container=256, tables=4096, tables_bytes=None):
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
    return getattr(lib, NAME)(
        ptrs, dtype, ext, st, n, n_fields, layout, quad, mirror, src, swap, H, W,
        ctypes.c_void_p(container), n_fields if out_fields is None else out_fields, out_field0,
        ctypes.c_void_p(tables), ctypes.c_size_t(tables_bytes), None)


def _error(lib, code, *words, **kw):
    assert _call(lib, **kw) == code
    msg = lib.pp_last_error()
    assert NAME.encode() in msg, msg
    for word in words:
        assert word in msg, msg


# the error cases of tests/test_ingest_ex_abi.py, through the new symbol
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
    (dict(quad=5), ESHAPE, b'shape'),
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
    assert _call(lib, ptrs=[256, 258], dtype=1, n_img=0) == 0     # a half is aligned to 2
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


def test_table_buffer_errors(lib):
    need = lib.pp_ragged_conv_tables_size(2)
    _error(lib, ENOMEM, b'table', b'small', tables_bytes=need - 1)
    _error(lib, EINVAL, b'misaligned', tables=4096 + 4)
    _error(lib, EINVAL, b'misaligned', container=256 + 2)
    # the container needs 4-byte alignment only; what passes these checks would launch, so
    # the accepted side is probed with the empty batch
    assert _call(lib, container=256 + 4, tables=4096 + 4, tables_bytes=0, n_img=0) == 0


def test_negative_strides(lib):
    dense = ((12, 4), (4, 2))
    assert _call(lib, strides=dense, n_img=0) == 0
    _error(lib, EINVAL, b'negative', strides=((-12, 4), (4, 2)))
    _error(lib, EINVAL, b'negative', strides=((12, 4), (-4, 2)))
    _error(lib, EINVAL, b'negative', strides=((12, -4), (4, 2)))
    _error(lib, EINVAL, b'negative', strides=((12, 4), (4, -2)))
    # the row stride of an image of one row says nothing
    assert _call(lib, extents=((1, 4), (2, 2)), strides=((4, -7), (4, 2)), n_img=0) == 0
    assert _call(lib, extents=((1, 4), (1, 1)), strides=((4, -7), (1, -1 << 40)), n_img=0) == 0
    # ... but its channel stride does
    _error(lib, EINVAL, b'negative', extents=((1, 4), (1, 1)), strides=((4, -7), (-1, 0)))
    # 64-bit strides are taken
    assert _call(lib, strides=((10 ** 15, 10 ** 12), (4, 2)), n_img=0) == 0


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_empty_batch(lib, dtype):
    """n_img = 0 returns 0 with the hflip tables and an output field range, with and without
    strides, whatever the table buffer."""
    from openpifpaf_amd import heads
    flip = heads.caf_hflip(constants.COCO_KEYPOINTS, constants.COCO_PERSON_SKELETON)
    for strides in (None, ((12, 4), (4, 2))):
        assert _call(lib, dtype=dtype, n_img=0, src=flip.src_field, swap=flip.swap_ends,
                     mirror=1, out_fields=44, out_field0=25, strides=strides) == 0
    assert _call(lib, dtype=dtype, n_img=0, extents=(), tables_bytes=0) == 0
    # 65 fields without tables are fine (the limit is the tables')
    assert _call(lib, dtype=dtype, n_img=0, n_fields=65, layout=CIFDET, mirror=1) == 0


def test_table_layout(lib):
    size, offset = getattr(lib, SIZE), getattr(lib, OFFSET)
    for n in (0, -1, -(1 << 31)):
        assert size(n) == 0 and offset(n) == 0
    for n in (1, 2, 3, 255, 256, 65535):
        assert offset(n) % 8 == 0
        assert size(n) == offset(n) + 8 * n
        # in front of the field extents: a pointer, two strides and the conv extents per image
        assert offset(n) >= n * (8 + 16 + 8)
