"""pp_fields_from_conv_strided without a GPU: the export, its argument errors (all checked
before any launch) and which stride patterns it accepts.  Accepted patterns are probed with
n_img = 0, which passes every check and launches nothing."""
import ctypes
import os
import re

import pytest

from openpifpaf_amd import _lib, constants

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
EINVAL, ESHAPE = -1, -2
CIF, CAF, CIFDET = 0, 1, 2
NAME = 'pp_fields_from_conv_strided'


@pytest.fixture(scope='module')
def lib():
    from openpifpaf_amd import build
    build.build(verbose=False)
    return _lib.load()


def test_symbol_declared_and_exported(lib):
    text = open(os.path.join(REPO, 'include', 'pifpaf_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'\bint\s+' + NAME + r'\s*\(', text)
    assert NAME in _lib.EXPORTED
    assert hasattr(lib, NAME)
    assert len(_lib._SIGNATURES[NAME][0]) == 16


def nchw(ch, h, w):
    return [ch * h * w, h * w, w, 1]


def nhwc(ch, h, w):
    return [h * w * ch, 1, w * ch, ch]


def _call(lib, strides='nchw', dtype=0, n_img=1, n_fields=19, layout=CAF, h=3, w=4, quad=1,
          src=None, swap=None, out_fields=None, out_field0=0, mirror=0):
    """Dummy pointers: never dereferenced, every call ends before a launch."""
    dummy = ctypes.c_void_p(256)
    ch = n_fields * (5, 9, 7)[layout if 0 <= layout <= 2 else 0] * 4 ** quad
    if isinstance(strides, str):
        strides = {'nchw': nchw, 'nhwc': nhwc}[strides](ch, h, w)
    strides = (ctypes.c_int64 * 4)(*strides)
    src = None if src is None else (ctypes.c_int32 * len(src))(*src)
    swap = None if swap is None else (ctypes.c_uint8 * len(swap))(*swap)
    return getattr(lib, NAME)(
        dummy, dtype, strides, n_img, n_fields, layout, h, w, quad, mirror, src, swap, dummy,
        n_fields if out_fields is None else out_fields, out_field0, None)


@pytest.mark.parametrize('dim', [0, 1, 2, 3])
@pytest.mark.parametrize('base', ['nchw', 'nhwc'])
def test_negative_stride(lib, base, dim):
    strides = {'nchw': nchw, 'nhwc': nhwc}[base](19 * 9 * 4, 3, 4)
    strides[dim] = -strides[dim]
    assert _call(lib, strides, n_img=2) == EINVAL
    msg = lib.pp_last_error()
    assert NAME.encode() in msg and b'negative' in msg, msg


def test_neither_class(lib):
    """Steps along both the channels and the columns."""
    ch = 19 * 9 * 4
    assert _call(lib, [ch * 3 * 8 * 2, 2, 2 * ch * 8, 2]) == EINVAL
    msg = lib.pp_last_error()
    assert NAME.encode() in msg and b'channel' in msg and b'column' in msg, msg
    # also with n_img = 0: the class is decided before the empty batch returns
    assert _call(lib, [ch * 3 * 8 * 2, 2, 2 * ch * 8, 2], n_img=0) == EINVAL


# the error cases of tests/test_ingest_ex_abi.py, through the new symbol and both classes
@pytest.mark.parametrize('strides', ['nchw', 'nhwc'])
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
    (dict(h=0), ESHAPE, b'shape'),
    (dict(quad=5), ESHAPE, b'shape'),
    (dict(n_img=-1), ESHAPE, b'shape'),
])
def test_ex_argument_errors(lib, strides, kw, code, word):
    assert _call(lib, strides, **kw) == code
    msg = lib.pp_last_error()
    assert NAME.encode() in msg and word in msg, msg


def test_null_pointers(lib):
    dummy = ctypes.c_void_p(256)
    strides = (ctypes.c_int64 * 4)(*nchw(340, 3, 4))
    fn = getattr(lib, NAME)
    for conv, st, out in ((None, strides, dummy), (dummy, None, dummy), (dummy, strides, None)):
        assert fn(conv, 0, st, 1, 17, CIF, 3, 4, 1, 0, None, None, out, 17, 0, None) == EINVAL
        assert b'NULL' in lib.pp_last_error()


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_accepted_strides_and_empty_batch(lib, dtype):
    """n_img = 0 returns 0 for dense NCHW, dense channels-last and their slices, with the
    hflip tables and an output field range as pp_fields_from_conv_ex takes them."""
    from openpifpaf_amd import heads
    flip = heads.caf_hflip(constants.COCO_KEYPOINTS, constants.COCO_PERSON_SKELETON)
    ch = 19 * 9 * 4
    for strides in ('nchw', 'nhwc',
                    nchw(ch + 341, 5, 7),    # channel slice and spatial crop of NCHW
                    nhwc(ch + 341, 5, 7),    # the same of channels-last
                    [0, 12, 4, 1],           # an expanded (broadcast) batch
                    [7, 1, 10 ** 12, 10 ** 10]):  # 64-bit strides
        assert _call(lib, strides, dtype=dtype, n_img=0, src=flip.src_field,
                     swap=flip.swap_ends, mirror=1, out_fields=44, out_field0=25) == 0


def test_extent_one_strides_are_ignored(lib):
    """h = w = 1: the row and column strides say nothing, whatever they hold; the image
    stride of a single image likewise."""
    for dtype in (0, 1, 2):
        assert _call(lib, [5, 1, -3, 77], dtype=dtype, n_img=0, h=1, w=1) == 0
        assert _call(lib, [5, 40, 10 ** 15, -1], dtype=dtype, n_img=0, h=1, w=1) == 0
    # one column: a channel stride of 2 is fine (planar), the column stride is not read
    assert _call(lib, [9999, 2, 1, 2], n_img=0, h=3, w=1) == 0
    # one image: a negative image stride is not read, but n_img = 2 reads it
    ch = 19 * 9 * 4
    assert _call(lib, [-1] + nchw(ch, 3, 4)[1:], n_img=0) == 0
    assert _call(lib, [-1] + nchw(ch, 3, 4)[1:], n_img=2) == EINVAL
