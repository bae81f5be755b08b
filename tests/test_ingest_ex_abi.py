"""pp_fields_from_conv_ex without a GPU: the export, its argument errors (all checked before
any launch), the hflip tables against the reference's, and the reference fixture against
the closed form the GPU tests compose with."""
import ctypes
import os
import re

import numpy as np
import pytest

import golden_util as gu
import hflip_util as hu
import oracle
from openpifpaf_amd import _lib, constants

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
EINVAL, ESHAPE = -1, -2
CIF, CAF, CIFDET = 0, 1, 2


@pytest.fixture(scope='module')
def lib():
    from openpifpaf_amd import build
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(gu.GOLDEN, 'heads_hflip.npz'))


def test_symbol_declared_and_exported(lib):
    text = open(os.path.join(REPO, 'include', 'pifpaf_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'\bint\s+pp_fields_from_conv_ex\s*\(', text)
    assert 'pp_fields_from_conv_ex' in _lib.EXPORTED
    assert hasattr(lib, 'pp_fields_from_conv_ex')
    assert len(_lib._SIGNATURES['pp_fields_from_conv_ex'][0]) == 15


def _call(lib, dtype=0, n_fields=19, layout=CAF, src=None, swap=None, out_fields=None,
          out_field0=0, mirror=0):
    dummy = ctypes.c_void_p(256)  # never dereferenced: every case fails before the launch
    src = None if src is None else (ctypes.c_int32 * len(src))(*src)
    swap = None if swap is None else (ctypes.c_uint8 * len(swap))(*swap)
    return lib.pp_fields_from_conv_ex(
        dummy, dtype, 1, n_fields, layout, 3, 4, 1, mirror, src, swap, dummy,
        n_fields if out_fields is None else out_fields, out_field0, None)


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
])
def test_argument_errors(lib, kw, code, word):
    assert _call(lib, **kw) == code
    msg = lib.pp_last_error()
    assert b'pp_fields_from_conv_ex' in msg and word in msg, msg


def test_null_pointers(lib):
    dummy = ctypes.c_void_p(256)
    assert lib.pp_fields_from_conv_ex(None, 0, 1, 17, CIF, 3, 4, 1, 0, None, None, dummy,
                                      17, 0, None) == EINVAL
    assert b'NULL' in lib.pp_last_error()
    assert lib.pp_fields_from_conv_ex(dummy, 0, 1, 17, CIF, 3, 4, 1, 0, None, None, None,
                                      17, 0, None) == EINVAL


def test_empty_batch_is_ok_without_gpu(lib):
    """n_img = 0 launches nothing: valid tables pass every check."""
    from openpifpaf_amd import heads
    flip = heads.caf_hflip(constants.COCO_KEYPOINTS, constants.COCO_PERSON_SKELETON)
    src, swap = flip.tables(19)
    dummy = ctypes.c_void_p(256)
    for dtype in (0, 1, 2):
        assert lib.pp_fields_from_conv_ex(dummy, dtype, 0, 19, CAF, 3, 4, 1, 1, src, swap,
                                          dummy, 44, 25, None) == 0
    # 65 fields without tables are fine (the limit is the tables')
    assert lib.pp_fields_from_conv_ex(dummy, 0, 0, 65, CIFDET, 3, 4, 1, 1, None, None, dummy,
                                      65, 0, None) == 0


def test_hflip_tables_equal_the_reference_modules(golden):
    from openpifpaf_amd import heads
    cif = heads.cif_hflip(constants.COCO_KEYPOINTS)
    assert cif.swap_ends is None
    assert list(cif.src_field) == golden['cif_flip_indices'].tolist()
    caf = heads.caf_hflip(constants.COCO_KEYPOINTS, constants.COCO_PERSON_SKELETON)
    assert list(caf.src_field) == golden['caf_flip_indices'].tolist()
    swapped = [i for i, s in enumerate(caf.swap_ends) if s]
    assert swapped == golden['caf_reverse_direction'].tolist()
    assert [constants.COCO_PERSON_SKELETON[i] for i in swapped] == [(12, 13), (6, 7), (2, 3)]
    with pytest.raises(ValueError):
        caf.tables(17)


def test_hflip_tables_last_match_wins():
    """PafHFlip's loop order (heads.py:186-191): a reversed match overrides a direct one,
    and each match is the first index of the mirrored skeleton."""
    from openpifpaf_amd import heads
    kps = ['a', 'left_b', 'right_b']
    flip = {'left_b': 'right_b', 'right_b': 'left_b'}
    # edge 0 (left_b, right_b) mirrors to (right_b, left_b) = itself reversed; edge 1 is
    # already that reversed edge, so both match directly AND reversed
    t = heads.caf_hflip(kps, [(2, 3), (3, 2), (1, 2), (1, 3)], flip)
    assert t.src_field == (0, 1, 3, 2) and t.swap_ends == (1, 1, 0, 0)
    # no mirrored partner in the skeleton: the field stays, nothing swaps
    t = heads.caf_hflip(kps, [(1, 2)], flip)
    assert t.src_field == (0,) and t.swap_ends == (0,)
    assert heads.cif_hflip(kps, flip).src_field == (0, 2, 1)


@pytest.mark.parametrize('quad', [0, 1, 2])
@pytest.mark.parametrize('kind,n_fields', [('cif', 17), ('caf', 19)])
def test_reference_fixture_equals_closed_form(golden, kind, n_fields, quad):
    """The reference's modules (fixture) against permute / mirror / negate-x / swap on the
    conv followed by the pinned oracle ingest: bit for bit."""
    conv = golden['q%d_%s_conv' % (quad, kind)].astype(np.float32)
    src = golden['%s_flip_indices' % kind].tolist()
    swap = None
    if kind == 'caf':
        swap = [int(i in golden['caf_reverse_direction'].tolist()) for i in range(n_fields)]
    want = golden['q%d_%s' % (quad, kind)]
    got = oracle.fields_from_conv(hu.compose(conv, n_fields, kind, quad, src, swap),
                                  n_fields, kind, 0)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert got.tobytes() == want.tobytes()
