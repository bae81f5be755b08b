"""pp_pack_det_records without a GPU: the symbol is declared and exported, and every argument
refusal comes back with its status and message before anything touches HIP (the pointers are
dummy values), as test_abi.py::test_handover_refusals_pinned pins them for pp_pack_records."""
import ctypes
import os
import re

import pytest

from openpifpaf_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'pp_pack_det_records'
PP_OK, PP_EINVAL, PP_ESHAPE = 0, -1, -2


@pytest.fixture(scope='module')
def lib():
    from openpifpaf_amd import build
    build.build(verbose=False)
    return _lib.load()


def test_symbol_declared_and_exported(lib):
    text = open(os.path.join(REPO, 'include', 'pifpaf_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    decl = re.search(r'\bint\s+' + NAME + r'\s*\(([^)]*)\)', text)
    assert decl, NAME
    assert len(decl.group(1).split(',')) == 10 == len(_lib._SIGNATURES[NAME][0])
    assert NAME in _lib.EXPORTED and hasattr(lib, NAME)


def _args(dets=16, counts=16, status=16, n=1, cap=8, out=16, out_cap=8, out_counts=16,
          out_status=16):
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    return [p(dets), p(counts), p(status), n, cap, p(out), out_cap, p(out_counts),
            p(out_status), None]


NULL = NAME + ': NULL argument'
SHAPE = NAME + ': bad shape'
PAIR = NAME + ': d_status and out_status go together'
REFUSALS = [
    ('NULL d_dets', _args(dets=0), PP_EINVAL, NULL),
    ('NULL d_counts', _args(counts=0), PP_EINVAL, NULL),
    ('NULL out', _args(out=0), PP_EINVAL, NULL),
    ('NULL out_counts', _args(out_counts=0), PP_EINVAL, NULL),
    ('d_status without out_status', _args(out_status=0), PP_EINVAL, PAIR),
    ('out_status without d_status', _args(status=0), PP_EINVAL, PAIR),
    ('n_img=-1', _args(n=-1), PP_ESHAPE, SHAPE),
    ('det_capacity=0', _args(cap=0), PP_ESHAPE, SHAPE),
    ('det_capacity=-1', _args(cap=-1), PP_ESHAPE, SHAPE),
    ('out_capacity=-1', _args(out_cap=-1), PP_ESHAPE, SHAPE),
    ('NULL out and n_img=-1', _args(out=0, n=-1), PP_EINVAL, NULL),
    ('out + 8', _args(out=24), PP_EINVAL, NAME + ': destination not 16-byte aligned'),
    ('d_dets + 8', _args(dets=24), PP_EINVAL, NAME + ': records not 16-byte aligned'),
    ('out + 8 and n_img=0', _args(out=24, n=0), PP_EINVAL,
     NAME + ': destination not 16-byte aligned'),
    ('n_img=0', _args(n=0), PP_OK, None),
    ('n_img=0 without status', _args(n=0, status=0, out_status=0), PP_OK, None),
    ('n_img=0 and out_capacity=0', _args(n=0, out_cap=0), PP_OK, None),
]


@pytest.mark.parametrize('label,args,status,message', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(lib, label, args, status, message):
    rc = lib.pp_pack_det_records(*args)
    assert rc == status, label
    if message is not None:
        assert lib.pp_last_error().decode() == message
