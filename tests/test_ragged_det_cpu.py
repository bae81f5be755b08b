"""Ragged CifDet batches without a GPU: the guard that zero-padding changes the detections (the
reason pp_cifdet_decode_ragged exists), and the two exports with every argument error, all
returned before any copy or launch.  Pointers are dummies that are never dereferenced;
accepted arguments are probed with n_img = 0, which passes every check and launches nothing."""
import ctypes
import os
import re

import pytest

import oracle
import ragged_det_util as rd
from openpifpaf_amd import _abi, _lib
from openpifpaf_amd.decoder.generator.cifdet import det_nms_config

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
EINVAL, ESHAPE, ENOMEM = -1, -2, -5
NAME, SIZE = 'pp_cifdet_decode_ragged', 'pp_cifdet_ragged_workspace_size'


# ---- the padding guard ----------------------------------------------------------------------
def test_zero_padding_gives_other_detections():
    """det_uniform at the five shapes smaller than the 24x30 container, seeds 0-5: the oracle's
    own-size decode differs from its decode of the zero-padded field in every one of the 30
    cases (measured: 30 of 30); at the container's own size padding changes nothing."""
    cfg = rd.config('uniform')
    differ = 0
    for h, w in rd.SHAPES:
        for seed in range(6):
            own = rd.own_decode('uniform', h, w, seed)
            pad = oracle.cifdet_decode(rd.padded(rd.image('uniform', h, w, seed)), cfg)
            same = len(own) == len(pad) and all(
                own[n].tobytes() == pad[n].tobytes() for n in ('field', 'score', 'bbox'))
            if (h, w) == rd.CONTAINER:
                assert same, seed
            else:
                assert len(own) > 0, (h, w, seed)
                differ += not same
    print('padded decodes that differ:', differ, 'of 30')
    assert differ == 30


# ---- the C ABI ------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from openpifpaf_amd import build
    build.build(verbose=False)
    return _lib.load()


def test_symbols_declared_and_exported(lib):
    text = open(os.path.join(REPO, 'include', 'pifpaf_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name, ret, n_args in ((NAME, 'int', 17), (SIZE, 'size_t', 6)):
        assert re.search(r'\b' + ret + r'\s+' + name + r'\s*\(', text), name
        assert name in _lib.EXPORTED
        assert hasattr(lib, name)
        assert len(_lib._SIGNATURES[name][0]) == n_args
        decl = re.search(name + r'\s*\((.*?)\)\s*;', text, flags=re.S).group(1)
        assert len(decl.split(',')) == n_args
    assert lib.pp_version() == _abi.PP_ABI_VERSION == 4


DUMMY = 256
ARGS = ('det', 'd_extents', 'extents', 'cfg', 'nms', 'out', 'counts', 'status', 'workspace')


def _call(lib, extents=((3, 4), (5, 7)), n_img=None, K=3, H=5, W=7, cap=64, cfg=None,
          workspace_bytes=None, null=(), cifhr=None):
    """Two images of 3x4 and 5x7 in a 5x7 container, unless told otherwise."""
    n = len(extents) if n_img is None else n_img
    cfg = cfg or rd.config('uniform')
    nms = det_nms_config()
    ext = (ctypes.c_int32 * max(2 * len(extents), 2))(*[v for row in extents for v in row])
    if workspace_bytes is None:
        workspace_bytes = getattr(lib, SIZE)(max(n, 0), K, H, W, ctypes.byref(cfg), cap)
    p = {name: ctypes.c_void_p(DUMMY) for name in ARGS}
    p.update(extents=ext, cfg=ctypes.byref(cfg), nms=ctypes.byref(nms))
    for name in null:
        p[name] = None
    return getattr(lib, NAME)(p['det'], n, K, H, W, p['d_extents'], p['extents'], p['cfg'],
                              p['nms'], cifhr, p['out'], cap, p['counts'], p['status'],
                              p['workspace'], ctypes.c_size_t(workspace_bytes), None)


def _error(lib, code, *words, **kw):
    assert _call(lib, **kw) == code
    msg = lib.pp_last_error()
    assert NAME.encode() in msg, msg
    for word in words:
        assert word in msg, msg


@pytest.mark.parametrize('name', ARGS)
def test_null_arguments(lib, name):
    _error(lib, EINVAL, b'NULL', null=(name,))
    _error(lib, EINVAL, b'NULL', null=(name,), n_img=0)


@pytest.mark.parametrize('kw', [dict(n_img=-1), dict(K=0), dict(H=0), dict(W=0), dict(cap=0),
                                dict(K=4097)])
def test_bad_shapes(lib, kw):
    _error(lib, ESHAPE, b'shape', workspace_bytes=1 << 30, **kw)


@pytest.mark.parametrize('extents', [((0, 4), (5, 7)), ((3, 0), (5, 7)), ((3, 4), (-1, 7)),
                                     ((3, 4), (6, 7)), ((3, 4), (5, 8)), ((3, 8), (5, 7))])
def test_extent_errors(lib, extents):
    _error(lib, ESHAPE, b'extent', b'container', extents=extents)


def test_extents_that_fill_the_container_pass(lib):
    # what passes every check would launch, so the accepted side is probed with the empty batch
    assert _call(lib, extents=((5, 7), (1, 1)), n_img=0) == 0


@pytest.mark.parametrize('kw', [dict(cif_threshold=-0.1), dict(seed_threshold=-0.1),
                                dict(cif_threshold=float('nan')),
                                dict(seed_threshold=float('nan'))])
def test_negative_thresholds(lib, kw):
    cfg = _abi.make_config(**dict(dict(cif_threshold=0.1, seed_threshold=0.1), **kw))
    _error(lib, EINVAL, b'threshold', cfg=cfg)
    _error(lib, EINVAL, b'threshold', cfg=cfg, n_img=0)
    zero = _abi.make_config(cif_threshold=0.0, seed_threshold=0.0)
    assert _call(lib, cfg=zero, n_img=0) == 0


def test_workspace_too_small(lib):
    cfg = rd.config('uniform')
    need = getattr(lib, SIZE)(2, 3, 5, 7, ctypes.byref(cfg), 64)
    assert need > 0
    _error(lib, ENOMEM, b'workspace', b'small', workspace_bytes=need - 1)
    _error(lib, ENOMEM, b'workspace', b'small', workspace_bytes=0)


def test_workspace_size(lib):
    """The ragged size is the uniform one at the container's shape, and 0 for what the uniform
    query rejects."""
    cfg = rd.config('uniform')
    size, uniform = getattr(lib, SIZE), lib.pp_cifdet_workspace_size
    for n, k, h, w, cap in ((1, 3, 5, 7, 64), (12, 3, 24, 30, 720), (2, 2, 65, 67, 4355)):
        assert size(n, k, h, w, ctypes.byref(cfg), cap) == uniform(n, k, h, w, ctypes.byref(cfg),
                                                                   cap) > 0
    for n, k, h, w, cap in ((-1, 3, 5, 7, 64), (1, 0, 5, 7, 64), (1, 3, 0, 7, 64), (1, 3, 5, 7, 0)):
        assert size(n, k, h, w, ctypes.byref(cfg), cap) == 0
    assert size(1, 3, 5, 7, None, 64) == 0


def test_empty_batch(lib):
    assert _call(lib, extents=(), n_img=0, workspace_bytes=0, null=()) == 0
    assert _call(lib, n_img=0, cifhr=ctypes.c_void_p(DUMMY)) == 0
