"""Ragged multi-scale batches without a GPU: the new exports and their signatures, every
refusal of pp_decode_multi_ragged and pp_fields_pack_ragged_heads (all returned before
anything touches HIP, so dummy pointers do), the entry-major table layout, and the guard that
gives the GPU tests their worth: for the images they decode, zero-padding every head to its
container gives other records than decoding every head at its own size."""
import ctypes
import os
import re

import numpy as np
import pytest

import ragged_multi_util as rmu
from openpifpaf_amd import _abi, _lib

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
OK, EINVAL, ESHAPE, ENOMEM = 0, -1, -2, -5
DECODE, PACK = 'pp_decode_multi_ragged', 'pp_fields_pack_ragged_heads'
SIZE, OFFSET = 'pp_ragged_heads_tables_size', 'pp_ragged_heads_extents_offset'
SIX = [(p, 0) for p in rmu.PIXELS]


@pytest.fixture(scope='module')
def lib():
    from openpifpaf_amd import build
    build.build(verbose=False)
    return _lib.load()


def test_symbols_declared_and_exported(lib):
    text = open(os.path.join(REPO, 'include', 'pifpaf_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name, ret, n_args in ((DECODE, 'int', 19), (PACK, 'int', 10), (SIZE, 'size_t', 2),
                              (OFFSET, 'size_t', 2)):
        assert re.search(r'\b' + ret + r'\s+' + name + r'\s*\(', text), name
        assert name in _lib.EXPORTED
        assert hasattr(lib, name)
        assert len(_lib._SIGNATURES[name][0]) == n_args
        decl = re.search(name + r'\s*\((.*?)\)\s*;', text, flags=re.S).group(1)
        assert len(decl.split(',')) == n_args
    # pp_decode_multi plus the two tables, in pp_decode_ragged's place for them
    multi = re.search(r'pp_decode_multi\s*\((.*?)\)\s*;', text, flags=re.S).group(1)
    ragged = re.search(DECODE + r'\s*\((.*?)\)\s*;', text, flags=re.S).group(1)
    names = lambda decl: [a.split()[-1].lstrip('*') for a in decl.split(',')]
    assert [a for a in names(ragged) if a not in ('d_extents', 'extents')] == names(multi)


def test_table_sizes(lib):
    """(n_heads, n_img) pointers, then the (n_heads, n_img, 2) int32 extents, entry-major."""
    assert lib.pp_ragged_heads_tables_size(6, 20) == 6 * 20 * 16
    assert lib.pp_ragged_heads_extents_offset(6, 20) == 6 * 20 * 8
    assert lib.pp_ragged_heads_tables_size(3, 1) == lib.pp_ragged_tables_size(3)
    assert lib.pp_ragged_heads_extents_offset(3, 1) == lib.pp_ragged_extents_offset(3)
    for n, heads in ((0, 2), (-1, 2), (2, 0), (2, 33)):
        assert lib.pp_ragged_heads_tables_size(n, heads) == 0
        assert lib.pp_ragged_heads_extents_offset(n, heads) == 0
    assert lib.pp_ragged_heads_tables_size(1, 32) == 32 * 16


# ---- pp_decode_multi_ragged -------------------------------------------------------------------
def _scales(entries):
    """entries: (role, H, W, stride) per pp_scale entry, dummy field pointers."""
    arr = (_abi.Scale * len(entries))()
    for e, (role, h, w, stride) in enumerate(entries):
        arr[e] = _abi.Scale(256 if role != _abi.ROLE_CAF else None,
                            256 if role != _abi.ROLE_CIF else None, h, w, stride, 0.0, 0.0, 0.0, role)
    return arr


TWO = ((_abi.ROLE_CIF, 8, 10, 8), (_abi.ROLE_CIF, 4, 5, 16), (_abi.ROLE_CAF, 8, 10, 8),
       (_abi.ROLE_CAF, 4, 5, 16))
FULL = ((8, 10), (4, 5), (8, 10), (4, 5))


def _decode(lib, entries=TWO, extents=(FULL,), n_img=None, d_extents=256, host=True, hr=None,
            cfg=None, workspace_bytes=16, skeleton=True, k=17, pairs=0):
    """extents: per image, one (h, w) per entry; laid out entry-major as the ABI wants."""
    n = len(extents) if n_img is None else n_img
    table = np.ascontiguousarray(np.array(extents, np.int32).reshape(len(extents), -1, 2)
                                 .transpose(1, 0, 2))
    skel = _abi.skeleton_array(rmu.SKEL)
    cfg = cfg or rmu.config('eval')
    arr = _scales(entries)
    return lib.pp_decode_multi_ragged(
        arr, len(arr), pairs, n, k, 19, ctypes.c_void_p(d_extents),
        table.ctypes.data_as(ctypes.c_void_p) if host else None,
        skel.ctypes.data_as(ctypes.c_void_p) if skeleton else None, ctypes.byref(cfg),
        ctypes.c_void_p(hr), ctypes.c_void_p(256), 8, ctypes.c_void_p(256), ctypes.c_void_p(256),
        ctypes.c_void_p(256), ctypes.c_size_t(workspace_bytes), 15, None)


def _refused(lib, code, *words, **kw):
    assert _decode(lib, **kw) == code
    msg = lib.pp_last_error()
    for word in words:
        assert word in msg, msg


def test_decode_refusals(lib):
    _refused(lib, EINVAL, b'pp_decode_multi_ragged', b'NULL', d_extents=None)
    _refused(lib, EINVAL, b'pp_decode_multi_ragged', b'NULL', host=False)
    _refused(lib, EINVAL, b'pp_decode_multi_ragged', b'd_cifhr', hr=256)
    for name in ('cif_threshold', 'seed_threshold', 'caf_threshold', 'complete_caf_threshold'):
        _refused(lib, EINVAL, b'pp_decode_multi_ragged', b'thresholds',
                 cfg=rmu.config('eval', **{name: -0.5}))
    hrmap = TWO + ((_abi.ROLE_HRMAP, 8, 10, 8),)
    _refused(lib, EINVAL, b'pp_decode_multi_ragged', b'PP_ROLE_HRMAP', entries=hrmap,
             extents=(FULL + ((8, 10),),))
    # ... and all of them for an empty batch too, which reads no extent
    _refused(lib, EINVAL, b'NULL', d_extents=None, n_img=0)
    _refused(lib, EINVAL, b'd_cifhr', hr=256, n_img=0)
    _refused(lib, EINVAL, b'thresholds', cfg=rmu.config('eval', caf_threshold=-0.5), n_img=0)
    _refused(lib, EINVAL, b'PP_ROLE_HRMAP', entries=hrmap, extents=(FULL + ((8, 10),),), n_img=0)


@pytest.mark.parametrize('entry', range(4))
@pytest.mark.parametrize('bad', [(0, 1), (1, 0), (-1, 3), (99, 1), (1, 99)])
def test_decode_extent_refusals(lib, entry, bad):
    """An extent <= 0 or beyond ITS entry's (H, W), in any entry and any image."""
    h, w = FULL[entry]
    row = list(FULL)
    row[entry] = (h + 1, w) if bad == (99, 1) else (h, w + 1) if bad == (1, 99) else bad
    _refused(lib, ESHAPE, b'pp_decode_multi_ragged', b'extent', extents=(FULL, tuple(row)))
    _refused(lib, ESHAPE, b'extent', extents=(tuple(row), FULL))


def test_decode_accepts(lib):
    """What passes the ragged checks reaches pp_decode_multi's own (here: the workspace), and an
    empty batch is PP_OK."""
    small = ((3, 10), (4, 1), (8, 2), (1, 5))
    _refused(lib, ENOMEM, b'workspace too small', extents=(FULL, small))
    # the fine head's extent may exceed the coarse head's container: each entry has its own
    _refused(lib, ENOMEM, b'workspace too small', extents=(((8, 10), (1, 1), (8, 10), (1, 1)),))
    assert _decode(lib, n_img=0) == OK
    assert _decode(lib, n_img=0, extents=(((0, 0),) * 4,)) == OK
    one = ((_abi.ROLE_CIF, 8, 10, 8), (_abi.ROLE_CAF, 8, 10, 8))
    _refused(lib, ENOMEM, b'workspace too small', entries=one, extents=(((8, 10), (5, 3)),))
    assert _decode(lib, entries=one, extents=(((8, 10), (8, 10)),), n_img=0) == OK
    # pp_decode_multi's refusals stay in force
    _refused(lib, ESHAPE, k=25)
    _refused(lib, EINVAL, b'NULL', skeleton=False)
    _refused(lib, ESHAPE, b'multiple', pairs=1, entries=TWO[:1] + TWO[2:],
             extents=(((8, 10), (8, 10), (4, 5)),))


# ---- pp_fields_pack_ragged_heads --------------------------------------------------------------
def _pack(lib, extents=(((3, 4), (2, 2)), ((5, 7), (1, 1))), sizes=((5, 7), (5, 7)),
          planes=(85, 171), ptrs=None, containers=(256, 512), n_img=None, n_heads=None,
          tables=4096, tables_bytes=None, null=None):
    """extents[m][i]: head m, image i."""
    nh = len(extents) if n_heads is None else n_heads
    n = len(extents[0]) if n_img is None else n_img
    flat = [v for head in extents for e in head for v in e]
    ext = (ctypes.c_int32 * len(flat))(*flat)
    m = len(flat) // 2
    ptr = (ctypes.c_void_p * m)(*(ptrs if ptrs is not None else [256] * m))
    pl = (ctypes.c_int32 * len(planes))(*planes)
    sz = (ctypes.c_int32 * (2 * len(sizes)))(*[v for s in sizes for v in s])
    out = (ctypes.c_void_p * len(containers))(*containers)
    args = [ptr, ext, n, nh, pl, sz, out, ctypes.c_void_p(tables)]
    if null is not None:
        args[null] = None
    if tables_bytes is None:
        tables_bytes = lib.pp_ragged_heads_tables_size(max(n, 0), max(nh, 0))
    return lib.pp_fields_pack_ragged_heads(*args, ctypes.c_size_t(tables_bytes), None)


def _pack_refused(lib, code, *words, **kw):
    assert _pack(lib, **kw) == code
    msg = lib.pp_last_error()
    assert PACK.encode() in msg, msg
    for word in words:
        assert word in msg, msg


def test_pack_refusals(lib):
    for null in (0, 1, 4, 5, 6, 7):
        _pack_refused(lib, EINVAL, b'NULL', null=null)
        _pack_refused(lib, EINVAL, b'NULL', null=null, n_img=0)
    _pack_refused(lib, EINVAL, b'NULL field', ptrs=[256, 256, 0, 256])
    _pack_refused(lib, EINVAL, b'NULL container', containers=(256, 0))
    _pack_refused(lib, EINVAL, b'misaligned', containers=(256, 514))
    _pack_refused(lib, EINVAL, b'misaligned', tables=4096 + 4)
    _pack_refused(lib, ESHAPE, b'shape', n_heads=0)
    _pack_refused(lib, ESHAPE, b'shape', n_img=-1)
    _pack_refused(lib, ESHAPE, b'shape', planes=(85, 0))
    _pack_refused(lib, ESHAPE, b'shape', sizes=((5, 7), (0, 7)))
    _pack_refused(lib, ESHAPE, b'shape', sizes=((5, 7), (1 << 16, 1 << 15)))
    _pack_refused(lib, ESHAPE, b'PP_MAX_SCALES', n_heads=33, extents=(((1, 1),),) * 33,
                  sizes=((1, 1),) * 33, planes=(1,) * 33, containers=(256,) * 33)
    for bad in ((0, 2), (2, 0), (-1, 2), (6, 7), (5, 8)):
        _pack_refused(lib, ESHAPE, b'extent', b'container', extents=(((3, 4), (2, 2)), ((5, 7), bad)))
        _pack_refused(lib, ESHAPE, b'extent', b'container', extents=(((3, 4), bad), ((5, 7), (1, 1))))
    # each head against its own container
    _pack_refused(lib, ESHAPE, b'extent', sizes=((5, 7), (5, 6)))
    need = lib.pp_ragged_heads_tables_size(2, 2)
    _pack_refused(lib, ENOMEM, b'table', b'small', tables_bytes=need - 1)
    # what passes these checks would launch: the accepted side is probed with the empty batch
    assert _pack(lib, n_img=0) == OK
    assert _pack(lib, n_img=0, tables=4096 + 4, tables_bytes=0, containers=(256 + 4, 512)) == OK
    assert _pack(lib, n_img=0, n_heads=32, extents=(((1, 1),),) * 32, sizes=((1, 1),) * 32,
                 planes=(1,) * 32, containers=(256,) * 32) == OK


# ---- the python route's refusals that need no device ------------------------------------------
def test_options_still_refused_with_a_multi_scale_config():
    from openpifpaf_amd import constants, decoder
    fc = decoder.FieldConfig(**rmu.field_config_kwargs('ms2'))
    cc = decoder.CifCaf(fc, keypoints=constants.COCO_KEYPOINTS, skeleton=rmu.SKEL)
    fields = list(rmu.image('ms2', 97, 129, 0))
    for kw in ({'group': object()}, {'initial_annotations': [object()]}, {'keep_cifhr': True}):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            cc.decode_ragged([fields], **kw)
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            cc.coco_ragged([fields], [{}], **kw)
    with pytest.raises(TypeError, match='unexpected'):
        cc.decode_ragged([fields], bogus=1)


def test_short_per_head_lists_are_refused():
    """The reference zips the per-head lists, so a short one drops heads there; a ragged batch
    asks for one entry per head, before anything goes to a device."""
    from openpifpaf_amd import constants, decoder, engine
    kw = rmu.field_config_kwargs('ms2')
    fields = list(rmu.image('ms2', 97, 129, 0))
    for name in ('cif_strides', 'cif_min_scales', 'caf_strides', 'caf_min_distances',
                 'caf_max_distances'):
        fc = decoder.FieldConfig(**dict(kw, **{name: kw[name][:1]}))
        with pytest.raises(NotImplementedError, match=name + ' has 1'):
            engine.check_head_lists(fc)
        cc = decoder.CifCaf(fc, keypoints=constants.COCO_KEYPOINTS, skeleton=rmu.SKEL)
        with pytest.raises(NotImplementedError, match='single-scale'):
            cc.decode_ragged([fields])
        with pytest.raises(NotImplementedError, match=name):
            cc.coco_ragged([fields], [{}])
    engine.check_head_lists(decoder.FieldConfig(**kw))
    for name in rmu.CONFIGS:
        engine.check_head_lists(decoder.FieldConfig(**rmu.field_config_kwargs(name)))


# ---- the guard --------------------------------------------------------------------------------
def test_field_sizes():
    for name in rmu.PLANTED:
        strides = rmu.field_config_kwargs(name)['cif_strides']
        for h_px, w_px in rmu.PIXELS:
            fields = rmu.image(name, h_px, w_px, 0)
            assert len(fields) == 2 * len(strides)
            for m, stride in enumerate(strides):
                want = ((h_px - 1) // stride + 1, (w_px - 1) // stride + 1)
                assert fields[2 * m].shape == (17, 5) + want
                assert fields[2 * m + 1].shape == (19, 9) + want
    blocks = rmu.padded(rmu.images('ms2', SIX))
    assert [b.shape[3:] for b in blocks] == [(24, 30), (24, 30), (12, 15), (12, 15)]


@pytest.mark.parametrize('mode', rmu.MODES)
@pytest.mark.parametrize('name', rmu.PLANTED)
def test_padding_gives_other_records(name, mode):
    """A condition of the GPU tests' worth, on the seed-0 images they decode: every image
    decodes to at least one record, and at least one image's records change when every head is
    zero-padded to its container.  (Seed 0 meets both in all six combinations; no other seed
    was needed.)"""
    cfg = rmu.config(mode)
    own = [rmu.own_decode(name, h, w, seed, mode, cfg) for (h, w), seed in SIX]
    assert all(len(r) >= 1 for r in own), [len(r) for r in own]
    padded = rmu.padded_decode(name, SIX, cfg)
    differ = [i for i, (a, b) in enumerate(zip(own, padded))
              if len(a) != len(b) or any(a[k].tobytes() != b[k].tobytes()
                                         for k in ('data', 'joint_scales', 'score'))]
    assert differ, 'zero-padding changed nothing: the ragged route would be untested'
    # the largest image fills every container: padding is the identity there
    assert 5 not in differ
