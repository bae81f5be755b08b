"""Eval preprocessing with extended scale, turns and the multi-scale input pyramid
(eval_coco.py:359-384, transforms/rotate.py, network/nets.py:111-131): the host twin
pp_preprocess_views_cpu through EvalViews.batch_cpu against the reference's fixture
(tests/golden/preprocess_views.npz), against EvalPreprocess with the flags off and against
NumPy slicing, the metas and annotations, the refusals and the argument checks of both entries.
All comparisons are exact.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import preprocess_util as pu
import preprocess_views_util as vu
from openpifpaf_amd import _abi, _lib, preprocess, preprocess_views, transforms
from openpifpaf_amd.transforms import EvalPreprocess, EvalViews

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
HEADER = os.path.join(REPO, 'include', 'pifpaf_amd.h')
NAMES = ('pp_preprocess_views_tables_size', 'pp_preprocess_views', 'pp_preprocess_views_cpu')
PP_OK, PP_EINVAL, PP_ESHAPE, PP_ENOMEM = 0, -1, -2, -5


@pytest.fixture(scope='module')
def lib():
    from openpifpaf_amd import build
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope='module')
def cases():
    return vu.load()[1]


# ---- 1. ABI -----------------------------------------------------------------------------
def test_symbols_declared_and_exported(lib):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert lib.pp_version() == _abi.PP_ABI_VERSION == 4
    assert transforms.EvalViews is preprocess_views.EvalViews
    assert lib.pp_preprocess_views_tables_size(0, 10) == 0
    assert lib.pp_preprocess_views_tables_size(3, 0) == 0
    one = lib.pp_preprocess_views_tables_size(1, 1)
    assert one >= 3 * 256 * 4
    assert lib.pp_preprocess_views_tables_size(3, 10) > lib.pp_preprocess_views_tables_size(3, 1) \
        > one


def test_view_image_layout_matches_header(tmp_path):
    fields = ('src_offset', 'h', 'w', 'th', 'tw', 'left', 'top', 'H', 'W', 'rot', 'reserved')
    src = tmp_path / 'view_layout.c'
    src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "pifpaf_amd.h"
int main(void) {
  printf("%%zu", sizeof(pp_view_image));
%s
  printf("\\n%%d %%d %%d %%d %%d\\n", PP_VIEW_R1, PP_VIEW_R1_5, PP_VIEW_R2, PP_VIEW_R3, PP_VIEW_R5);
  return 0;
}
''' % '\n'.join('  printf(" %%zu", offsetof(pp_view_image, %s));' % f for f in fields))
    exe = tmp_path / 'view_layout'
    subprocess.check_call(['gcc', '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    d = _abi.VIEW_IMAGE_DTYPE
    assert d.names == fields
    assert [int(v) for v in lines[0].split()] == [d.itemsize] + [d.fields[k][1] for k in fields]
    assert d.itemsize == ctypes.sizeof(_abi.ViewImage)
    assert [(n, getattr(_abi.ViewImage, n).offset) for n, _ in _abi.ViewImage._fields_] == \
        [(k, d.fields[k][1]) for k in fields]
    assert [int(v) for v in lines[1].split()] == [
        _abi.PP_VIEW_R1, _abi.PP_VIEW_R1_5, _abi.PP_VIEW_R2, _abi.PP_VIEW_R3, _abi.PP_VIEW_R5]
    assert _abi.PP_VIEW_ALL == 31


# ---- 2. what the comparisons need so as not to pass vacuously, from the fixture alone ----
def test_fixture_conditions(cases):
    fx = vu.load()[0]
    assert all(c.src.min() > 0 for c in cases)
    pyr = [c for c in cases if c.ms and not c.ori]
    edges = {c.long_edge for c in pyr}
    assert edges == {16, 17, 26, 29, 30, 33, 47}
    assert {e % 3 for e in edges} == {0, 1, 2} and {e % 5 == 0 for e in edges} == {True, False}
    assert {-(-e * e // 1024) for e in edges} == {1, 2, 3}  # workgroup tiles per canvas
    assert all(c.src.shape[0] != c.src.shape[1] for c in pyr)
    fill = np.uint8(preprocess.FILL)
    assert any((c.u8[:, 0] == fill).all() and not (c.u8[0] == fill).all() for c in pyr)  # left pad
    assert any((c.u8[0] == fill).all() and not (c.u8[:, 0] == fill).all() for c in pyr)  # top pad
    # the black last rescaled row of the (8, 2) -> 26 source, kept by reduction 5 (row 25)
    c = next(c for c in pyr if c.src.shape[:2] == (8, 2))
    inner = (c.u8[25] != fill).any(axis=1)
    assert inner.any() and (c.u8[25][inner] == 0).all() and (c.u8[24][inner] != 0).any()
    zero = ((np.float32(0) - np.float32(preprocess.MEAN)) / np.float32(preprocess.STD))
    cols = [x // 5 for x in range(26) if x % 5 == 0 and inner[x]]
    assert cols and (c.views[4][:, 5, cols] == zero[:, None]).all()
    for c in cases:
        if c.views is not None:  # view sizes and the mirrored half really mirrored
            n = c.long_edge
            assert [v.shape for v in c.views[:5]] == \
                [(3, s, s) for s in preprocess_views.view_sizes(n)]
            assert all(np.array_equal(c.views[v + 5], c.views[v][:, :, ::-1]) for v in range(5))
            assert not np.array_equal(c.views[5], c.views[0])
    turns = [c for c in cases if not c.ms]
    only_ori = [c for c in turns if c.ori and not c.ext]
    assert {float(c.meta['rotation'][0]) for c in only_ori} == {0.0, 90.0, 180.0, 270.0}
    assert all(c.u8.shape[0] == c.long_edge for c in only_ori)  # at full size
    for tight in (False, True):
        ext = [c for c in turns if c.ext and not c.ori and c.tight == tight]
        for edge in (16, 17, 33):
            longest = {int(round(max(c.meta['valid_area'][2:]))) + 1
                       for c in ext if c.long_edge == edge}
            assert longest == {edge, (edge - 1) // 2 + 1}
    both = [c for c in turns if c.ext and c.ori]
    assert any(c.meta['rotation'][0] and max(c.meta['valid_area'][2:]) < c.long_edge // 2 + 1
               for c in both)
    assert {c.long_edge for c in turns} == {16, 17, 33}
    assert {c.image_id for c in turns} == set(range(1, 9))
    # no turned canvas equals its unturned one: image id 1 of the same run is not turned; with
    # extended scale too, the same id's canvas of the run without turns has the same scale
    by = {(c.mode, c.image_id): c for c in turns}
    n = 0
    for c in turns:
        if c.meta['rotation'][0]:
            flat = by[((c.long_edge, c.tight, True, False, False), c.image_id)] if c.ext \
                else by[(c.mode, 1)]
            assert flat.meta['rotation'][0] == 0.0 and flat.u8.shape == c.u8.shape
            assert not np.array_equal(flat.u8, c.u8), c.name
            n += 1
    assert n >= 30
    c = next(c for c in cases if c.name == 'all_')
    assert c.long_edge == 29 and c.meta['rotation'][0] == 90.0
    assert float(fx['anns_turned_rotation'][0]) == 90.0
    assert max(fx['anns_half_valid_area'][2:]) < int(fx['anns_long_edge']) // 2 + 1


# ---- 3. the twin against the fixture ----------------------------------------------------
@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('dtype', vu.ALL_DTYPES)
def test_single_images_equal_reference(lib, cases, dtype, channels_last):
    for c in cases:
        pp = vu.make(c, dtype, channels_last)
        out, metas = pp.batch_cpu([c.src], None if c.image_id is None else [c.given_meta()])
        assert len(metas) == 1
        vu.check_meta(metas[0], c)
        vu.check_image(c, out, 0, dtype, channels_last)


def _anns(fx):
    return [{'keypoints': fx['anns_in_keypoints'][a].reshape(-1).tolist(),
             'bbox': fx['anns_in_bbox'][a].tolist(), 'segmentation': [[0.0, 1.0]]}
            for a in range(2)]


@pytest.mark.parametrize('label, flags', [('turned', dict(orientation_invariant=True)),
                                          ('half', dict(extended_scale=True))])
def test_anns_equal_reference(lib, label, flags):
    fx = vu.load()[0]
    edge, image_id = int(fx['anns_long_edge']), int(fx['anns_image_id'])
    src = fx['s%d_src' % edge]
    pp = EvalViews(edge, **flags)
    anns = _anns(fx)
    vplan = pp._view_plan(src.shape[0], src.shape[1], {'image_id': image_id})
    got = vplan.anns(anns)
    assert 'segmentation' in anns[0]  # the caller's annotations are not edited
    for a in range(2):
        assert 'segmentation' not in got[a]
        for key in ('keypoints', 'bbox', 'bbox_original'):
            assert got[a][key].dtype == np.float32
            assert got[a][key].tobytes() == fx['anns_%s_%s' % (label, key)][a].tobytes(), key
    _, (meta,) = pp.batch_cpu([src], [{'image_id': image_id}])
    want = vu.Case(label, src, edge, image_id=image_id, meta=vu._meta(fx, 'anns_%s_' % label))
    vu.check_meta(meta, want)


# ---- 4. mixed batches -------------------------------------------------------------------
@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('dtype', vu.ALL_DTYPES)
def test_mixed_batches_equal_single_images(lib, cases, dtype, channels_last):
    """Every case that one object serves in one call (different ids, so different turns and
    scales side by side): each image gets what it gets alone."""
    sizes = set()
    for mode, group in vu.groups(cases).items():
        pp = vu.make(mode, dtype, channels_last)
        metas_in = None if group[0].image_id is None else [c.given_meta() for c in group]
        out, metas = pp.batch_cpu([c.src for c in group], metas_in)
        assert len(metas) == len(group)
        sizes.add(len(group))
        for i, c in enumerate(group):
            vu.check_meta(metas[i], c)
            vu.check_image(c, out, i, dtype, channels_last)
    assert 8 in sizes


# ---- 5. flags off -----------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.uint8])
def test_flags_off_equals_eval_preprocess(lib, dtype):
    for tight in (False, True):
        for (long_edge, _), group in pu.groups(pu.load()[1]).items():
            if long_edge is None and not tight:
                continue
            images = [c.src for c in group]
            kw = dict(tight_padding=tight, dtype=dtype, channels_last=tight)
            want, want_metas = EvalPreprocess(long_edge, **kw).batch_cpu(images)
            got, metas = EvalViews(long_edge, **kw).batch_cpu(images)
            if not tight:
                want, got = [want], [got]
            assert len(want) == len(got)
            for w, g in zip(want, got):
                assert g.shape == w.shape and g.strides == w.strides and g.dtype == w.dtype
                assert g.tobytes() == w.tobytes()
            for a, b in zip(metas, want_metas):
                assert set(a) == set(b)
                for k in pu.META_KEYS:
                    assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype
                assert a['rotation'] == b['rotation'] and a['hflip'] is b['hflip']


# ---- 6. index arithmetic, exhaustively small --------------------------------------------
def _servable(pp, rng, long_edge):
    """A seeded non-square image and the first image id from long_edge on that the chain
    accepts (the reference's own size assertions refuse some small half-scale sizes)."""
    for image_id in range(long_edge, long_edge + 400):
        h, w = (int(v) for v in rng.integers(2, 60, 2))
        if h == w and long_edge > 2:  # at long_edge 2 only a square image keeps both edges >= 2
            continue
        try:
            pp._view_plan(h, w, {'image_id': image_id})
        except (AssertionError, ValueError):
            continue
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), image_id
    raise AssertionError('no servable image for long_edge {}'.format(long_edge))


@pytest.mark.parametrize('hflip', [True, False])
def test_views_equal_slicing_of_the_turned_canvas(lib, hflip):
    """Every L from 2 to 48, all three modes on, a non-square image (square at L = 2, where
    the chain accepts no other): the twin's views are NumPy slicing of the twin's own turned canvas (uint8, and float32 through the same slicing of the float32
    tensor)."""
    rng = np.random.default_rng(5)
    turns, halves = set(), set()
    for long_edge in range(2, 49):
        flags = dict(extended_scale=True, orientation_invariant=True)
        canvas_pp = EvalViews(long_edge, dtype=torch.uint8, **flags)
        src, image_id = _servable(canvas_pp, rng, long_edge)
        metas = [{'image_id': image_id}]
        canvas, (meta,) = canvas_pp.batch_cpu([src], metas)
        assert canvas.shape == (1, long_edge, long_edge, 3)
        turns.add(meta['rotation']['angle'])
        halves.add(max(meta['valid_area'][2:]) < long_edge // 2 + 1)
        want = vu.reduce_np(canvas, hflip)
        got, _ = EvalViews(long_edge, dtype=torch.uint8, multi_scale=True,
                           multi_scale_hflip=hflip, **flags).batch_cpu([src], metas)
        assert len(got) == len(want) == (10 if hflip else 5)
        for v, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and np.array_equal(g, w), (long_edge, v)
        tensor, _ = EvalViews(long_edge, channels_last=True, **flags).batch_cpu([src], metas)
        want = vu.reduce_np(tensor.transpose(0, 2, 3, 1), hflip)
        got, _ = EvalViews(long_edge, channels_last=True, multi_scale=True,
                           multi_scale_hflip=hflip, **flags).batch_cpu([src], metas)
        for v, (g, w) in enumerate(zip(got, want)):
            g = g.transpose(0, 2, 3, 1)
            assert g.shape == w.shape
            assert np.array_equal(pu.bits(g.copy()), pu.bits(w.copy())), (long_edge, v)
    assert turns == {0.0, 90, 180, 270} and halves == {True, False}


# ---- 7. Python-level checks -------------------------------------------------------------
def test_refusals():
    with pytest.raises(NotImplementedError, match='orientation_invariant with tight_padding'):
        EvalViews(33, tight_padding=True, orientation_invariant=True)
    with pytest.raises(NotImplementedError, match='scipy.ndimage.rotate'):
        EvalViews(33, tight_padding=True, orientation_invariant=True)
    with pytest.raises(NotImplementedError, match='multi_scale with tight_padding'):
        EvalViews(33, tight_padding=True, multi_scale=True)
    with pytest.raises(NotImplementedError, match='fast'):
        EvalViews(33, fast=True)
    with pytest.raises(NotImplementedError, match='resample'):
        EvalViews(33, resample=3)
    with pytest.raises(NotImplementedError, match='long_edge range'):
        EvalViews((30, 40), multi_scale=True)
    with pytest.raises(AssertionError):
        EvalViews(None, multi_scale=True)
    with pytest.raises(AssertionError):
        EvalViews(None, tight_padding=True, extended_scale=True)
    EvalViews(None, tight_padding=True)
    EvalViews(33, tight_padding=True, extended_scale=True)
    pp = EvalViews(33, multi_scale=True)
    for bad in (np.zeros((8, 8), np.uint8), np.zeros((8, 8, 4), np.uint8),
                np.zeros((8, 8, 3), np.float32)):
        with pytest.raises(NotImplementedError, match='3-channel uint8'):
            pp.batch_cpu([bad])


@pytest.mark.parametrize('kwargs, word', [(dict(extended_scale=True), 'extended_scale'),
                                          (dict(orientation_invariant=True),
                                           'orientation_invariant')])
def test_eval_preprocess_still_refuses(kwargs, word):
    with pytest.raises(NotImplementedError, match=word):
        EvalPreprocess(33, **kwargs)


def test_image_id_is_needed_only_for_a_choice(lib):
    im = np.full((9, 12, 3), 7, np.uint8)
    for flags in (dict(extended_scale=True), dict(orientation_invariant=True)):
        pp = EvalViews(17, **flags)
        for metas in (None, [None], [{}], [{'file_name': 'x'}], [{'image_id': 0}],
                      [{'image_id': -3}]):
            with pytest.raises(AssertionError):
                pp.batch_cpu([im], metas)
        pp.batch_cpu([im], [{'image_id': 1}])
    for pp in (EvalViews(17), EvalViews(17, multi_scale=True)):
        for metas in (None, [None], [{}], [{'image_id': 0}]):
            pp.batch_cpu([im], metas)
    with pytest.raises(ValueError, match='metas for'):
        EvalViews(17).batch_cpu([im], [None, None])


def test_plan_keeps_its_positional_signature():
    a = preprocess._Plan(43, 47, 98, False)
    b = preprocess._Plan(43, 47, 98, False, None)
    assert (a.th, a.tw, a.ltrb, a.H, a.W) == (b.th, b.tw, b.ltrb, b.H, b.W)
    half = preprocess._Plan(43, 47, 99, False, 50)
    assert max(half.th, half.tw) == 50 and (half.H, half.W) == (99, 99)
    tight = preprocess._Plan(43, 47, 99, True, 50)
    assert (tight.H, tight.W) == (49, 65)  # the next 16 k + 1 of (45, 50)
    assert (tight.th, tight.tw) == (half.th, half.tw) == (45, 50)


def test_empty_batches(lib):
    assert EvalViews(33, tight_padding=True).batch_cpu([]) == ([], [])
    assert EvalViews(33).batch_cpu([])[0].shape == (0, 3, 33, 33)
    views, metas = EvalViews(33, multi_scale=True, orientation_invariant=True).batch_cpu([])
    assert metas == [] and [v.shape for v in views] == \
        [(0, 3, s, s) for s in (33, 22, 17, 11, 7)] * 2


# ---- 8. argument checks of both entries -------------------------------------------------
def _call(lib, device, *, n=1, dtype=0, layout=0, reductions=31, mirror=1, src=True, descs=True,
          offs=True, out=True, mean=True, std=(0.229, 0.224, 0.225), fill=True, tables=True,
          tables_bytes=1 << 20, src_bytes=None, out_elems=None, offsets=None, **desc):
    """One 4x5 -> 8x10 image padded to 12x12, all ten views; device=True calls
    pp_preprocess_views with dummy device pointers (every refusal comes before anything
    touches them)."""
    d = np.zeros(1, _abi.VIEW_IMAGE_DTYPE)
    d[0] = (0, 4, 5, 8, 10, 1, 2, 12, 12, 0, 0)
    for k, v in desc.items():
        d[k] = v
    sizes = [12, 8, 6, 4, 3] * 2
    o = np.zeros(sum(3 * s * s for s in sizes), np.float32)
    off = np.zeros(10, np.int64)
    off[1:] = np.cumsum([3 * s * s for s in sizes])[:-1]
    if offsets is not None:
        for k, v in offsets.items():
            off[k] = v
    s = np.zeros(4 * 5 * 3, np.uint8)
    m = np.float32(preprocess.MEAN)
    sd = np.asarray(std, np.float32)
    f = np.uint8(preprocess.FILL)
    vp = lambda a, on: a.ctypes.data_as(ctypes.c_void_p) if on else None
    dev = lambda on: ctypes.c_void_p(256) if on else None
    head = [dev(src) if device else vp(s, src), s.size if src_bytes is None else src_bytes,
            vp(d, descs), vp(off, offs), n, reductions, mirror,
            dev(out) if device else vp(o, out), o.size if out_elems is None else out_elems,
            dtype, layout, vp(m, mean), vp(sd, True), vp(f, fill)]
    if device:
        return lib.pp_preprocess_views(*head, dev(tables), tables_bytes, None)
    return lib.pp_preprocess_views_cpu(*head)


BAD_ARGS = [
    ('turn of a non-square', dict(rot=1, W=13, reductions=1, mirror=0), PP_ESHAPE, 'turn needs'),
    ('pyramid of a non-square', dict(W=13), PP_ESHAPE, 'need a square'),
    ('mirror of a non-square', dict(W=13, reductions=1, mirror=1), PP_ESHAPE, 'need a square'),
    ('two views of a non-square', dict(H=13, reductions=5, mirror=0), PP_ESHAPE, 'need a square'),
    ('last view beyond buffer', dict(out_elems=3 * 2 * (144 + 64 + 36 + 16 + 9) - 1), PP_ESHAPE,
     'view region beyond'),
    ('view offset beyond buffer', dict(offsets={3: 3 * 2 * 269 - 47}), PP_ESHAPE,
     'view region beyond'),
    ('negative view offset', dict(offsets={7: -1}), PP_ESHAPE, 'view region beyond'),
    ('empty mask', dict(reductions=0), PP_EINVAL, 'reduction mask'),
    ('unknown mask', dict(reductions=32), PP_EINVAL, 'reduction mask'),
    ('negative mask', dict(reductions=-1), PP_EINVAL, 'reduction mask'),
    ('rot=4', dict(rot=4), PP_EINVAL, 'rot'),
    ('rot=-1', dict(rot=-1), PP_EINVAL, 'rot'),
    ('dtype=4', dict(dtype=4), PP_EINVAL, 'unknown dtype'),
    ('layout=2', dict(layout=2), PP_EINVAL, 'unknown layout'),
    ('NULL src', dict(src=False), PP_EINVAL, 'NULL'),
    ('NULL images', dict(descs=False), PP_EINVAL, 'NULL'),
    ('NULL offsets', dict(offs=False), PP_EINVAL, 'NULL'),
    ('NULL out', dict(out=False), PP_EINVAL, 'NULL'),
    ('NULL mean', dict(mean=False), PP_EINVAL, 'NULL'),
    ('NULL fill', dict(fill=False), PP_EINVAL, 'NULL'),
    ('std 0', dict(std=(0.229, 0.0, 0.225)), PP_EINVAL, 'std'),
    ('h=1', dict(h=1), PP_ESHAPE, 'edge < 2'),
    ('left too large', dict(left=3), PP_ESHAPE, 'does not fit'),
    ('src beyond buffer', dict(src_offset=1), PP_ESHAPE, 'beyond the source buffer'),
    ('n_img=-1', dict(n=-1), PP_ESHAPE, 'n_img'),
]
# pp_last_error() of every row as the library gave it before both entries shared one host
# layer, after the entry's name and ': ' (recorded from that build, not from this one)
_SQUARE = 'reduced or mirrored views need a square output (H == W)'
_REGION = 'a view region beyond the output buffer'
_MASK = 'empty or unknown reduction mask'
BAD_ARGS_TEXT = {
    'turn of a non-square': 'a turn needs a square output (H == W)',
    'pyramid of a non-square': _SQUARE, 'mirror of a non-square': _SQUARE,
    'two views of a non-square': _SQUARE,
    'last view beyond buffer': _REGION, 'view offset beyond buffer': _REGION,
    'negative view offset': _REGION,
    'empty mask': _MASK, 'unknown mask': _MASK, 'negative mask': _MASK,
    'rot=4': 'rot must be 0, 1, 2 or 3', 'rot=-1': 'rot must be 0, 1, 2 or 3',
    'dtype=4': 'unknown dtype', 'layout=2': 'unknown layout',
    'NULL src': 'NULL argument', 'NULL images': 'NULL argument', 'NULL offsets': 'NULL argument',
    'NULL out': 'NULL argument', 'NULL mean': 'NULL argument', 'NULL fill': 'NULL argument',
    'std 0': 'std must be finite and not 0',
    'h=1': 'a source or target edge < 2',
    'left too large': 'the target does not fit its output with this pad',
    'src beyond buffer': 'a source image beyond the source buffer',
    'n_img=-1': 'n_img < 0',
}


@pytest.mark.parametrize('device', [False, True], ids=['cpu', 'device'])
@pytest.mark.parametrize('case', BAD_ARGS, ids=[c[0] for c in BAD_ARGS])
def test_bad_arguments(lib, case, device):
    name, kwargs, code, word = case
    assert _call(lib, device, **kwargs) == code
    assert word in lib.pp_last_error().decode()
    entry = 'pp_preprocess_views' if device else 'pp_preprocess_views_cpu'
    assert lib.pp_last_error().decode() == '{}: {}'.format(entry, BAD_ARGS_TEXT[name])


def test_tables_and_empty_batch(lib):
    assert _call(lib, False) == PP_OK
    assert _call(lib, False, rot=3) == PP_OK
    assert _call(lib, False, W=13, rot=0, reductions=1, mirror=0) == PP_OK  # plain, not square
    assert _call(lib, True, tables=False) == PP_EINVAL  # refused without a launch
    assert 'NULL' in lib.pp_last_error().decode()
    need = lib.pp_preprocess_views_tables_size(1, 10)
    assert _call(lib, True, tables_bytes=need - 1) == PP_ENOMEM
    assert 'table buffer too small' in lib.pp_last_error().decode()
    for device in (False, True):  # n_img == 0 succeeds whatever the pointers are
        assert _call(lib, device, n=0, src=False, descs=False, offs=False, out=False, mean=False,
                     fill=False, tables=False) == PP_OK


# ---- 9. the metas downstream ------------------------------------------------------------
def test_metas_feed_meta_record(lib, cases):
    turned = [c for c in cases if not c.ms and c.meta['rotation'][0]]
    assert {c.meta['rotation'][0] for c in turned} == {90.0, 180.0, 270.0}
    for c in turned:
        _, (meta,) = vu.make(c).batch_cpu([c.src], [c.given_meta()])
        rec = transforms.meta_record(meta)
        assert rec['rotation_angle'][0] == c.meta['rotation'][0]
        assert rec['rotation_width'][0] == rec['rotation_height'][0] == c.long_edge
        assert np.array_equal(rec['offset'][0], c.meta['offset'])
        assert np.array_equal(rec['scale'][0], c.meta['scale'])
        assert rec['width'][0] == c.src.shape[1] and rec['hflip'][0] == 0
