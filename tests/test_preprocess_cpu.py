"""Eval preprocessing (eval_coco.preprocess_factory: RescaleAbsolute, CenterPad /
CenterPadTight, EVAL_TRANSFORM): the host twin pp_preprocess_images_cpu through
EvalPreprocess.batch_cpu against the reference's fixture (tests/golden/preprocess.npz) and
against scipy.ndimage.zoom, the metas and annotations, the options that are out of scope and
the argument checks of both entries.  All comparisons are exact.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import preprocess_util as pu
from openpifpaf_amd import _abi, _lib, preprocess, transforms
from openpifpaf_amd.transforms import EvalPreprocess

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
HEADER = os.path.join(REPO, 'include', 'pifpaf_amd.h')
NAMES = ('pp_preprocess_tables_size', 'pp_preprocess_images', 'pp_preprocess_images_cpu')
PP_OK, PP_EINVAL, PP_ESHAPE = 0, -1, -2


@pytest.fixture(scope='module')
def lib():
    from openpifpaf_amd import build
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope='module')
def cases():
    return pu.load()[1]


def test_symbols_declared_and_exported(lib):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert lib.pp_version() == _abi.PP_ABI_VERSION == 4
    assert transforms.EvalPreprocess is preprocess.EvalPreprocess
    assert lib.pp_preprocess_tables_size(0) == 0
    assert lib.pp_preprocess_tables_size(3) > lib.pp_preprocess_tables_size(1) >= 3 * 256 * 4


def test_descriptor_layout_matches_header(tmp_path):
    src = tmp_path / 'desc_layout.c'
    src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "pifpaf_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(pp_image_desc),
         offsetof(pp_image_desc, src_offset), offsetof(pp_image_desc, out_offset),
         offsetof(pp_image_desc, h), offsetof(pp_image_desc, w), offsetof(pp_image_desc, th),
         offsetof(pp_image_desc, tw), offsetof(pp_image_desc, left), offsetof(pp_image_desc, top),
         offsetof(pp_image_desc, H), offsetof(pp_image_desc, W));
  printf("%d %d %d %d %d %d\\n", PP_PRE_F32, PP_PRE_F16, PP_PRE_BF16, PP_PRE_U8, PP_PRE_PLANAR,
         PP_PRE_CHANNELS_LAST);
  return 0;
}
''')
    exe = tmp_path / 'desc_layout'
    subprocess.check_call(['gcc', '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    d = _abi.IMAGE_DESC_DTYPE
    assert [int(v) for v in lines[0].split()] == [d.itemsize] + [
        d.fields[k][1] for k in ('src_offset', 'out_offset', 'h', 'w', 'th', 'tw', 'left', 'top',
                                 'H', 'W')]
    assert d.itemsize == ctypes.sizeof(_abi.ImageDesc)
    assert [int(v) for v in lines[1].split()] == [
        _abi.PP_PRE_F32, _abi.PP_PRE_F16, _abi.PP_PRE_BF16, _abi.PP_PRE_U8, _abi.PP_PRE_PLANAR,
        _abi.PP_PRE_CHANNELS_LAST]


def test_fixture_conditions(cases):
    """What the comparisons need so as not to pass vacuously, from the fixture alone."""
    fx = pu.load()[0]
    assert fx['row0'].any() and fx['col0'].any() and (~fx['row0'] & ~fx['col0']).any()
    assert all(c.src.min() > 0 for c in cases)
    assert any(c.meta['offset'][0] < 0 for c in cases) and any(c.meta['offset'][1] < 0 for c in cases)
    assert any(c.long_edge is None for c in cases)
    assert len({c.u8.shape for c in cases if c.tight}) > 3  # a ragged batch


# ---- the reference's fixture ------------------------------------------------------------
def check_case(case, got, dtype, channels_last):
    if dtype == torch.uint8:
        assert got.dtype == np.uint8 and got.shape == case.u8.shape, case.name
        assert got.tobytes() == case.u8.tobytes(), case.name
        return
    assert got.shape == (1,) + case.f32.shape, (case.name, got.shape)
    # a (1, 3, H, W) view of (1, H, W, 3) memory, or plain (1, 3, H, W) memory
    nhwc = got.transpose(0, 2, 3, 1).flags['C_CONTIGUOUS']
    assert nhwc == channels_last and got.flags['C_CONTIGUOUS'] != channels_last, case.name
    assert np.array_equal(pu.bits(np.ascontiguousarray(got)), pu.bits(pu.expected(case, dtype))), \
        (case.name, dtype, channels_last)


@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('dtype', pu.DTYPES + (torch.uint8,))
def test_single_images_equal_reference(lib, cases, dtype, channels_last):
    for c in cases:
        pp = EvalPreprocess(c.long_edge, tight_padding=c.tight, dtype=dtype,
                            channels_last=channels_last)
        out, metas = pp.batch_cpu([c.src])
        assert len(metas) == 1
        pu.check_meta(metas[0], c)
        check_case(c, pu.one(out, 0, c.tight, dtype), dtype, channels_last)


@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('dtype', pu.DTYPES + (torch.uint8,))
def test_mixed_batches_equal_single_images(lib, cases, dtype, channels_last):
    """Every case that one object serves in one call: each image gets what it gets alone."""
    for (long_edge, tight), group in pu.groups(cases).items():
        pp = EvalPreprocess(long_edge, tight_padding=tight, dtype=dtype,
                            channels_last=channels_last)
        out, metas = pp.batch_cpu([c.src for c in group])
        assert len(out) == len(metas) == len(group)
        for i, c in enumerate(group):
            pu.check_meta(metas[i], c)
            check_case(c, pu.one(out, i, tight, dtype), dtype, channels_last)


def test_all_cases_one_call(lib, cases):
    """The C entry itself takes any mix: all cases' descriptors in ONE call of the twin give
    each image the bytes it gets alone (float32 planar and uint8)."""
    plans = [preprocess._Plan(c.src.shape[0], c.src.shape[1], c.long_edge, c.tight) for c in cases]
    descs = np.zeros(len(cases), _abi.IMAGE_DESC_DTYPE)
    so = oo = 0
    for d, p in zip(descs, plans):
        d['src_offset'], d['out_offset'] = so, oo
        d['h'], d['w'], d['th'], d['tw'] = p.h, p.w, p.th, p.tw
        d['left'], d['top'], d['H'], d['W'] = p.ltrb[0], p.ltrb[1], p.H, p.W
        so += p.h * p.w * 3
        oo += p.H * p.W * 3
    src = np.concatenate([c.src.reshape(-1) for c in cases])
    mean, std = np.float32(preprocess.MEAN), np.float32(preprocess.STD)
    fill = np.uint8(preprocess.FILL)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for code, np_dtype in ((_abi.PP_PRE_F32, np.float32), (_abi.PP_PRE_U8, np.uint8)):
        out = np.zeros(oo, np_dtype)
        rc = lib.pp_preprocess_images_cpu(vp(src), so, vp(descs), len(cases), vp(out), oo, code,
                                          _abi.PP_PRE_PLANAR, vp(mean), vp(std), vp(fill))
        assert rc == PP_OK, lib.pp_last_error()
        for d, p, c in zip(descs, plans, cases):
            got = out[int(d['out_offset']):int(d['out_offset']) + 3 * p.H * p.W]
            want = c.f32 if code == _abi.PP_PRE_F32 else c.u8
            assert got.tobytes() == want.tobytes(), c.name


def test_input_kinds(lib, cases):
    """np.asarray-able objects (a PIL image when PIL is there, nested lists are not uint8) and
    host torch tensors give the array's result."""
    c = cases[0]
    pp = EvalPreprocess(c.long_edge, tight_padding=c.tight)
    want = pp.batch_cpu([c.src])[0]
    assert np.array_equal(pp.batch_cpu([torch.from_numpy(c.src.copy())])[0], want)

    class ArrayLike:
        def __array__(self, dtype=None, copy=None):
            return c.src

    assert np.array_equal(pp.batch_cpu([ArrayLike()])[0], want)
    try:
        import PIL.Image
    except ImportError:
        return
    assert np.array_equal(pp.batch_cpu([PIL.Image.fromarray(c.src)])[0], want)


def test_passed_meta_keys_are_kept(lib, cases):
    c = cases[1]
    given = {'image_id': 42, 'scale': np.array((2.0, 2.0)), 'file_name': 'x.jpg'}
    pp = EvalPreprocess(c.long_edge, tight_padding=c.tight)
    _, (meta,) = pp.batch_cpu([c.src], [given])
    assert meta['image_id'] == 42 and meta['file_name'] == 'x.jpg'
    assert np.array_equal(meta['scale'], 2.0 * c.meta['scale'])  # not overwritten, then scaled
    assert np.array_equal(given['scale'], (2.0, 2.0)) and set(given) == {'image_id', 'scale',
                                                                        'file_name'}
    assert np.array_equal(meta['offset'], c.meta['offset'])
    rec = transforms.meta_record(meta)
    assert rec['width'][0] == c.src.shape[1] and rec['hflip'][0] == 0


def test_metas_feed_meta_record(lib, cases):
    for c in cases:
        pp = EvalPreprocess(c.long_edge, tight_padding=c.tight)
        _, (meta,) = pp.batch_cpu([c.src], [{'image_id': 7}])
        want = transforms.meta_record(dict(c.meta, hflip=False, rotation=None))
        assert transforms.meta_record(meta).tobytes() == want.tobytes(), c.name


def test_anns_equal_reference(lib):
    fx, cases = pu.load()
    c = next(x for x in cases if x.name == 'c0_')
    anns = [{'keypoints': fx['anns_in_keypoints'][a].reshape(-1).tolist(),
             'bbox': fx['anns_in_bbox'][a].tolist(), 'segmentation': [[0.0, 1.0]]}
            for a in range(2)]
    plan = preprocess._Plan(c.src.shape[0], c.src.shape[1], c.long_edge, c.tight)
    got = plan.anns(anns)
    assert 'segmentation' in anns[0]  # the caller's annotations are not edited
    for a in range(2):
        assert 'segmentation' not in got[a]
        for key in ('keypoints', 'bbox', 'bbox_original'):
            assert got[a][key].dtype == np.float32
            assert got[a][key].tobytes() == fx['anns_' + key][a].tobytes(), key


# ---- out of scope -----------------------------------------------------------------------
@pytest.mark.parametrize('kwargs, word', [
    (dict(fast=True), 'fast'), (dict(resample=3), 'resample'), (dict(resample=0), 'resample'),
    (dict(extended_scale=True), 'extended_scale'),
    (dict(orientation_invariant=True), 'orientation_invariant'),
])
def test_out_of_scope_options(kwargs, word):
    with pytest.raises(NotImplementedError, match=word):
        EvalPreprocess(33, **kwargs)


def test_out_of_scope_long_edge_and_images(lib):
    with pytest.raises(NotImplementedError, match='long_edge range'):
        EvalPreprocess((30, 40))
    with pytest.raises(AssertionError):
        EvalPreprocess(None)
    EvalPreprocess(None, tight_padding=True)
    pp = EvalPreprocess(33)
    for bad in (np.zeros((8, 8), np.uint8), np.zeros((8, 8, 4), np.uint8),
                np.zeros((8, 8, 3), np.float32), np.zeros((8, 8, 1), np.uint8),
                torch.zeros((8, 8, 3), dtype=torch.int16)):
        with pytest.raises(NotImplementedError, match='3-channel uint8'):
            pp.batch_cpu([bad])


def test_rescaled_size_follows_the_reference():
    assert preprocess.rescaled_size(43, 47, 98) == (89, 98)    # int(43 * (98 / 47))
    assert preprocess.rescaled_size(85, 30, 17) == (17, 6)
    assert preprocess.rescaled_size(480, 640, 641) == (480, 641)
    # Python float arithmetic, not integer arithmetic: 7 * (122 / 14) is 60.99999999999999
    assert 7 * 122 // 14 == 61
    assert preprocess.rescaled_size(7, 14, 122) == (60, 122)
    assert preprocess.rescaled_size(14, 7, 122) == (122, 60)


# ---- argument checks --------------------------------------------------------------------
def _call(lib, device, *, n=1, dtype=0, layout=0, src=True, descs=True, out=True, mean=True,
          std=(0.229, 0.224, 0.225), fill=True, tables=True, src_bytes=None, out_elems=None,
          **desc):
    """One 4x5 -> 8x10 image padded to 12x12; device=True calls pp_preprocess_images with
    dummy device pointers (every refusal comes before anything touches them)."""
    d = np.zeros(1, _abi.IMAGE_DESC_DTYPE)
    d[0] = (0, 0, 4, 5, 8, 10, 1, 2, 12, 12)
    for k, v in desc.items():
        d[k] = v
    s = np.zeros(4 * 5 * 3, np.uint8)
    o = np.zeros(3 * 12 * 12, np.float32)
    m = np.float32(preprocess.MEAN)
    sd = np.asarray(std, np.float32)
    f = np.uint8(preprocess.FILL)
    vp = lambda a, on: a.ctypes.data_as(ctypes.c_void_p) if on else None
    dev = lambda on: ctypes.c_void_p(256) if on else None
    head = [dev(src) if device else vp(s, src), s.size if src_bytes is None else src_bytes,
            vp(d, descs), n, dev(out) if device else vp(o, out),
            o.size if out_elems is None else out_elems, dtype, layout, vp(m, mean), vp(sd, True),
            vp(f, fill)]
    if device:
        return lib.pp_preprocess_images(*head, dev(tables), 1 << 20, None)
    return lib.pp_preprocess_images_cpu(*head)


BAD_ARGS = [
    ('h=1', dict(h=1), PP_ESHAPE, 'edge < 2'),
    ('w=1', dict(w=1), PP_ESHAPE, 'edge < 2'),
    ('th=1', dict(th=1), PP_ESHAPE, 'edge < 2'),
    ('tw=0', dict(tw=0), PP_ESHAPE, 'edge < 2'),
    ('left too large', dict(left=3), PP_ESHAPE, 'does not fit'),
    ('top too large', dict(top=5), PP_ESHAPE, 'does not fit'),
    ('left<0', dict(left=-1), PP_ESHAPE, 'does not fit'),
    ('H too small', dict(H=9), PP_ESHAPE, 'does not fit'),
    ('H=0', dict(H=0), PP_ESHAPE, 'output size'),
    ('W=-3', dict(W=-3), PP_ESHAPE, 'output size'),
    ('out region beyond buffer', dict(out_offset=1), PP_ESHAPE, 'beyond the output buffer'),
    ('out buffer short', dict(out_elems=3 * 12 * 12 - 1), PP_ESHAPE, 'beyond the output buffer'),
    ('src beyond buffer', dict(src_offset=1), PP_ESHAPE, 'beyond the source buffer'),
    ('n_img=-1', dict(n=-1), PP_ESHAPE, 'n_img'),
    ('dtype=4', dict(dtype=4), PP_EINVAL, 'unknown dtype'),
    ('dtype=-1', dict(dtype=-1), PP_EINVAL, 'unknown dtype'),
    ('layout=2', dict(layout=2), PP_EINVAL, 'unknown layout'),
    ('std 0', dict(std=(0.229, 0.0, 0.225)), PP_EINVAL, 'std'),
    ('std inf', dict(std=(np.inf, 0.224, 0.225)), PP_EINVAL, 'std'),
    ('std nan', dict(std=(0.229, 0.224, np.nan)), PP_EINVAL, 'std'),
    ('NULL src', dict(src=False), PP_EINVAL, 'NULL'),
    ('NULL descs', dict(descs=False), PP_EINVAL, 'NULL'),
    ('NULL out', dict(out=False), PP_EINVAL, 'NULL'),
    ('NULL mean', dict(mean=False), PP_EINVAL, 'NULL'),
    ('NULL fill', dict(fill=False), PP_EINVAL, 'NULL'),
]
# pp_last_error() of every row as the library gave it before both entries shared one host
# layer, after the entry's name and ': ' (recorded from that build, not from this one)
_EDGE = 'a source or target edge < 2'
_FIT = 'the target does not fit its output with this pad'
_REGION = 'an output region beyond the output buffer'
_STD = 'std must be finite and not 0'
BAD_ARGS_TEXT = {
    'h=1': _EDGE, 'w=1': _EDGE, 'th=1': _EDGE, 'tw=0': _EDGE,
    'left too large': _FIT, 'top too large': _FIT, 'left<0': _FIT, 'H too small': _FIT,
    'H=0': 'output size out of range', 'W=-3': 'output size out of range',
    'out region beyond buffer': _REGION, 'out buffer short': _REGION,
    'src beyond buffer': 'a source image beyond the source buffer',
    'n_img=-1': 'n_img < 0',
    'dtype=4': 'unknown dtype', 'dtype=-1': 'unknown dtype', 'layout=2': 'unknown layout',
    'std 0': _STD, 'std inf': _STD, 'std nan': _STD,
    'NULL src': 'NULL argument', 'NULL descs': 'NULL argument', 'NULL out': 'NULL argument',
    'NULL mean': 'NULL argument', 'NULL fill': 'NULL argument',
}


@pytest.mark.parametrize('device', [False, True], ids=['cpu', 'device'])
@pytest.mark.parametrize('case', BAD_ARGS, ids=[c[0] for c in BAD_ARGS])
def test_bad_arguments(lib, case, device):
    name, kwargs, code, word = case
    assert _call(lib, device, **kwargs) == code
    assert word in lib.pp_last_error().decode()
    entry = 'pp_preprocess_images' if device else 'pp_preprocess_images_cpu'
    assert lib.pp_last_error().decode() == '{}: {}'.format(entry, BAD_ARGS_TEXT[name])


def test_null_tables_and_empty_batch(lib):
    assert _call(lib, True, tables=False) == PP_EINVAL  # refused without a launch
    assert _call(lib, False) == PP_OK
    for device in (False, True):  # n_img == 0 succeeds whatever the pointers are
        assert _call(lib, device, n=0, src=False, descs=False, out=False, mean=False,
                     fill=False, tables=False) == PP_OK
    pp = EvalPreprocess(33, tight_padding=True)
    assert pp.batch_cpu([]) == ([], [])
    assert EvalPreprocess(33).batch_cpu([])[0].shape == (0, 3, 33, 33)


# ---- scipy ------------------------------------------------------------------------------
def test_twin_equals_scipy_zoom(lib):
    """200 seeded (h, w, long_edge) with edges in [2, 90]: the rescaled region of the twin's
    uint8 output is scipy.ndimage.zoom(order=1) byte for byte (ties and edges included)."""
    ndimage = pytest.importorskip('scipy.ndimage')
    import warnings
    rng = np.random.default_rng(7)
    done = black = 0
    while done < 200:
        h, w, long_edge = (int(v) for v in rng.integers(2, 91, 3))
        try:
            th, tw = preprocess.rescaled_size(h, w, long_edge)
        except AssertionError:
            continue  # the reference's own assertion: scipy's output size would differ
        if th < 2 or tw < 2:
            continue
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            want = ndimage.zoom(im, (th / h, tw / w, 1), order=1)
        (got,), _ = EvalPreprocess(long_edge, tight_padding=True, dtype=torch.uint8).batch_cpu([im])
        plan = preprocess._Plan(h, w, long_edge, True)
        left, top = plan.ltrb[:2]
        assert got.shape == (plan.H, plan.W, 3)
        region = got[top:top + th, left:left + tw]
        assert region.shape == want.shape
        assert np.array_equal(region, want), (h, w, long_edge)
        outside = np.ones(got.shape[:2], bool)
        outside[top:top + th, left:left + tw] = False
        assert (got[outside] == np.uint8(preprocess.FILL)).all()
        black += int((want[-1] == 0).all() or (want[:, -1] == 0).all())
        done += 1
    assert black > 0  # the sweep met the zero last row / column
