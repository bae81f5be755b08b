"""Shared by tests/test_preprocess_views_cpu.py and tests/test_gpu_preprocess_views.py: the
cases of tests/golden/preprocess_views.npz (the reference's eval preprocessing with extended
scale and turns, and ShellMultiScale's input pyramid; gen_preprocess_views.py)."""
import os

import numpy as np
import torch

import preprocess_util as pu
from openpifpaf_amd.transforms import EvalViews

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                      'preprocess_views.npz')
META_KEYS = pu.META_KEYS
ALL_DTYPES = pu.DTYPES + (torch.uint8,)
_cache = {}


class Case:
    """One image through one mode: what the reference made of it."""

    def __init__(self, name, src, long_edge, tight=False, ext=False, ori=False, ms=False,
                 image_id=None, u8=None, f32=None, views=None, meta=None):
        self.name, self.src, self.long_edge = name, src, int(long_edge)
        self.tight, self.ext, self.ori, self.ms = bool(tight), bool(ext), bool(ori), bool(ms)
        self.image_id = None if image_id is None else int(image_id)
        self.u8, self.f32, self.views, self.meta = u8, f32, views, meta

    @property
    def mode(self):
        return self.long_edge, self.tight, self.ext, self.ori, self.ms

    def given_meta(self):
        return None if self.image_id is None else {'image_id': self.image_id}


def _meta(fx, pre, row=None):
    keys = META_KEYS + ('rotation',)
    return {k: fx[pre + k] if row is None else fx[pre + k][row] for k in keys}


def load():
    """(fixture arrays, list of Case); read once and never modified."""
    if _cache:
        return _cache['fx'], _cache['cases']
    fx = dict(np.load(GOLDEN))
    for v in fx.values():
        v.setflags(write=False)
    cases = []
    for pre in (str(p) for p in fx['pyr_names']):
        cases.append(Case(pre, fx[pre + 'src'], fx[pre + 'long_edge'], ms=True,
                          u8=fx[pre + 'u8'], views=[fx[pre + 'v%d' % v] for v in range(10)]))
    u8_at = f32_at = 0
    for i in range(len(fx['turn_long_edge'])):
        edge = int(fx['turn_long_edge'][i])
        shape = tuple(int(v) for v in fx['turn_u8_shape'][i])
        n = shape[0] * shape[1] * 3
        u8 = fx['turn_u8'][u8_at:u8_at + n].reshape(shape)
        u8_at += n
        f32 = None
        if edge == int(fx['turn_f32_edge']):
            f32 = fx['turn_f32'][f32_at:f32_at + n].reshape(3, shape[0], shape[1])
            f32_at += n
        cases.append(Case('t%d_' % i, fx['s%d_src' % edge], edge, fx['turn_tight'][i],
                          fx['turn_ext'][i], fx['turn_ori'][i], False, fx['turn_image_id'][i],
                          u8, f32, None, _meta(fx, 'turn_', i)))
    assert u8_at == fx['turn_u8'].size and f32_at == fx['turn_f32'].size
    cases.append(Case('all_', fx['all_src'], fx['all_long_edge'], False, True, True, True,
                      fx['all_image_id'], fx['all_u8'], None,
                      [fx['all_v%d' % v] for v in range(10)], _meta(fx, 'all_')))
    _cache['fx'], _cache['cases'] = fx, cases
    return fx, cases


def groups(cases):
    """Cases that one EvalViews object serves: {mode: [Case]}."""
    out = {}
    for c in cases:
        out.setdefault(c.mode, []).append(c)
    return out


def make(case_or_mode, dtype=torch.float32, channels_last=False, hflip=True):
    long_edge, tight, ext, ori, ms = getattr(case_or_mode, 'mode', case_or_mode)
    return EvalViews(long_edge, tight_padding=tight, extended_scale=ext,
                     orientation_invariant=ori, multi_scale=ms, multi_scale_hflip=hflip,
                     dtype=dtype, channels_last=channels_last)


def check_meta(meta, case):
    if case.meta is None:  # a pyramid case: EvalPreprocess's metas, checked by its own tests
        return
    for k in META_KEYS:
        got = np.asarray(meta[k])
        if k != 'width_height':
            assert got.dtype == np.float64, k
        assert got.dtype == case.meta[k].dtype, k
        assert np.array_equal(got, case.meta[k]), (case.name, k)
    assert meta['hflip'] is False
    angle, width, height = case.meta['rotation']
    if angle == 0.0:
        assert meta['rotation'] == {'angle': 0.0, 'width': None, 'height': None}, case.name
    else:
        assert meta['rotation'] == {'angle': angle, 'width': width, 'height': height}, case.name
        assert isinstance(meta['rotation']['angle'], int)
    assert meta['image_id'] == case.image_id


def reduce_np(canvas, hflip=True):
    """The 5 or 10 views of a (..., n, n, 3) canvas by the rules of nets.py:116-128 in NumPy
    slicing (axes -3 and -2)."""
    n = canvas.shape[-2]
    keep = np.array([i % 3 != 2 for i in range(n)])
    out = [canvas, canvas[..., keep, :, :][..., keep, :], canvas[..., ::2, ::2, :],
           canvas[..., ::3, ::3, :], canvas[..., ::5, ::5, :]]
    if hflip:
        out += [v[..., ::-1, :] for v in out]
    return out


def as_array(a):
    """A result as a contiguous NumPy array or CPU tensor in its logical (.., 3, n, n) order."""
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().contiguous()
    return np.ascontiguousarray(a)


def is_channels_last(a):
    """(B, 3, h, w) array or tensor whose memory is (B, h, w, 3)."""
    if isinstance(a, torch.Tensor):
        return a.permute(0, 2, 3, 1).is_contiguous()
    return a.transpose(0, 2, 3, 1).flags['C_CONTIGUOUS']


def check_image(case, result, i, dtype, channels_last):
    """Image i of a batch result of case's mode against the fixture, bit for bit: the canvas
    (uint8 results), the float tensor where the fixture holds it, every view of a pyramid."""
    if case.ms:
        assert len(result) == 10
        if dtype == torch.uint8:
            want = reduce_np(case.u8)
            for v in range(10):
                got = as_array(result[v][i])
                got = got.numpy() if isinstance(got, torch.Tensor) else got
                assert got.dtype == np.uint8 and got.shape == want[v].shape, (case.name, v)
                assert np.array_equal(got, want[v]), (case.name, v)
            return
        for v in range(10):
            got = result[v][i:i + 1]
            assert tuple(got.shape) == (1,) + case.views[v].shape, (case.name, v, got.shape)
            if got.shape[2] > 1:  # a 1 x 1 view is contiguous either way
                assert is_channels_last(got) == channels_last, (case.name, v)
            want = torch.from_numpy(case.views[v].copy())[None].to(dtype)
            assert np.array_equal(pu.bits(as_array(got)), pu.bits(want)), (case.name, v, dtype)
        return
    got = pu.one(result, i, case.tight, dtype)
    if dtype == torch.uint8:
        got = as_array(got)
        got = got.numpy() if isinstance(got, torch.Tensor) else got
        assert got.dtype == np.uint8 and got.shape == case.u8.shape, case.name
        assert got.tobytes() == case.u8.tobytes(), case.name
        return
    assert tuple(got.shape) == (1, 3) + case.u8.shape[:2], case.name
    assert is_channels_last(got) == channels_last, case.name
    if case.f32 is not None:
        want = torch.from_numpy(case.f32.copy())[None].to(dtype)
        assert np.array_equal(pu.bits(as_array(got)), pu.bits(want)), (case.name, dtype)
