"""Shared by tests/test_preprocess_cpu.py and tests/test_gpu_preprocess.py: the cases of
tests/golden/preprocess.npz (the reference's eval preprocessing chain, gen_preprocess.py)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'preprocess.npz')
META_KEYS = ('offset', 'scale', 'valid_area', 'width_height')
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_cache = {}


class Case:
    def __init__(self, fx, pre):
        self.name = pre
        self.src = fx[pre + 'src']
        self.long_edge = int(fx[pre + 'long_edge']) or None
        self.tight = bool(fx[pre + 'tight'])
        self.u8 = fx[pre + 'u8']
        self.f32 = fx[pre + 'f32']
        self.meta = {k: fx[pre + k] for k in META_KEYS}

    @property
    def mode(self):
        return self.long_edge, self.tight


def load():
    """(fixture arrays, list of Case); read once and never modified."""
    if not _cache:
        fx = dict(np.load(GOLDEN))
        for v in fx.values():
            v.setflags(write=False)
        _cache['fx'] = fx
        _cache['cases'] = [Case(fx, str(p)) for p in fx['names']]
    return _cache['fx'], _cache['cases']


def groups(cases):
    """Cases that one EvalPreprocess object serves: {(long_edge, tight): [Case]}."""
    out = {}
    for c in cases:
        out.setdefault(c.mode, []).append(c)
    return out


def bits(a):
    """Bit patterns of a float tensor / array (torch tensor on any device, or NumPy array; a
    NumPy uint16 array holds bfloat16 bits already)."""
    if isinstance(a, np.ndarray):
        if a.dtype == np.uint16:
            return a.astype(np.int64)
        a = torch.from_numpy(np.ascontiguousarray(a))
    a = a.detach().cpu().contiguous()
    view = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16,
            torch.uint8: torch.uint8}[a.dtype]
    return a.view(view).numpy().astype(np.int64) & (0xffffffff if a.dtype == torch.float32
                                                    else 0xffff)


def expected(case, dtype):
    """The fixture's (1, 3, H, W) tensor as `dtype`: the reference tensor's .to(dtype)."""
    return torch.from_numpy(case.f32.copy())[None].to(dtype)


def check_meta(meta, case):
    for k in META_KEYS:
        got = np.asarray(meta[k])
        if k != 'width_height':
            assert got.dtype == np.float64, k
        assert np.array_equal(got.astype(np.float64), case.meta[k].astype(np.float64)), k
    assert meta['hflip'] is False
    assert meta['rotation'] == {'angle': 0.0, 'width': None, 'height': None}


def one(result, i, tight, dtype):
    """Image i of a batch result as a (1, 3, H, W) array, or (H, W, 3) for uint8 results."""
    return result[i] if tight or dtype == torch.uint8 else result[i:i + 1]
