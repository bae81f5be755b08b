"""Shared by tests/test_ragged_multi_cpu.py and tests/test_gpu_ragged_multi.py: the images of
different pixel sizes a ragged multi-scale batch is made of, every head at its own field
size, their own-size decodes by the oracle (computed once per configuration and never
modified), and the zero-padded decodes the CPU guard compares them with."""
import functools

import numpy as np

from openpifpaf_amd import constants, synthetic
from openpifpaf_amd._abi import EVAL_CONFIG, PREDICT_CONFIG, make_config

SKEL = constants.COCO_PERSON_SKELETON
# stride-8 heads of 13-24 x 13-30 cells in a 24x30 container, stride-16 heads of 7-12 x 7-15
# cells in a 12x15 one; 105 and 121 are not 1 mod 16, so there the coarse head's own reach
# ((h - 1) * 16 + 1) is shorter than the stride-8 map
PIXELS = [(97, 129), (129, 97), (97, 233), (105, 105), (161, 121), (185, 233)]
# the planted configurations; 'coarse' puts the stride-16 head first, so the map is that
# head's and cells of the fine head lie beyond it
PLANTED = ('ms2', 'ms10', 'coarse')
CONFIGS = PLANTED + ('dense',)
MODES = ('eval', 'predict')


def config(mode, **kw):
    return make_config(**dict(EVAL_CONFIG if mode == 'eval' else PREDICT_CONFIG, **kw))


def _kwargs(strides, mins, dmin, dmax):
    n = len(strides)
    return dict(cif_indices=[2 * i for i in range(n)], caf_indices=[2 * i + 1 for i in range(n)],
                cif_strides=list(strides), caf_strides=list(strides), cif_min_scales=list(mins),
                caf_min_distances=list(dmin), caf_max_distances=list(dmax))


@functools.lru_cache(maxsize=None)
def field_config_kwargs(name):
    if name in synthetic.MULTI_CASES:
        return _kwargs(*synthetic.MULTI_CASES[name])
    if name == 'coarse':
        return _kwargs([16, 8], [12.0, 0.0], [36.0, 0.0], [None, 160.0])
    assert name == 'dense'
    return _kwargs([8, 16], [0.0, 0.0], [0.0, 0.0], [None, None])


@functools.lru_cache(maxsize=None)
def image(name, h_px, w_px, seed):
    """The head list [cif_0, caf_0, cif_1, caf_1, ...] of one image, read-only."""
    if name in synthetic.MULTI_CASES:
        fields, _ = synthetic.multi_case(name, seed, h_px, w_px, n_people=3)
    elif name == 'coarse':
        fields = [f for pair in synthetic.planted_multi(h_px, w_px, [16, 8], n_people=3, seed=seed)
                  for f in pair]
    else:
        fields = []
        for si, stride in enumerate((8, 16)):
            h, w = (h_px - 1) // stride + 1, (w_px - 1) // stride + 1
            fields += list(synthetic.uniform(h, w, seed=seed * 2 + si))
    for f in fields:
        f.setflags(write=False)
    return tuple(fields)


def images(name, pixels_seeds):
    return [image(name, h, w, seed) for (h, w), seed in pixels_seeds]


_OWN = {}


def own_decode(name, h_px, w_px, seed, cfg_key, cfg):
    """The image decoded alone by the oracle, every head at its own size: what a ragged
    decode must give for it.  `cfg_key` names `cfg` in the cache."""
    import oracle
    key = (name, h_px, w_px, seed, cfg_key)
    if key not in _OWN:
        members = oracle.Members(list(image(name, h_px, w_px, seed)), **field_config_kwargs(name))
        recs = oracle.decode_multi(members, SKEL, cfg)
        recs.setflags(write=False)
        _OWN[key] = recs
    return _OWN[key]


def padded(fields_list):
    """Per head, the images' fields stacked after zero-padding to the head's largest size."""
    out = []
    for m in range(len(fields_list[0])):
        heads = [f[m] for f in fields_list]
        h, w = max(a.shape[2] for a in heads), max(a.shape[3] for a in heads)
        block = np.zeros((len(heads),) + heads[0].shape[:2] + (h, w), np.float32)
        for i, a in enumerate(heads):
            block[i, :, :, :a.shape[2], :a.shape[3]] = a
        out.append(block)
    return out


def padded_decode(name, pixels_seeds, cfg):
    """Every image decoded by the oracle after zero-padding each head to its container."""
    import oracle
    blocks = padded(images(name, pixels_seeds))
    return [oracle.decode_multi(oracle.Members([b[i] for b in blocks],
                                               **field_config_kwargs(name)), SKEL, cfg)
            for i in range(len(pixels_seeds))]
