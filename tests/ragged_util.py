"""Shared by tests/test_ragged_cpu.py and tests/test_gpu_ragged.py: the small images of
different field sizes a ragged batch is made of, their own-size decodes by the host twin
(computed once per configuration and never modified), and the record comparison."""
import functools

import numpy as np

from openpifpaf_amd import constants, stages_cpu, synthetic
from openpifpaf_amd._abi import ANN_DTYPE, EVAL_CONFIG, PREDICT_CONFIG, make_config

# five sizes whose right or bottom edge lies inside the 24x30 container, and the container
SHAPES = [(13, 17), (17, 13), (13, 30), (14, 14), (21, 16), (24, 30)]
CONTAINER = (24, 30)
SEEDS = range(6)
# what the oracle's records hold (it does not set `image` or the record's padding)
ORACLE_KEYS = ('data', 'joint_scales', 'score', 'n_decoding', 'decoding_pairs', 'decoding_xyv',
               'n_frontier', 'frontier_pairs')
# generator, decoder defaults; uniform fields in predict defaults decode to nothing here
CASES = [('planted', 'eval'), ('uniform', 'eval'), ('planted', 'predict')]

SKELETONS = {'coco': constants.COCO_PERSON_SKELETON, 'dense': constants.DENSE_DECODE_SKELETON}


def config(mode, **kw):
    return make_config(**dict(EVAL_CONFIG if mode == 'eval' else PREDICT_CONFIG, **kw))


@functools.lru_cache(maxsize=None)
def image(kind, h, w, seed, skeleton='coco'):
    """(cif (17, 5, h, w), caf (C, 9, h, w)) of one image, read-only."""
    skel = SKELETONS[skeleton]
    if kind == 'planted':
        cif, caf = synthetic.generate('planted', h, w, seed, skeleton=skel, n_people=3)
    else:
        cif, caf = synthetic.generate('uniform', h, w, seed, n_caf=len(skel))
    cif.setflags(write=False)
    caf.setflags(write=False)
    return cif, caf


def images(kind, shapes_seeds, skeleton='coco'):
    return [image(kind, h, w, seed, skeleton) for (h, w), seed in shapes_seeds]


_OWN = {}


def own_decode(kind, h, w, seed, cfg_key, cfg, skeleton='coco'):
    """The image decoded alone at its own size by the host twin (stages_cpu.decode_batch):
    what a ragged decode must give for it.  `cfg_key` names `cfg` in the cache."""
    key = (kind, h, w, seed, cfg_key, skeleton)
    if key not in _OWN:
        cif, caf = image(kind, h, w, seed, skeleton)
        recs, _ = stages_cpu.decode_batch(cif[None], caf[None], SKELETONS[skeleton], cfg,
                                          n_threads=1)
        recs.setflags(write=False)
        _OWN[key] = recs
    return _OWN[key]


def assert_same_records(got, want, image_index, keys=None):
    """Field by field, bit for bit; `image` is the record's position in the ragged batch."""
    assert len(got) == len(want), (image_index, len(got), len(want))
    for name in keys or ANN_DTYPE.names:
        if name == 'image':
            assert (got[name] == image_index).all(), image_index
        else:
            assert got[name].tobytes() == want[name].tobytes(), (image_index, name)


def padded(fields):
    """The fields stacked after zero-padding to the largest size (NumPy)."""
    return stages_cpu.pad_container(list(fields))[0]
