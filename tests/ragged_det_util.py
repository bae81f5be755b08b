"""Shared by tests/test_ragged_det_cpu.py and tests/test_gpu_ragged_det.py: the small CifDet
images of different field sizes a ragged detection batch is made of, and their own-size
results by the C oracle (computed once per configuration and never modified)."""
import functools

import numpy as np

import oracle
import ragged_util as ru
from openpifpaf_amd import synthetic
from openpifpaf_amd._abi import make_config

K = 3
CIF_THRESHOLD = 0.1
SEED_THRESHOLD = {'uniform': 0.1, 'planted': 0.3}
SHAPES, CONTAINER = ru.SHAPES, ru.CONTAINER
# the smallest extents: own occupancy grids of zero rows or columns (H' = 1: int(1 / 2) = 0)
# beside a container whose grid has some, images of two or three cells beside full ones
SMALL = [(1, 1), (1, 6), (2, 7), (3, 4), (5, 5)]


def config(kind=None, seed_threshold=None):
    th = SEED_THRESHOLD[kind] if seed_threshold is None else seed_threshold
    return make_config(cif_threshold=CIF_THRESHOLD, seed_threshold=th)


@functools.lru_cache(maxsize=None)
def image(kind, h, w, seed, k=K):
    """(k, 7, h, w) CifDet fields of one image, read-only."""
    if kind == 'planted':
        det = synthetic.det_planted(h, w, n_categories=k, n_objects=4, seed=seed)
    else:
        det = synthetic.det_uniform(h, w, n_categories=k, seed=seed)
    det.setflags(write=False)
    return det


@functools.lru_cache(maxsize=None)
def own_decode(kind, h, w, seed, k=K, seed_threshold=None, instance_threshold=None):
    """oracle.cifdet_decode of the image alone at its own size (`instance_threshold`:
    nms.Detection's, default 0.1)."""
    nms = oracle.det_nms_defaults()
    if instance_threshold is not None:
        nms.instance_threshold = instance_threshold
    recs = oracle.cifdet_decode(image(kind, h, w, seed, k), config(kind, seed_threshold), nms)
    recs.setflags(write=False)
    return recs


@functools.lru_cache(maxsize=None)
def own_hr(kind, h, w, seed, k=K):
    """oracle.cifdet_hr of the image alone at its own size: (k, H', W')."""
    hr = oracle.cifdet_hr(image(kind, h, w, seed, k), config(kind))
    hr.setflags(write=False)
    return hr


def padded(det, shape=CONTAINER):
    """The image zero-padded on the right and bottom to `shape`."""
    out = np.zeros(det.shape[:2] + tuple(shape), np.float32)
    out[:, :, :det.shape[2], :det.shape[3]] = det
    return out


def assert_same_records(got, want, image_index):
    """field, score and bbox bit for bit; `image` is the record's position in the batch."""
    assert len(got) == len(want), (image_index, len(got), len(want))
    for name in ('field', 'score', 'bbox'):
        assert got[name].tobytes() == want[name].tobytes(), (image_index, name)
    assert (got['image'] == image_index).all(), image_index
