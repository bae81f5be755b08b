"""The frontier's slot count per lane (csrc/grow_frontier.hpp) on an MI355X: one slot when the
skeleton has at most 64 directed edges, two above.

The launchers pick the kernel instance by the number of directed edges nd, so the cases sit
on both sides of the switch with K = 24: 32 distinct pairs (nd = 64, the last lane of the
one-slot form in use), the same with a self-loop added (nd = 65: a self-loop is one directed
edge) and 33 distinct pairs (nd = 66), then COCO (nd = 38) and the dense COCO skeleton
(nd = 88).  A single image runs seed_loop_ext_kernel and complete_kernel, a batch of 136 the
one-CU seed_loop_kernel.  Every record is compared byte for byte with the host twin that ships
in the library (pp_decode_batch_cpu).
"""
import numpy as np
import pytest

import kc_util as kc

pytestmark = pytest.mark.gpu

_PAIRS = kc.CASES['k24c64'][1]
SKELETONS = {
    'nd64': (_PAIRS[:32], 64),
    'nd65': (_PAIRS[:32] + [(12, 12)], 65),
    'nd66': (_PAIRS[:33], 66),
}
K = 24


def directed_edges(skeleton):
    """nd as the launchers count it (by_source, cifcaf.py:62-65): distinct (start, end)."""
    return len({(a, b) for a, b in skeleton} | {(b, a) for a, b in skeleton})


def _device(cif, caf, skeleton, cfg):
    import torch
    from openpifpaf_amd import engine
    recs, offsets, _ = engine.DecodeEngine().decode(
        torch.from_numpy(cif).cuda(), torch.from_numpy(caf).cuda(), skeleton, cfg)
    return recs.copy(), np.array(offsets)


def _same(got, want, where):
    assert len(got) == len(want), (where, len(got), len(want))
    for key in got.dtype.names:  # every field of the record (not the padding between them)
        assert got[key].tobytes() == want[key].tobytes(), (where, key)


def _inputs(name, gen):
    skeleton = SKELETONS[name][0]
    if gen == 'uniform':
        return kc.uniform_kc(K, len(skeleton), 20, 23, 0)
    return kc.planted_kc(K, skeleton, *kc.PLANTED_SIZE, seed=kc.PLANTED_SEED)


@pytest.mark.parametrize('name', list(SKELETONS))
def test_skeletons_have_the_directed_edges_they_are_named_for(name):
    skeleton, nd = SKELETONS[name]
    assert directed_edges(skeleton) == nd
    assert len(skeleton) <= 64 and max(max(e) for e in skeleton) <= K


@pytest.mark.parametrize('gen', ['uniform', 'planted'])
@pytest.mark.parametrize('name', list(SKELETONS))
def test_single_image_vs_twin(name, gen):
    from openpifpaf_amd import stages_cpu
    skeleton = SKELETONS[name][0]
    cif, caf = _inputs(name, gen)
    cfg = kc.config('eval')
    want, want_off = stages_cpu.decode_batch(cif[None], caf[None], skeleton, cfg)
    got, off = _device(cif[None], caf[None], skeleton, cfg)
    assert np.array_equal(off, want_off)
    _same(got, want, (name, gen))
    assert len(got) >= 3


@pytest.mark.parametrize('name', list(SKELETONS))
def test_batch_vs_twin(name):
    """136 images (four distinct planted ones, repeated): no external helper workgroups, so
    the one-CU seed_loop_kernel runs."""
    from openpifpaf_amd import stages_cpu
    skeleton = SKELETONS[name][0]
    four = [kc.planted_kc(K, skeleton, *kc.PLANTED_SIZE, seed=s) for s in range(4)]
    cif4, caf4 = np.stack([f[0] for f in four]), np.stack([f[1] for f in four])
    cfg = kc.config('eval')
    want, want_off = stages_cpu.decode_batch(cif4, caf4, skeleton, cfg)
    n = 136
    got, off = _device(np.tile(cif4, (n // 4, 1, 1, 1, 1)), np.tile(caf4, (n // 4, 1, 1, 1, 1)),
                       skeleton, cfg)
    assert len(off) == n + 1
    for i in range(n):
        g = got[off[i]:off[i + 1]].copy()
        assert (g['image'] == i).all()
        g['image'] = i % 4
        _same(g, want[want_off[i % 4]:want_off[i % 4 + 1]], (name, i))
    assert off[-1] >= 3 * n


@pytest.mark.parametrize('which', ['coco', 'dense'])
def test_coco_and_dense_vs_twin(which):
    from openpifpaf_amd import constants, stages_cpu, synthetic
    skeleton = (constants.COCO_PERSON_SKELETON if which == 'coco'
                else constants.DENSE_DECODE_SKELETON)
    assert directed_edges(skeleton) == (38 if which == 'coco' else 88)
    cif, caf = synthetic.planted(*kc.PLANTED_SIZE, n_people=4, seed=0, skeleton=skeleton)
    cfg = kc.config('eval')
    want, want_off = stages_cpu.decode_batch(cif[None], caf[None], skeleton, cfg)
    got, off = _device(cif[None], caf[None], skeleton, cfg)
    assert np.array_equal(off, want_off)
    _same(got, want, which)
    assert len(got) >= 3
