"""Shared by tests/test_edges_cpu.py and tests/test_gpu_edges.py: tests/golden/edges.npz (the
reference's connection_value / p2p_value, tests/golden/gen_edges.py) and the query tables
that go with its arrays."""
import functools
import os

import numpy as np

import golden_util
from openpifpaf_amd import _edges, constants

CASES = ('p40_s0_predict', 'p40_s3_max', 'u10_s0_eval', 'p31x41_kth', 'u10_kth')
SKELETON = list(constants.COCO_PERSON_SKELETON)
SKELETON_M1 = np.asarray(SKELETON) - 1


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(golden_util.GOLDEN, 'edges.npz'), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def case(name):
    """The keys of one case without their prefix (golden_util.case_inputs reads them)."""
    g = {k[len(name) + 1:]: v for k, v in golden().items() if k.startswith(name + '_')}
    g['table'] = np.concatenate([g['ann_data'], g['ann_joint_scales'][:, :, None]], axis=2)
    return g


@functools.lru_cache(maxsize=None)
def case_fields(name):
    """(cif, caf) of a case, rebuilt from openpifpaf_amd.synthetic and checked by SHA-256."""
    cif, caf, _ = golden_util.case_inputs(case(name))
    return cif, caf


def same_bits(got, ref):
    """Bit patterns equal; any NaN matches any NaN."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nan = np.isnan(got) & np.isnan(ref)
    bad = (got.view(np.uint32) != ref.view(np.uint32)) & ~nan
    assert not bad.any(), '{} of {} differ, first at {}: {!r} != {!r}'.format(
        bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][0], ref[bad][0])


def connection_queries(g):
    """The (n_ann * 2C) queries of conn_rm1 / conn_rm0, in their order."""
    return _edges.connection_queries(g['table'], SKELETON_M1)


def p2p_queries(g):
    """The (n_ann * n_ann * C * 2) queries of p2p, in its order."""
    return _edges.p2p_queries(g['table'], g['table'], SKELETON_M1)


def edge_queries():
    """The queries of the edge_* arrays: sources and targets on set 1 (forward) of the pair
    (edge_bwd, edge_fwd) cut to n columns."""
    g = golden()
    return g['edge_sources'], g['edge_targets'], np.ones(len(g['edge_sources']), np.int32)


def edge_sets(n):
    g = golden()
    return [np.ascontiguousarray(g['edge_bwd'][:, :n]), np.ascontiguousarray(g['edge_fwd'][:, :n])]


def start_set(g):
    """[a, e]: the start joint of directed edge e of annotation a is set (v > 0)."""
    return g['ann_data'][:, SKELETON_M1.reshape(-1), 2] > 0
