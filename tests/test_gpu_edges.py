"""Batched connection_value / p2p_value on the device (csrc/edges.hip): pp_connection_values
and pp_p2p_values through openpifpaf_amd.functional and through CifCaf.connection_value,
p2p_value, connection_values and p2p_values, against the reference's own results in
tests/golden/edges.npz (bit patterns, any NaN matching any NaN) and against the host twins.
The column sets are this package's device CafScored of the same synthetic fields (pinned to
the reference by the decode fixtures)."""
import ctypes
import functools

import numpy as np
import pytest

import edges_util as eu
from openpifpaf_amd import _edges, constants, functional, functional_cpu
from openpifpaf_amd import decoder as dec
from openpifpaf_amd._abi import EDGE_QUERY_DTYPE
from openpifpaf_amd._lib import call
from openpifpaf_amd.annotation import Annotation

pytestmark = pytest.mark.gpu


def src4(q):
    return np.stack([q['x'], q['y'], q['v'], q['s']], axis=1)


def tgt3(q):
    return np.stack([q['tx'], q['ty'], q['ts']], axis=1)


@functools.lru_cache(maxsize=None)
def device_caf_scored(name):
    """CafScored of the case's fields, filled once on the device at 0.1."""
    import torch
    cif, caf = (torch.from_numpy(f).cuda() for f in eu.case_fields(name))
    fc = dec.FieldConfig()
    hr = dec.CifHr(fc).fill([cif, caf]).accumulated
    cs = dec.CafScored(hr, fc, eu.SKELETON).fill([cif, caf])
    assert cs.packed is not None and cs.packed.n_sets == 2 * len(eu.SKELETON)
    return cs


def decoder_of(g):
    d = dec.CifCaf(dec.FieldConfig(), keypoints=constants.COCO_KEYPOINTS, skeleton=eu.SKELETON)
    d.connection_method = str(g['connection_method'])
    d.keypoint_threshold = float(g['keypoint_threshold'])
    return d


def annotations(g):
    out = []
    for data, scales in zip(g['ann_data'], g['ann_joint_scales']):
        a = Annotation(constants.COCO_KEYPOINTS, eu.SKELETON)
        a.data[:] = data
        a.joint_scales[:] = scales
        out.append(a)
    return out


@pytest.mark.parametrize('name', eu.CASES)
def test_device_entries_match_reference(name):
    g = eu.case(name)
    sets = device_caf_scored(name).packed
    q = eu.connection_queries(g)
    for rm in (True, False):
        got = functional.connection_values(
            sets, src4(q), q['set'], connection_method=str(g['connection_method']),
            keypoint_threshold=float(g['keypoint_threshold']), reverse_match=rm)
        eu.same_bits(got.reshape(g['conn_rm%d' % rm].shape), g['conn_rm%d' % rm])
    q = eu.p2p_queries(g)
    got = functional.p2p_values(sets, src4(q), tgt3(q), q['set'])
    eu.same_bits(got.reshape(g['p2p'].shape), g['p2p'])


@pytest.mark.parametrize('name', eu.CASES)
def test_batched_members_match_reference(name):
    g = eu.case(name)
    d, anns, cs = decoder_of(g), annotations(g), device_caf_scored(name)
    for rm in (True, False):
        eu.same_bits(d.connection_values(anns, cs, reverse_match=rm), g['conn_rm%d' % rm])
    eu.same_bits(dec.CifCaf.p2p_values(anns, anns, cs, eu.SKELETON), g['p2p'])


@pytest.mark.parametrize('name', eu.CASES)
def test_single_calls_match_reference_and_batched(name):
    """connection_value / p2p_value one call at a time, with the reference's return
    conventions, element-wise identical to the batched forms: every connection query of the
    case, and p2p against every target (three annotations) or one target per query."""
    g = eu.case(name)
    d, anns, cs = decoder_of(g), annotations(g), device_caf_scored(name)
    batched = {rm: d.connection_values(anns, cs, reverse_match=rm) for rm in (True, False)}
    p2p = dec.CifCaf.p2p_values(anns, anns, cs, eu.SKELETON)
    n = 0
    for a, ann in enumerate(anns):
        for ci, (j1, j2) in enumerate(eu.SKELETON_M1):
            for dr, (start, end) in enumerate(((j1, j2), (j2, j1))):
                n += 1
                for rm in (True, False):
                    r = d.connection_value(ann, cs, start, end, reverse_match=rm)
                    assert len(r) == 4
                    if not any(r):
                        assert all(isinstance(v, float) for v in r)
                    else:
                        assert all(isinstance(v, np.float32) for v in r)
                    eu.same_bits(np.array(r, np.float32), g['conn_rm%d' % rm][a, 2 * ci + dr])
                    eu.same_bits(np.array(r, np.float32), batched[rm][a, 2 * ci + dr])
                for t in (range(len(anns)) if len(anns) <= 3 else [(a + n) % len(anns)]):
                    tg = anns[t]
                    v = dec.CifCaf.p2p_value(
                        ann.data[start], cs, ann.joint_scales[start],
                        (tg.data[end, 0], tg.data[end, 1], tg.joint_scales[end],
                         tg.data[end, 2]), ci, dr == 0)
                    assert isinstance(v, np.float32) or (isinstance(v, float) and v == 0.0)
                    eu.same_bits(np.float32(v), g['p2p'][a, t, ci, dr])
                    eu.same_bits(np.float32(v), p2p[a, t, ci, dr])


@pytest.mark.parametrize('n_q', [1, 4, 5])
def test_query_counts(n_q):
    """A workgroup with idle waves (1, 5 = 4 + 1) and a full one; the full tables of
    test_device_entries_match_reference run many workgroups."""
    g = eu.case('p40_s0_predict')
    sets = device_caf_scored('p40_s0_predict').packed
    q = eu.connection_queries(g)[40:40 + n_q]  # start joints that are set
    got = functional.connection_values(sets, src4(q), q['set'], keypoint_threshold=0.001)
    eu.same_bits(got, g['conn_rm1'].reshape(-1, 4)[40:40 + n_q])
    assert got.any()
    q = eu.p2p_queries(g)[:n_q]
    got = functional.p2p_values(sets, src4(q), tgt3(q), q['set'])
    eu.same_bits(got, g['p2p'].reshape(-1)[:n_q])


def test_no_queries_on_device():
    sets = device_caf_scored('u10_s0_eval').packed
    assert functional.connection_values(sets, np.zeros((0, 4), np.float32), []).shape == (0, 4)
    r = functional.p2p_values(sets, np.zeros((0, 4), np.float32), np.zeros((0, 3), np.float32),
                              [], device=True)
    assert tuple(r.shape) == (0,)


@pytest.mark.parametrize('n', [0, 1, 2, 63, 64, 65])
def test_edge_sets_and_row_pitch(n):
    """Sets of 0 .. 65 columns (under, at and over one wave's stride), once packed tightly and
    once with a row pitch larger than the count and NaN in the columns past it."""
    import torch
    g = eu.golden()
    src, tgt, sets = eu.edge_queries()
    tight = _edges.pack_sets(eu.edge_sets(n))
    cols = np.full((2, 9, n + 7), np.nan, np.float32)
    cols[:, :, :n] = tight.cols[:, :, :n]
    wide = _edges.PackedSets(torch.from_numpy(cols).cuda(), torch.from_numpy(tight.counts).cuda())
    for packed in (eu.edge_sets(n), wide):
        for rm in (True, False):
            got = functional.connection_values(
                packed, src, sets, keypoint_threshold=float(g['edge_keypoint_threshold']),
                reverse_match=rm)
            eu.same_bits(got, g['edge_conn_rm%d_n%d' % (rm, n)])
        eu.same_bits(functional.p2p_values(packed, src, tgt, sets), g['edge_p2p_n%d' % n])


def test_p2p_corners_on_device():
    g = eu.golden()
    got = functional.p2p_values(eu.edge_sets(65), g['corner_sources'], g['corner_targets'],
                                np.ones(len(g['corner_sources']), np.int32))
    eu.same_bits(got, g['corner_p2p'])
    assert np.isnan(got[3]) and got[4] == 0.0


def test_set_index_out_of_range_reads_as_empty():
    """The device entry cannot refuse a table in device memory: an index outside
    [0, n_sets) is an empty set (the Python API checks host tables before the launch)."""
    import torch
    from openpifpaf_amd import _device
    p = _edges.pack_sets(eu.edge_sets(65), _device.require())
    src, tgt, _ = eu.edge_queries()
    q = _edges.queries(src[:3], [-1, 2, 2 ** 30], tgt[:3])
    qd = torch.from_numpy(q.view(np.uint8)).cuda()
    out = torch.full((3, 4), 7.0, dtype=torch.float32, device='cuda')
    call('pp_connection_values', _device.ptr(p.cols), ctypes.c_int64(9 * p.cap),
         ctypes.c_int64(p.cap), _device.ptr(p.counts), 2, _device.ptr(qd), ctypes.c_int64(3), 0,
         ctypes.c_float(0.0), 1, _device.ptr(out), _device.stream())
    assert not out.cpu().numpy().any()
    out1 = torch.full((3,), 7.0, dtype=torch.float32, device='cuda')
    call('pp_p2p_values', _device.ptr(p.cols), ctypes.c_int64(9 * p.cap), ctypes.c_int64(p.cap),
         _device.ptr(p.counts), 2, _device.ptr(qd), ctypes.c_int64(3), 0, _device.ptr(out1),
         _device.stream())
    assert not out1.cpu().numpy().any()
    assert q.dtype == EDGE_QUERY_DTYPE


def test_caf_scored_over_two_fills_is_repacked():
    """A CafScored concatenated over two fill_caf calls keeps no packed buffer; the batched
    members repack its lists and agree with the host twins over the same columns."""
    import torch
    name = 'u10_s0_eval'
    g = eu.case(name)
    cif, caf = (torch.from_numpy(f).cuda() for f in eu.case_fields(name))
    fc = dec.FieldConfig()
    hr = dec.CifHr(fc).fill([cif, caf]).accumulated
    cs = dec.CafScored(hr, fc, eu.SKELETON).fill_caf(caf, 8)
    assert cs.packed is not None
    cs.fill_caf(caf, 8)  # every column twice: equal scores meet the blend's tie rule
    assert cs.packed is None
    one = device_caf_scored(name)
    assert all(a.shape[1] == 2 * b.shape[1] for a, b in zip(cs.forward, one.forward))
    assert sum(a.shape[1] for a in cs.forward) > 0
    d, anns = decoder_of(g), annotations(g)
    host = _edges.caf_scored_sets(cs, len(eu.SKELETON))
    q = eu.connection_queries(g)
    want = functional_cpu.connection_values(host, src4(q), q['set'])
    eu.same_bits(d.connection_values(anns, cs).reshape(-1, 4), want)
    q = eu.p2p_queries(g)
    want = functional_cpu.p2p_values(host, src4(q), tgt3(q), q['set'])
    eu.same_bits(dec.CifCaf.p2p_values(anns, anns, cs, eu.SKELETON).reshape(-1), want)


def test_host_backed_caf_scored():
    """NumPy fields give a host-backed CafScored; the members upload its lists."""
    name = 'u10_s0_eval'
    g = eu.case(name)
    cif, caf = eu.case_fields(name)
    fc = dec.FieldConfig()
    hr = dec.CifHr(fc).fill([cif, caf]).accumulated
    cs = dec.CafScored(hr, fc, eu.SKELETON).fill([cif, caf])
    assert isinstance(cs.forward[0], np.ndarray) and cs.packed is None
    d, anns = decoder_of(g), annotations(g)
    eu.same_bits(d.connection_values(anns, cs), g['conn_rm1'])
    eu.same_bits(dec.CifCaf.p2p_values(anns, anns, cs, eu.SKELETON), g['p2p'])
    r = d.connection_value(anns[0], cs, 5, 7)
    eu.same_bits(np.array(r, np.float32), g['conn_rm1'][0, 2 * d.by_source[5][7][0]])


def test_device_result_stays_on_device():
    import torch
    name = 'p40_s0_predict'
    g = eu.case(name)
    d, anns, cs = decoder_of(g), annotations(g), device_caf_scored(name)
    t = d.connection_values(anns, cs, device=True)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32
    eu.same_bits(t.cpu().numpy(), d.connection_values(anns, cs))
    t = dec.CifCaf.p2p_values(anns, anns, cs, eu.SKELETON, device=True)
    assert isinstance(t, torch.Tensor) and t.is_cuda
    eu.same_bits(t.cpu().numpy(), g['p2p'])


def test_device_and_host_twin_byte_identical():
    """The full planted case, both entries: the kernel and its host twin over the same packed
    sets give the same bytes."""
    name = 'p40_s0_predict'
    g = eu.case(name)
    sets = device_caf_scored(name).packed
    host = _edges.pack_sets(sets)
    q = eu.connection_queries(g)
    for rm in (True, False):
        for method in ('blend', 'max'):
            kw = dict(connection_method=method, keypoint_threshold=0.001, reverse_match=rm)
            a = functional.connection_values(sets, src4(q), q['set'], **kw)
            b = functional_cpu.connection_values(host, src4(q), q['set'], **kw)
            assert a.tobytes() == b.tobytes()
    q = eu.p2p_queries(g)
    for exp_mode in ('numpy_simd', 'correct'):
        a = functional.p2p_values(sets, src4(q), tgt3(q), q['set'], exp_mode=exp_mode)
        b = functional_cpu.p2p_values(host, src4(q), tgt3(q), q['set'], exp_mode=exp_mode)
        assert not np.isnan(a).any() and a.tobytes() == b.tobytes()
