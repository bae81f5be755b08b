"""Batched connection_value / p2p_value (cifcaf.py:194-245), the host twins
(pp_connection_values_cpu, pp_p2p_values_cpu through openpifpaf_amd.functional_cpu) against
the reference's own results in tests/golden/edges.npz: bit patterns, any NaN matching any
NaN.  The column sets are this package's host CafScored of the same synthetic fields (pinned
to the reference by the decode fixtures)."""
import ctypes
import functools

import numpy as np
import pytest

import edges_util as eu
from openpifpaf_amd import _edges, functional_cpu, stages_cpu
from openpifpaf_amd._abi import EDGE_QUERY_DTYPE, make_config
from openpifpaf_amd._lib import PPError, load


@functools.lru_cache(maxsize=None)
def host_sets(name):
    """The case's 2C column sets, set 2 c backward and 2 c + 1 forward, at 0.1."""
    cif, caf = eu.case_fields(name)
    cfg = make_config()
    hr = stages_cpu.cifhr(cif[None], cfg)
    fwd, bwd = stages_cpu.caf_scored(caf[None], hr, eu.SKELETON, 0.1, cfg)[0]
    return _edges.pack_sets([s for pair in zip(bwd, fwd) for s in pair])


@pytest.mark.parametrize('name', eu.CASES)
@pytest.mark.parametrize('reverse_match', [True, False])
def test_connection_values_match_reference(name, reverse_match):
    g = eu.case(name)
    q = eu.connection_queries(g)
    got = functional_cpu.connection_values(
        host_sets(name), np.stack([q['x'], q['y'], q['v'], q['s']], axis=1), q['set'],
        connection_method=str(g['connection_method']),
        keypoint_threshold=float(g['keypoint_threshold']), reverse_match=reverse_match)
    eu.same_bits(got.reshape(len(g['table']), -1, 4), g['conn_rm%d' % reverse_match])


@pytest.mark.parametrize('name', eu.CASES)
def test_p2p_values_match_reference(name):
    g = eu.case(name)
    q = eu.p2p_queries(g)
    got = functional_cpu.p2p_values(
        host_sets(name), np.stack([q['x'], q['y'], q['v'], q['s']], axis=1),
        np.stack([q['tx'], q['ty'], q['ts']], axis=1), q['set'])
    eu.same_bits(got.reshape(g['p2p'].shape), g['p2p'])


@pytest.mark.parametrize('n', [0, 1, 2, 63, 64, 65])
def test_edge_sets_match_reference(n):
    g = eu.golden()
    assert n in g['edge_ns']
    src, tgt, sets = eu.edge_queries()
    for rm in (True, False):
        got = functional_cpu.connection_values(
            eu.edge_sets(n), src, sets, keypoint_threshold=float(g['edge_keypoint_threshold']),
            reverse_match=rm)
        eu.same_bits(got, g['edge_conn_rm%d_n%d' % (rm, n)])
    got = functional_cpu.p2p_values(eu.edge_sets(n), src, tgt, sets)
    eu.same_bits(got, g['edge_p2p_n%d' % n])
    if n == 0:
        assert not got.any()


def test_p2p_corners_match_reference():
    g = eu.golden()
    got = functional_cpu.p2p_values(eu.edge_sets(65), g['corner_sources'], g['corner_targets'],
                                    np.ones(len(g['corner_sources']), np.int32))
    eu.same_bits(got, g['corner_p2p'])
    by_name = dict(zip([str(s) for s in g['corner_names']], got))
    assert by_name['source_scale_zero'] == 0.0 and by_name['source_scale_negative'] == 0.0
    assert by_name['target_scale_zero_off'] == 0.0
    assert np.isnan(by_name['nan_first_kept'])  # Python's max() keeps a NaN first element
    assert np.isfinite(by_name['nan_later_kept'])  # ... and never takes a later one


def test_reference_conditions():
    """What the fixture must show for the comparisons above to mean something, re-asserted
    from the stored arrays (tests/golden/gen_edges.py asserts the same when it writes them).
    The connection counts are over the edges whose start joint is set."""
    g = eu.golden()
    p40 = eu.case('p40_s0_predict')
    st = eu.start_set(p40)
    nz = p40['conn_rm1'].any(axis=2)
    assert nz[st].sum() >= 0.9 * st.sum()
    assert (p40['p2p'] > 1e-3).sum() >= 100
    u10 = eu.case('u10_s0_eval')
    rm1, rm0 = u10['conn_rm1'].any(axis=2), u10['conn_rm0'].any(axis=2)
    assert (rm0 & ~rm1).sum() >= 10  # results that reverse_match turns to zero
    assert rm1.sum() >= 10
    assert (g['blend_returns'] > 0).all()  # every return of _target_with_blend was taken
    # zeroed by the 0.3 threshold alone: none in the planted image (its reference scores are
    # all above 0.70), the uniform image's weak scores are
    assert g['p31x41_kth_zeroed_by_threshold'] + g['u10_kth_zeroed_by_threshold'] >= 1
    assert float(g['p31x41_kth_keypoint_threshold']) == 0.3
    assert str(g['p40_s3_max_connection_method']) == 'max'
    c = g['corner_p2p']
    assert c[0] == 0 and c[1] == 0 and c[2] == 0 and np.isnan(c[3]) and np.isfinite(c[4])
    assert g['corner_divide_warning'][2]


def test_no_queries():
    sets = eu.edge_sets(65)
    assert functional_cpu.connection_values(sets, np.zeros((0, 4), np.float32), []).shape == (0, 4)
    assert functional_cpu.p2p_values(sets, np.zeros((0, 4), np.float32),
                                     np.zeros((0, 3), np.float32), []).shape == (0,)
    lib = load()  # n_q == 0 is success whatever the pointers
    assert lib.pp_connection_values_cpu(None, 9, 1, None, 0, None, 0, 0, 0.0, 1, None) == 0
    assert lib.pp_p2p_values_cpu(None, 9, 1, None, 0, None, 0, 0, None) == 0
    assert lib.pp_connection_values(None, 9, 1, None, 0, None, 0, 0, 0.0, 1, None, None) == 0
    assert lib.pp_p2p_values(None, 9, 1, None, 0, None, 0, 0, None, None) == 0


def _raw(lib, name, cols, counts, q, out, *, set_stride=None, pitch=None, n_sets=None,
         n_q=None, method=0, reverse_match=1):
    pitch = cols.shape[2] if pitch is None else pitch
    args = [cols.ctypes.data, 9 * cols.shape[2] if set_stride is None else set_stride, pitch,
            counts.ctypes.data, len(counts) if n_sets is None else n_sets, q.ctypes.data,
            len(q) if n_q is None else n_q, method]
    if 'connection' in name:
        args += [ctypes.c_float(0.0), reverse_match]
    args.append(None if out is None else out.ctypes.data)
    if not name.endswith('_cpu'):
        args.append(None)  # stream
    return getattr(lib, name)(*args)


@pytest.mark.parametrize('name', ['pp_connection_values_cpu', 'pp_p2p_values_cpu',
                                  'pp_connection_values', 'pp_p2p_values'])
def test_admission_errors(name):
    """PP_ESHAPE / PP_EINVAL with a message and no launch: the device entries refuse before
    touching the device, so these run without one."""
    lib = load()
    p = _edges.pack_sets(eu.edge_sets(65))
    cols, counts = p.cols, p.counts
    q = np.zeros(3, EDGE_QUERY_DTYPE)
    out = np.zeros((3, 4), np.float32)
    assert _raw(lib, name, cols, counts, q, out, n_q=-1) == -2
    assert _raw(lib, name, cols, counts, q, out, pitch=-1) == -2
    assert _raw(lib, name, cols, counts, q, out, set_stride=9 * cols.shape[2] - 1) == -2
    assert b'bad shape' in lib.pp_last_error()
    assert _raw(lib, name, cols, counts, q, out, n_sets=-1) == -2
    assert _raw(lib, name, cols, counts, q, out, method=4) == -1
    assert b'connection method not known' in lib.pp_last_error()
    assert _raw(lib, name, cols, counts, q, None) == -1
    assert b'NULL argument' in lib.pp_last_error()
    if 'connection' in name:  # the reverse match reads set ^ 1
        assert _raw(lib, name, cols, counts, q, out, n_sets=1) == -2
        assert b'pairs' in lib.pp_last_error()
    if name.endswith('_cpu'):  # a host table's set indices are checked
        q['set'] = [0, 2, 1]
        assert _raw(lib, name, cols, counts, q, out) == -1
        assert b'query 1 names set 2 of 2' in lib.pp_last_error()


def test_python_argument_errors():
    sets = eu.edge_sets(2)
    src = np.zeros((2, 4), np.float32)
    with pytest.raises(ValueError, match='set index'):
        functional_cpu.connection_values(sets, src, [0, 2])
    with pytest.raises(ValueError, match='set indices'):
        functional_cpu.connection_values(sets, src, [0])
    with pytest.raises(ValueError, match=r'\(9, N\)'):
        functional_cpu.connection_values([np.zeros((8, 3), np.float32)] * 2, src, [0, 1])
    with pytest.raises(Exception, match='connection method not known'):
        functional_cpu.connection_values(sets, src, [0, 1], connection_method='mean')
    with pytest.raises(PPError, match='pairs'):
        functional_cpu.connection_values(sets[:1], src, [0, 0])
    # without the reverse match a single set will do
    assert functional_cpu.connection_values(sets[:1], src, [0, 0],
                                            reverse_match=False).shape == (2, 4)
