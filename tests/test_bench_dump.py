"""bench.py --dump-outputs: dump_outputs writes a step's records as float arrays, the same
arrays for full (pp_ann) and compact (pp_pack_compact) records of the same annotations, and
a fixed sample when they pass the size limit.  Host only: the records come from the C++
twin of the decode (stages_cpu.decode_batch)."""
import os

import numpy as np
import pytest

import bench
from openpifpaf_amd import constants, stages_cpu, synthetic
from openpifpaf_amd._abi import EVAL_CONFIG, PACK_ALL, make_config, packed_dtype

FIELDS = ('offsets', 'data', 'joint_scales', 'score', 'image', 'n_decoding', 'n_frontier',
          'decoding_pairs', 'decoding_xyv', 'frontier_pairs')


@pytest.fixture(scope='module')
def records():
    skel = constants.COCO_PERSON_SKELETON
    cif, caf = synthetic.batch('planted', 3, 40, 40, first_seed=7, skeleton=skel, n_people=4)
    recs, offsets = stages_cpu.decode_batch(cif, caf, skel, make_config(**EVAL_CONFIG),
                                            n_threads=2)
    assert len(recs) >= 6
    return recs, offsets


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def _compact(recs, k, c):
    """The compact form of full records (include/pifpaf_amd.h, pp_pack_compact)."""
    out = np.zeros(len(recs), packed_dtype(k, c, PACK_ALL))
    for name in ('score', 'image', 'n_decoding', 'n_frontier'):
        out[name] = recs[name]
    out['data'] = recs['data'][:, :k]
    out['joint_scales'] = recs['joint_scales'][:, :k]
    out['decoding_pairs'] = recs['decoding_pairs'][:, :k]
    out['frontier_pairs'] = recs['frontier_pairs'][:, :out.dtype['frontier_pairs'].shape[0]]
    xyv = recs['decoding_xyv'][:, :k]
    out['decoding_v'] = xyv[:, :, [2, 5]]
    for r in range(len(recs)):
        for i in range(recs['n_decoding'][r]):
            a, b = recs['decoding_pairs'][r, i]
            out['decoding_xy'][r, a] = xyv[r, i, 0:2]
            out['decoding_xy'][r, b] = xyv[r, i, 3:5]
    return out


def test_dump_full_records(records, tmp_path):
    recs, offsets = records
    bench.dump_outputs(str(tmp_path), recs, offsets)
    got = _load(str(tmp_path))
    assert sorted(got) == sorted(FIELDS)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    np.testing.assert_array_equal(got['offsets'], offsets)
    np.testing.assert_array_equal(got['data'], recs['data'][:, :17])
    np.testing.assert_array_equal(got['score'], recs['score'])
    np.testing.assert_array_equal(got['image'], recs['image'])
    for r in range(len(recs)):
        nd, nf = recs['n_decoding'][r], recs['n_frontier'][r]
        np.testing.assert_array_equal(got['decoding_xyv'][r, :nd], recs['decoding_xyv'][r, :nd])
        np.testing.assert_array_equal(got['decoding_pairs'][r, :nd],
                                      recs['decoding_pairs'][r, :nd])
        np.testing.assert_array_equal(got['frontier_pairs'][r, :nf],
                                      recs['frontier_pairs'][r, :nf])
        assert not got['decoding_xyv'][r, nd:].any() and not got['frontier_pairs'][r, nf:].any()


def test_dump_compact_equals_full(records, tmp_path):
    recs, offsets = records
    bench.dump_outputs(str(tmp_path / 'full'), recs, offsets)
    bench.dump_outputs(str(tmp_path / 'compact'), _compact(recs, 17, 19), offsets)
    full, compact = _load(str(tmp_path / 'full')), _load(str(tmp_path / 'compact'))
    assert sorted(full) == sorted(compact)
    for name, arr in full.items():
        if name == 'frontier_pairs':  # the compact record holds min(88, 4 C) frontier slots
            arr = arr[:, :compact[name].shape[1]]
        np.testing.assert_array_equal(compact[name], arr, err_msg=name)


def test_dump_sample_is_fixed_and_bounded(records, tmp_path):
    recs, offsets = records
    limit = 8192
    for sub in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / sub), recs, offsets, limit=limit)
    a, b = _load(str(tmp_path / 'a')), _load(str(tmp_path / 'b'))
    assert sum(os.path.getsize(str(tmp_path / 'a' / f)) for f in os.listdir(str(tmp_path / 'a'))) <= limit
    rows = a['rows'].astype(np.int64)
    assert 0 < len(rows) < len(recs) and (np.diff(rows) > 0).all()
    np.testing.assert_array_equal(a['data'], recs['data'][rows, :17])
    np.testing.assert_array_equal(a['offsets'], offsets)
    for name in a:
        np.testing.assert_array_equal(a[name], b[name])
