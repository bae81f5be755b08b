"""The in-place inverse (pp_annotations_inverse / pp_dets_inverse, csrc/inverse.hip over
csrc/inverse.hpp) on whole batches of synthetic records: the reference's fixture
(tests/golden/inverse.npz) tiled over a grid of more than one block, odd inputs against
oracle.annotations_inverse, and the COCO record kernels (which share inverse.hpp) against the
in-place result.  No decode is run; all comparisons are by bytes."""
import os

import numpy as np
import pytest

import golden_util as gu
import oracle
from openpifpaf_amd import _abi, eval_coco, transforms
from openpifpaf_amd._abi import ANN_DTYPE, DET_DTYPE
from test_oracle_golden import inverse_metas

pytestmark = pytest.mark.gpu

CAP = 300
NAMES = ('shift', 'flip', 'rot')
COUNTS = (0, 257, 300)  # two blocks of 256 in x, the second partial


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


@pytest.fixture(scope='module')
def g():
    with np.load(os.path.join(gu.GOLDEN, 'inverse.npz'), allow_pickle=False) as z:
        return {key: z[key] for key in z.files}


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        return torch.from_numpy(a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))).cuda()
    return torch.from_numpy(a).cuda()


def _host(t, dtype):
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype=dtype).reshape(t.shape[:2]).copy()


def _meta_block(metas):
    return np.concatenate([transforms.meta_record(m) for m in metas])


def _inverse(torch, recs, counts, metas, k=17, hswap=None, det=False):
    """(records after one in-place call, NaN flags or None)"""
    d = _dev(torch, recs)
    flags = transforms.inverse_records(
        d, _dev(torch, np.asarray(counts, np.int32)), _dev(torch, _meta_block(metas)).reshape(-1),
        k=k, hswap=None if hswap is None else _dev(torch, np.asarray(hswap, np.int32)), det=det)
    torch.cuda.synchronize()
    return _host(d, recs.dtype), None if flags is None else flags.cpu().numpy().tolist()


# ---- poses: the reference's fixture, tiled ----------------------------------------------------
@pytest.fixture(scope='module')
def pose_case(torch, g):
    """The fixture's 8 poses tiled record-wise over 3 images x 300 slots (every slot filled,
    those at and above the count too), one in-place call: (before, after, flags, metas, hswap)"""
    src = np.arange(CAP) % len(g['pose_data'])
    nd = g['pose_dxyv'].shape[1]
    recs = np.zeros((len(COUNTS), CAP), ANN_DTYPE)
    recs['data'][:, :, :17] = g['pose_data'][src]
    recs['joint_scales'][:, :, :17] = g['pose_scales'][src]
    recs['decoding_xyv'][:, :, :nd] = g['pose_dxyv'][src]
    recs['decoding_pairs'][:, :, :nd] = g['pose_dpairs'][src]
    recs['n_decoding'] = g['pose_nd'][src]
    recs['n_keypoints'] = 17
    recs['score'] = 0.25 + 0.001 * np.arange(CAP)
    recs['image'] = np.arange(len(COUNTS))[:, None]
    metas = [inverse_metas()[name] for name in NAMES]
    hswap = transforms.swap_table(metas[1]['horizontal_swap'], 17)
    after, flags = _inverse(torch, recs, COUNTS, metas, hswap=hswap)
    return recs, after, flags, metas, hswap


def test_pose_batch_equals_fixture(g, pose_case):
    before, after, flags, _, _ = pose_case
    src = np.arange(CAP) % len(g['pose_data'])
    nd = g['pose_dxyv'].shape[1]
    want = before.copy()
    for i, (name, count) in enumerate(zip(NAMES, COUNTS)):
        want['data'][i, :count, :17] = g[name + '_pose_data'][src[:count]]
        want['joint_scales'][i, :count, :17] = g[name + '_pose_scales'][src[:count]]
        want['decoding_xyv'][i, :count, :nd] = g[name + '_pose_dxyv'][src[:count]]
    assert flags == [0, 0, 0]
    for i, count in enumerate(COUNTS):
        for key in ('data', 'joint_scales', 'decoding_xyv'):
            assert after[key][i, :count].tobytes() == want[key][i, :count].tobytes(), (i, key)
        assert after[i, count:].tobytes() == before[i, count:].tobytes(), i  # untouched
    assert after.tobytes() == want.tobytes()  # and every other field of the kept records
    assert after[1, :257].tobytes() != before[1, :257].tobytes()


# ---- odd inputs against the oracle ------------------------------------------------------------
ODD_COUNTS = (1, 257, 400, 0)  # 400: clamped to the capacity


def _odd_case(k):
    rng = np.random.default_rng(1000 + k)
    n = len(ODD_COUNTS)
    recs = np.zeros((n, CAP), ANN_DTYPE)
    recs['data'][:, :, :k, :2] = rng.uniform(-50, 600, (n, CAP, k, 2)).astype(np.float32)
    recs['data'][:, :, :k, 2] = rng.choice([0.0, 0.004, 0.3, 1.0], (n, CAP, k)).astype(np.float32)
    recs['joint_scales'][:, :, :k] = rng.uniform(0, 8, (n, CAP, k)).astype(np.float32)
    recs['decoding_xyv'] = rng.uniform(-50, 600, recs['decoding_xyv'].shape).astype(np.float32)
    recs['n_decoding'] = np.array([0, k - 1, 30])[np.arange(CAP) % 3]  # 30: PP_MAX_KP rows
    recs['n_keypoints'] = k
    recs['score'] = rng.random((n, CAP))
    recs['data'][1, 256, 2, 0] = np.nan  # the last record of image 1 that is looked at
    named = inverse_metas()
    metas = [named['shift'], named['flip'], named['flip'], named['rot']]
    perm = np.arange(k, dtype=np.int32)
    perm[[0, 1, k - 2, k - 1]] = [1, 0, k - 1, k - 2]
    # not a permutation: sources k - 2 and k - 1 both write row k - 2 (the last one wins),
    # nobody writes row k - 1 (it comes out zero)
    drop = np.arange(k, dtype=np.int32)
    drop[[0, 1, k - 1]] = [1, 0, k - 2]
    return recs, metas, perm, drop


@pytest.mark.parametrize('k', [5, 24])
def test_odd_inputs_equal_oracle(torch, k):
    """One swap table serves a call, so the batch goes through twice: image 1 is the flip
    with the permutation in the first call, image 2 the flip with the table that is not one
    in the second; both flipped images are compared in both."""
    recs, metas, perm, drop = _odd_case(k)
    assert sorted(perm) == list(range(k)) and sorted(set(drop)) != list(range(k))
    for table in (perm, drop):
        after, flags = _inverse(torch, recs, ODD_COUNTS, metas, k=k, hswap=table)
        assert flags == [0, 1, 0, 0]
        want = recs.copy()
        for i, count in enumerate(ODD_COUNTS):
            c = min(count, CAP)
            data, scales, dxyv = oracle.annotations_inverse(
                recs['data'][i, :c, :k], recs['joint_scales'][i, :c, :k],
                recs['decoding_xyv'][i, :c], recs['n_decoding'][i, :c], metas[i], table)
            want['data'][i, :c, :k] = data
            want['joint_scales'][i, :c, :k] = scales
            want['decoding_xyv'][i, :c] = dxyv
        nan_rec = after[1, 256]
        for key in ('data', 'joint_scales', 'decoding_xyv'):
            assert np.array_equal(nan_rec[key], want[key][1, 256], equal_nan=True), key
        assert np.isnan(nan_rec['data']).sum() == 1
        after[1, 256] = want[1, 256]  # every other record by bytes, untouched ones included
        assert after.tobytes() == want.tobytes()
        if table is drop:
            assert not after['data'][2, :, k - 1].any()  # the row nobody writes
            assert after['data'][1, :256, k - 2].any()


# ---- detections -------------------------------------------------------------------------------
def test_det_batch_equals_fixture(torch, g):
    src = np.arange(CAP) % len(g['det_bbox'])
    recs = np.zeros((len(COUNTS), CAP), DET_DTYPE)
    recs['field'], recs['score'] = g['det_field'][src], g['det_score'][src]
    recs['bbox'] = g['det_bbox'][src]
    recs['image'] = np.arange(len(COUNTS))[:, None]
    metas = [inverse_metas()[name] for name in NAMES]
    after, _ = _inverse(torch, recs, COUNTS, metas, det=True)
    want = recs.copy()
    for i, (name, count) in enumerate(zip(NAMES, COUNTS)):
        want['bbox'][i, :count] = g[name + '_det_bbox'][src[:count]]
    for i, count in enumerate(COUNTS):
        assert after['bbox'][i, :count].tobytes() == want['bbox'][i, :count].tobytes(), i
        assert after[i, count:].tobytes() == recs[i, count:].tobytes(), i
    for key in ('field', 'score', 'image', 'pad_'):
        assert after[key].tobytes() == recs[key].tobytes(), key
    assert after.tobytes() == want.tobytes()


# ---- one source, two users --------------------------------------------------------------------
def test_coco_keypoints_round_the_in_place_result(torch, pose_case):
    before, after, _, metas, hswap = pose_case
    ids = np.arange(40, 40 + len(COUNTS), dtype=np.int64)
    got = eval_coco.coco_records(
        _dev(torch, before), _dev(torch, np.asarray(COUNTS, np.int32)),
        _dev(torch, _meta_block(metas)).reshape(-1), _dev(torch, ids),
        k=17, hswap=_dev(torch, hswap), small_threshold=0.0, max_per_image=CAP)
    assert np.diff(got.offsets).tolist() == [1, 257, 300]  # image 0: its dummy record
    assert got.flags.tolist() == [_abi.PP_COCO_EMPTY, 0, 0]
    for i, count in enumerate(COUNTS):
        kp = got.records['keypoints'][got.offsets[i]:got.offsets[i] + count, :, 0:2]
        xy = after['data'][i, :count, :17, 0:2].astype(np.float64)
        assert kp.tobytes() == (np.rint(xy * 100.0) / 100.0).tobytes(), i
