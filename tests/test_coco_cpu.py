"""COCO prediction records (EvalCoco.from_predictions, eval_coco.py:108-158): the host twins
pp_coco_keypoints_cpu / pp_coco_dets_cpu against the reference's fixture
(tests/golden/coco_records.npz), against from_predictions restated on NumPy records, and
their rounding against the installed NumPy and Python.  All comparisons are exact.  No GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import coco_util
from openpifpaf_amd import _abi, _lib, eval_coco
from openpifpaf_amd._abi import ANN_DTYPE, PP_COCO_EMPTY, PP_COCO_NAN
from openpifpaf_amd.transforms import META_DTYPE

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


@pytest.fixture(scope='module')
def lib():
    from openpifpaf_amd import build
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope='module')
def fx():
    return coco_util.load_fixture()


# ---- the reference's fixture ------------------------------------------------------------
@pytest.mark.parametrize('tag', ['coco', 'chain5'])
def test_twin_equals_reference(lib, fx, tag):
    recs, counts, metas, ids, hswap, k = coco_util.pose_batch(fx, tag)
    before = recs.tobytes()
    for key, th, cap in coco_util.param_sets(fx, tag):
        got = eval_coco.coco_records_cpu(recs, counts, metas, ids, k=k, hswap=hswap,
                                         small_threshold=th, max_per_image=cap)
        assert coco_util.dumps(got.predictions()) == str(fx[key]), key
        again = eval_coco.coco_records_cpu(recs, counts, metas, ids, k=k, hswap=hswap,
                                           small_threshold=th, max_per_image=cap)
        assert got.records.tobytes() == again.records.tobytes(), key
        assert got.records.dtype.itemsize == lib.pp_coco_record_size(k)
    assert recs.tobytes() == before  # the input records are only read


def test_twin_equals_reference_detections(lib, fx):
    recs, counts, metas, ids = coco_util.det_batch(fx)
    for cap in (20, 1):
        got = eval_coco.coco_records_cpu(recs, counts, metas, ids, det=True, max_per_image=cap)
        assert coco_util.dumps(got.predictions()) == str(fx['det_json_m%d' % cap])
        assert got.flags.tolist() == [0, 0, 0, PP_COCO_EMPTY]


def test_fixture_conditions(lib, fx):
    """What the GPU test needs so as not to pass vacuously, from the reference's output and
    the fixture's inputs alone."""
    recs, counts, metas, ids, hswap, k = coco_util.pose_batch(fx, 'coco')
    assert str(fx['route']) in ('EvalCoco', 'per-annotation')
    n_in = {int(i): int(c) for i, c in zip(ids, counts)}
    th = float(fx['coco_small_threshold'])
    assert th > 0
    per = {}
    for key, _, cap in coco_util.param_sets(fx, 'coco'):
        preds = json.loads(str(fx[key]))
        for i in ids:
            mine = [p for p in preds if p['image_id'] == int(i)]
            dummy = len(mine) == 1 and mine[0]['bbox'] == [0, 0, 1, 1] and mine[0]['score'] == 0.001
            per[key, int(i)] = 0 if dummy else len(mine)
            assert len(mine) >= 1
    full0 = {i: per['coco_json_t0_m20', i] for i in n_in}
    full1 = {i: per['coco_json_t1_m20', i] for i in n_in}
    assert any(0 < full1[i] < min(n_in[i], 20) for i in n_in)    # loses some, not all
    assert any(full1[i] == 0 and n_in[i] > 0 for i in n_in)      # loses all: the dummy
    assert any(n_in[i] > 20 and full0[i] == 20 for i in n_in)    # more survivors than the cap
    assert any(per['coco_json_t1_m1', i] == 1 and full1[i] > 1 for i in n_in)
    assert any(metas['hflip'][j] and counts[j] for j in range(len(ids))) and hswap.tolist() != \
        list(range(k))
    assert any(metas['rotation_angle'][j] != 0 and counts[j] for j in range(len(ids)))
    assert any(n_in[i] == 0 for i in n_in)                         # an image without poses


# ---- from_predictions restated on NumPy records ------------------------------------------
def test_twin_equals_restated_logic(lib):
    rng = np.random.default_rng(11)
    k, n_img, cap = 17, 8, 200
    recs, counts = coco_util.random_poses(rng, n_img, cap, k, [200] * n_img)
    recs['score'][0, :6] = [np.nan, 0.0004, 0.0005, 0.0015, 0.0025, -1.0]
    recs['score'][1, :40] = 0.4375  # ties
    metas = coco_util.random_metas(rng, n_img)
    metas['hflip'][:2] = (1, 0)
    ids = np.arange(500, 500 + n_img, dtype=np.int64)
    hswap = coco_util.random_swap(rng, k)
    th = coco_util.split_threshold(recs, counts, metas, hswap, k)
    for small, cap_ in ((0.0, 20), (th, 20), (th, 200), (th, 1), (1e9, 20), (-1.0, 3)):
        got = eval_coco.coco_records_cpu(recs, counts, metas, ids, k=k, hswap=hswap,
                                         small_threshold=small, max_per_image=cap_,
                                         category_id=3)
        want, nans = coco_util.predictions_numpy(recs, counts, metas, ids, hswap, k, small, cap_, 3)
        assert not nans.any() and not (got.flags & PP_COCO_NAN).any()
        assert coco_util.dumps(got.predictions()) == coco_util.dumps(want), (small, cap_)
    kept = np.diff(eval_coco.coco_records_cpu(recs, counts, metas, ids, k=k, hswap=hswap,
                                              small_threshold=th, max_per_image=200).offsets)
    assert ((kept > 0) & (kept < 200)).all()  # the threshold splits every image
    empty = eval_coco.coco_records_cpu(recs, counts, metas, ids, k=k, hswap=hswap,
                                       small_threshold=1e9)
    assert (empty.flags == PP_COCO_EMPTY).all()


def test_nan_coordinate_flags_the_image(lib):
    rng = np.random.default_rng(12)
    k = 17
    recs, counts = coco_util.random_poses(rng, 3, 30, k, [30, 30, 30])
    recs['data'][1, 25, 4, 1] = np.nan  # beyond the cap: the reference asserts all the same
    metas = coco_util.random_metas(rng, 3)
    got = eval_coco.coco_records_cpu(recs, counts, metas, [1, 2, 3], k=k, max_per_image=20)
    assert (got.flags & PP_COCO_NAN).tolist() == [0, 1, 0]
    _, nans = coco_util.predictions_numpy(recs, counts, metas, [1, 2, 3], None, k)
    assert nans.tolist() == [False, True, False]
    with pytest.raises(AssertionError):
        got.predictions()


# ---- rounding against the installed NumPy and Python --------------------------------------
def _through_twin(values, scores):
    """float32 `values` as coordinates and float64 `scores` through pp_coco_keypoints_cpu
    with the identity meta (offset -0.0: x + -0.0 is x for every x, -0.0 included): (rounded
    coordinates, rounded scores)."""
    k = 24
    per = 2 * k
    n = max(-(-len(values) // per), len(scores), 1)
    vals = np.zeros(n * per, np.float32)
    vals[:len(values)] = values
    recs = np.zeros((1, n), ANN_DTYPE)
    recs['data'][0, :, :, :2] = vals.reshape(n, k, 2)
    recs['score'][0, :len(scores)] = scores
    metas = np.zeros(1, META_DTYPE)
    metas['scale'] = 1.0
    metas['offset'] = -0.0
    got = eval_coco.coco_records_cpu(recs, [n], metas, [1], k=k, max_per_image=n)
    out = got.records['keypoints'][:, :, :2].reshape(-1)[:len(values)]
    return out, got.records['score'][:len(scores)]


def test_rounding_matches_numpy_and_python(lib):
    rng = np.random.default_rng(13)
    ties = (2.0 * np.arange(-20000, 20000) + 1.0) / 8.0
    assert ties.min() < -4999 and ties.max() > 4999
    rand = np.concatenate([
        rng.uniform(-700, 700, 500000), rng.uniform(-1, 1, 250000),
        rng.standard_normal(150000) * 10.0 ** rng.integers(-6, 30, 150000),
        (rng.integers(-500000, 500000, 100000) + 0.5) / 100.0]).astype(np.float32)
    special = np.array([0.0, -0.0, -0.001, 0.001, 1e30, -1e30, 0.005, -0.005, 0.015, 2.675],
                       np.float32)
    values = np.concatenate([ties.astype(np.float32), rand, special])
    assert len(rand) == 1000000
    scores = np.concatenate([rng.random(300000),
                             [0.0, 0.0004999, 0.0005, 0.0015, 0.0025, 1.0, -0.3, 0.9995]])
    got, got_s = _through_twin(values, scores)
    want = np.around(values.astype(np.float64), 2)
    assert got.tobytes() == want.tobytes()  # bytes: -0.0 stays -0.0
    py = np.array([round(float(v), 2) for v in values])
    assert got.tobytes() == py.tobytes()
    at = len(ties) + len(rand)
    assert str(got[at + 1]) == '-0.0' and str(got[at + 2]) == '-0.0' and got[at + 4] == float(np.float32(1e30))
    want_s = np.array([max(0.001, round(np.float64(s), 3)) for s in scores])
    assert got_s.tobytes() == want_s.tobytes()
    # a detection's float32 score: round(float(np.float32), 3)
    dscores = rng.random(50000).astype(np.float32)
    recs = np.zeros((1, len(dscores)), _abi.DET_DTYPE)
    recs['score'][0] = dscores
    metas = np.zeros(1, META_DTYPE)
    metas['scale'] = 1.0
    det = eval_coco.coco_records_cpu(recs, [len(dscores)], metas, [1], det=True,
                                     max_per_image=len(dscores))
    want_d = np.array([max(0.001, round(float(s), 3)) for s in dscores])
    assert det.records['score'].tobytes() == want_d.tobytes()


# ---- ABI ----------------------------------------------------------------------------------
def test_record_sizes_and_dtypes(lib, tmp_path):
    for k in (1, 17, 24):
        assert lib.pp_coco_record_size(k) == 56 + 24 * k == _abi.coco_dtype(k).itemsize
    assert lib.pp_coco_record_size(0) == 0 and lib.pp_coco_record_size(25) == 0
    assert lib.pp_coco_workspace_size(256) >= 4 * 256 and lib.pp_coco_workspace_size(-1) == 0
    import subprocess
    src = tmp_path / 'coco_layout.c'
    src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "pifpaf_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(pp_coco_det), offsetof(pp_coco_det, score),
         offsetof(pp_coco_det, bbox), offsetof(pp_coco_det, category_id), sizeof(pp_coco_params),
         offsetof(pp_coco_params, max_per_image), offsetof(pp_coco_params, category_id));
  return 0;
}
''')
    exe = tmp_path / 'coco_layout'
    subprocess.check_call(['gcc', '-I', os.path.join(REPO, 'include'), str(src), '-o', str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    d, p = _abi.COCO_DET_DTYPE, _abi.CocoParams
    assert vals == [d.itemsize, d.fields['score'][1], d.fields['bbox'][1],
                    d.fields['category_id'][1], ctypes.sizeof(p), p.max_per_image.offset,
                    p.category_id.offset]
    pose = _abi.coco_dtype(17)
    assert [pose.fields[n][1] for n in d.names[:4]] == [d.fields[n][1] for n in d.names[:4]]
    assert pose.fields['n_keypoints'][1] == d.fields['pad_'][1] and pose.fields['keypoints'][1] == 56


def test_symbols_declared_in_header():
    text = open(os.path.join(REPO, 'include', 'pifpaf_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in ('pp_coco_record_size', 'pp_coco_workspace_size', 'pp_coco_keypoints',
                 'pp_coco_dets', 'pp_coco_keypoints_cpu', 'pp_coco_dets_cpu'):
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in _lib.EXPORTED


def test_refusals_without_gpu(lib):
    p = ctypes.byref(_abi.CocoParams(0.0, 20, 1))
    bad_cap = ctypes.byref(_abi.CocoParams(0.0, 0, 1))
    d = ctypes.c_void_p(4096)
    null = ctypes.c_void_p(0)

    def pose(anns=d, counts=d, n=1, cap=8, k=17, metas=d, ids=d, params=p, out=d, out_cap=8,
             oc=d, of=d, ws=d):
        return lib.pp_coco_keypoints(anns, counts, n, cap, k, metas, ids, null, params, out,
                                     out_cap, oc, of, ws, None)

    def det(dets=d, counts=d, n=1, cap=8, metas=d, ids=d, params=p, out=d, out_cap=8, oc=d,
            of=d, ws=d):
        return lib.pp_coco_dets(dets, counts, n, cap, metas, ids, params, out, out_cap, oc, of,
                                ws, None)

    for fn in (pose, det):
        for arg in ('counts', 'metas', 'ids', 'out', 'oc', 'of', 'ws'):
            assert fn(**{arg: null}) == -1, arg
            assert b'NULL' in lib.pp_last_error()
        assert fn(params=None) == -1
        assert fn(params=bad_cap) == -2 and b'max_per_image' in lib.pp_last_error()
        assert fn(n=-1) == -2 and fn(cap=0) == -2 and fn(out_cap=-1) == -2
        assert fn(out=ctypes.c_void_p(4100)) == -1 and b'aligned' in lib.pp_last_error()
        assert fn(n=0) == 0
    assert pose(anns=null) == -1 and det(dets=null) == -1
    assert pose(k=25) == -2 and b'PP_MAX_KP' in lib.pp_last_error()
    assert pose(k=0) == -2
    # the twins refuse the same way
    assert lib.pp_coco_keypoints_cpu(d, d, 1, 8, 25, d, d, null, p, d, 8, d, d) == -2
    assert lib.pp_coco_keypoints_cpu(d, d, 1, 8, 17, d, d, null, bad_cap, d, 8, d, d) == -2
    assert lib.pp_coco_keypoints_cpu(null, d, 1, 8, 17, d, d, null, p, d, 8, d, d) == -1
    assert lib.pp_coco_dets_cpu(d, d, -1, 8, d, d, p, d, 8, d, d) == -2
    assert lib.pp_coco_dets_cpu(d, d, 1, 8, d, d, None, d, 8, d, d) == -1


def test_out_capacity_convention_twin(lib):
    """Records at packed index >= out_capacity are not written; the counts stay complete."""
    rng = np.random.default_rng(14)
    recs, counts = coco_util.random_poses(rng, 3, 10, 5, [4, 0, 7])
    metas = coco_util.random_metas(rng, 3)
    full = eval_coco.coco_records_cpu(recs, counts, metas, [1, 2, 3], k=5)
    assert np.diff(full.offsets).tolist() == [4, 1, 7]
    part = eval_coco.coco_records_cpu(recs, counts, metas, [1, 2, 3], k=5, out_capacity=11)
    assert np.diff(part.offsets).tolist() == [4, 1, 7]
    assert part.records.tobytes() == full.records[:11].tobytes()
