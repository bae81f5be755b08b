"""Shared by tests/test_coco_cpu.py and tests/test_gpu_coco.py: the reference fixture
(tests/golden/coco_records.npz, written by tests/golden/gen_coco.py) as record batches,
EvalCoco.from_predictions restated on NumPy records, and synthetic record batches."""
import json
import math
import os

import numpy as np

from openpifpaf_amd._abi import ANN_DTYPE, DET_DTYPE
from openpifpaf_amd.transforms import META_DTYPE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CAPS = (20, 3, 1)


def dumps(preds):
    """The fixture's text form: json.dumps without spaces after the separators."""
    return json.dumps(preds, separators=(',', ':'))


def load_fixture():
    with np.load(os.path.join(GOLDEN, 'coco_records.npz'), allow_pickle=False) as z:
        return {key: z[key] for key in z.files}


def metas_of(fx, prefix):
    n = len(fx[prefix + 'hflip'])
    m = np.zeros(n, META_DTYPE)
    for key in ('offset', 'scale', 'rotation_angle', 'rotation_width', 'rotation_height',
                'width', 'hflip'):
        m[key] = fx[prefix + key]
    return m, fx[prefix + 'image_id'].astype(np.int64)


def pose_batch(fx, tag):
    """(recs (n_img, cap) ANN_DTYPE, counts, metas, image_ids, hswap, K) of a fixture group."""
    k = int(fx[tag + '_K'])
    src = fx[tag + '_img_src']
    data, scales, score = (fx[tag + '_src_' + n] for n in ('data', 'scales', 'score'))
    n, cap = len(src), data.shape[1]
    recs = np.zeros((n, cap), ANN_DTYPE)
    recs['data'][:, :, :k] = data[src]
    recs['joint_scales'][:, :, :k] = scales[src]
    recs['score'] = score[src]
    recs['n_keypoints'] = k
    recs['image'] = np.arange(n)[:, None]
    counts = fx[tag + '_src_counts'][src].astype(np.int32)
    metas, ids = metas_of(fx, tag + '_meta_')
    return recs, counts, metas, ids, fx[tag + '_hswap'].astype(np.int32), k


def det_batch(fx):
    """The det_* records of inverse.npz under the fixture's detection metas."""
    with np.load(os.path.join(GOLDEN, 'inverse.npz'), allow_pickle=False) as z:
        field, score, bbox = z['det_field'], z['det_score'], z['det_bbox']
    counts = fx['det_counts'].astype(np.int32)
    recs = np.zeros((len(counts), max(1, len(field))), DET_DTYPE)
    recs['field'], recs['score'], recs['bbox'] = field, score, bbox
    metas, ids = metas_of(fx, 'det_meta_')
    return recs, counts, metas, ids


def param_sets(fx, tag):
    """(fixture key, small_threshold, max_per_image) of every stored parameter set."""
    return [('%s_json_t%d_m%d' % (tag, ti, cap), th, cap)
            for ti, th in enumerate((0.0, float(fx[tag + '_small_threshold']))) for cap in CAPS]


# ---------------------------------------------------------------------------------------
# from_predictions (eval_coco.py:108-158) restated on NumPy records, step by step as
# openpifpaf_amd.eval_coco.coco_predictions runs it on Annotation objects
# ---------------------------------------------------------------------------------------
def inverse_numpy(data, scales, meta, hswap):
    """Preprocess.annotations_inverse (preprocess.py:35-82) on one record's arrays."""
    data, scales = data.copy(), scales.copy()
    angle = -float(meta['rotation_angle'])
    if angle != 0.0:
        rw, rh = float(meta['rotation_width']), float(meta['rotation_height'])
        c, s = math.cos(angle / 180.0 * math.pi), math.sin(angle / 180.0 * math.pi)
        x_old = data[:, 0].copy() - (rw - 1) / 2
        y_old = data[:, 1].copy() - (rh - 1) / 2
        data[:, 0] = (rw - 1) / 2 + c * x_old + s * y_old
        data[:, 1] = (rh - 1) / 2 - s * x_old + c * y_old
    data[:, 0] += meta['offset'][0]
    data[:, 1] += meta['offset'][1]
    data[:, 0] = data[:, 0] / meta['scale'][0]
    data[:, 1] = data[:, 1] / meta['scale'][1]
    nan = bool(np.any(np.isnan(data)))
    scales = (scales / meta['scale'][0]).astype(np.float32)
    if meta['hflip']:
        data[:, 0] = -data[:, 0] + (np.int64(meta['width']) - 1)
        if hswap is not None:
            target = np.zeros(data.shape)
            for si, ti in enumerate(hswap):
                target[ti] = data[si]
            data = target.astype(np.float32)
    return data, scales, nan


def scale_numpy(data, v_th=0.01):
    m = data[:, 2] > v_th
    if not np.any(m):
        return 0.0
    return max(np.max(data[m, 0]) - np.min(data[m, 0]), np.max(data[m, 1]) - np.min(data[m, 1]))


def json_numpy(data, scales, score, category_id, image_id):
    v_mask = data[:, 2] > 0.0
    keypoints = np.copy(data)
    keypoints[v_mask, 2] = np.maximum(0.01, keypoints[v_mask, 2])
    keypoints = np.around(keypoints.astype(np.float64), 2)
    if np.any(v_mask):
        x = np.min(data[:, 0][v_mask] - scales[v_mask])
        y = np.min(data[:, 1][v_mask] - scales[v_mask])
        bbox = [x, y, np.max(data[:, 0][v_mask] + scales[v_mask]) - x,
                np.max(data[:, 1][v_mask] + scales[v_mask]) - y]
    else:
        bbox = [0, 0, 0, 0]
    return {'keypoints': keypoints.reshape(-1).tolist(),
            'bbox': [round(float(c), 2) for c in bbox],
            'score': max(0.001, round(np.float64(score), 3)),
            'category_id': category_id, 'image_id': image_id}


def predictions_numpy(recs, counts, metas, ids, hswap, k, small_threshold=0.0, max_per_image=20,
                      category_id=1):
    """(predictions, per-image NaN flags)"""
    out, nans = [], []
    for i in range(len(counts)):
        inv = [inverse_numpy(r['data'][:k], r['joint_scales'][:k], metas[i], hswap) + (r['score'],)
               for r in recs[i, :min(int(counts[i]), recs.shape[1])]]
        nans.append(any(t[2] for t in inv))
        if small_threshold:
            inv = [t for t in inv if scale_numpy(t[0]) >= small_threshold]
        inv = inv[:max_per_image]
        image = [json_numpy(d, s, sc, category_id, int(ids[i])) for d, s, _, sc in inv]
        if not image:
            image.append({'image_id': int(ids[i]), 'category_id': 1,
                          'keypoints': np.zeros((k * 3,)).tolist(), 'bbox': [0, 0, 1, 1],
                          'score': 0.001})
        out += image
    return out, np.array(nans)


# ---------------------------------------------------------------------------------------
# synthetic batches
# ---------------------------------------------------------------------------------------
def random_metas(rng, n):
    m = np.zeros(n, META_DTYPE)
    m['offset'] = rng.uniform(-20, 20, (n, 2)).round(2)
    m['scale'] = rng.uniform(0.4, 1.6, (n, 2)).round(3)
    rot = rng.random(n) < 0.4
    m['rotation_angle'] = np.where(rot, rng.uniform(-30, 30, n).round(1), 0.0)
    m['rotation_width'] = np.where(rot, 481.0, 0.0)
    m['rotation_height'] = np.where(rot, 361.0, 0.0)
    m['width'] = rng.integers(300, 700, n)
    m['hflip'] = rng.random(n) < 0.5
    return m


def random_swap(rng, k):
    """A row permutation made of disjoint transpositions, as hflip tables are."""
    table = np.arange(k, dtype=np.int32)
    p = rng.permutation(k)
    for a, b in zip(p[0:k - 1:2], p[1:k:2]):
        if rng.random() < 0.7:
            table[a], table[b] = b, a
    return table


def random_poses(rng, n_img, cap, k, counts):
    """Poses of widely varying extent, with v = 0, v below and above 0.01, and tied scores."""
    recs = np.zeros((n_img, cap), ANN_DTYPE)
    centre = rng.uniform(20, 400, (n_img, cap, 1, 2))
    extent = rng.choice([0.5, 3.0, 12.0, 40.0, 120.0], (n_img, cap, 1, 1))
    xy = centre + rng.uniform(-1, 1, (n_img, cap, k, 2)) * extent
    v = rng.choice([0.0, 0.004, 0.0100001, 0.3, 0.9, 1.0], (n_img, cap, k)) * \
        rng.choice([1.0, 1.0, 0.5], (n_img, cap, k))
    recs['data'][:, :, :k, :2] = xy.astype(np.float32)
    recs['data'][:, :, :k, 2] = v.astype(np.float32)
    recs['joint_scales'][:, :, :k] = rng.uniform(0, 6, (n_img, cap, k)).astype(np.float32)
    recs['score'] = rng.choice(np.round(rng.random(16), 3), (n_img, cap)) * \
        rng.choice([1.0, 0.99999, 0.5], (n_img, cap))
    recs['n_keypoints'] = k
    recs['image'] = np.arange(n_img)[:, None]
    return recs, np.asarray(counts, np.int32)


def split_threshold(recs, counts, metas, hswap, k):
    """A small_threshold between the scales of each image's records where possible: the
    median of every record's scale after the inverse."""
    vals = [scale_numpy(inverse_numpy(r['data'][:k], r['joint_scales'][:k], metas[i], hswap)[0])
            for i in range(len(counts)) for r in recs[i, :min(int(counts[i]), recs.shape[1])]]
    vals = [float(v) for v in vals if v > 0]
    return float(np.median(vals)) if vals else 1.0
