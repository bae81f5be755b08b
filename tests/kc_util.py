"""Keypoint counts and skeletons other than COCO's: the cases, their synthetic inputs and
the fixture loaders shared by tests/test_kc_cpu.py, tests/test_gpu_kc.py and
tests/golden/gen_golden.py (section `kc`).

The decoder is generic in the number of keypoints K <= PP_MAX_KP (24) and of skeleton edges
C <= PP_MAX_EDGES (64).  The skeletons below are literal lists of 1-based pairs, so a case
does not depend on a NumPy stream; check_skeleton() states what every one of them obeys.
"""
import glob
import os

import numpy as np

from openpifpaf_amd import synthetic
from openpifpaf_amd._abi import EVAL_CONFIG, PREDICT_CONFIG, make_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

_K20C33 = [
    # a path over all 20 joints, about half of its edges reversed
    (1, 2), (3, 2), (3, 4), (5, 4), (5, 6), (6, 7), (8, 7), (8, 9), (9, 10), (11, 10),
    (11, 12), (12, 13), (14, 13), (14, 15), (15, 16), (17, 16), (17, 18), (18, 19), (20, 19),
    # 14 chords
    (1, 3), (4, 2), (1, 5), (6, 3), (2, 7), (8, 4), (5, 10), (12, 6), (7, 14), (16, 8),
    (9, 18), (20, 10), (11, 15), (19, 13),
]

_K24C64 = [
    # joints i, i + 1 (23 edges)
    (1, 2), (3, 2), (3, 4), (5, 4), (5, 6), (7, 6), (7, 8), (9, 8), (9, 10), (11, 10),
    (11, 12), (13, 12), (13, 14), (15, 14), (15, 16), (17, 16), (17, 18), (19, 18), (19, 20),
    (21, 20), (21, 22), (23, 22), (23, 24),
    # joints i, i + 2 (22 edges)
    (3, 1), (2, 4), (5, 3), (4, 6), (7, 5), (6, 8), (9, 7), (8, 10), (11, 9), (10, 12),
    (13, 11), (12, 14), (15, 13), (14, 16), (17, 15), (16, 18), (19, 17), (18, 20), (21, 19),
    (20, 22), (23, 21), (22, 24),
    # joints i, i + 5 (19 edges)
    (1, 6), (7, 2), (3, 8), (9, 4), (5, 10), (11, 6), (7, 12), (13, 8), (9, 14), (15, 10),
    (11, 16), (17, 12), (13, 18), (19, 14), (15, 20), (21, 16), (17, 22), (23, 18), (19, 24),
]

# name -> (K, skeleton); what each reaches is listed in DESIGN.md ("envelope")
CASES = {
    'pair2': (2, [(1, 2)]),
    'loop3': (3, [(1, 2), (2, 3), (3, 1)]),
    'iso4': (4, [(1, 2), (3, 1)]),
    'chain5': (5, [(1, 2), (2, 3), (3, 4), (4, 5)]),
    'split6': (6, [(1, 2), (2, 3), (4, 5), (5, 6)]),
    'k8c7': (8, [(1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8)]),
    'k20c33': (20, _K20C33),
    'k24star': (24, [(1, j) for j in range(2, 25)]),
    'k24c64': (24, _K24C64),
}
NAMES = tuple(CASES)
# every joint reachable from every other one
CONNECTED = ('pair2', 'loop3', 'chain5', 'k8c7', 'k20c33', 'k24star', 'k24c64')
VARIANT_CASES = ('k24c64', 'chain5')  # get 'max' and 'greedy' fixtures too

# Skeletons that name an unordered pair more than once, so that by_source overwrites an entry
# in place (cifcaf.py:62-65: the later CAF index and direction at the earlier position).
# Outside NAMES: check_skeleton refuses them and they have no reference fixture; the oracle
# is their reference.
REPEATED = {
    'rep3': (3, [(1, 2), (2, 3), (2, 1), (2, 3)]),
    'rep4': (4, [(1, 2), (2, 3), (3, 4), (2, 1), (1, 2), (4, 3)]),
}

UNIFORM_SIZES = ((12, 15), (20, 23), (31, 34))
PLANTED_SIZE = (33, 40)
PLANTED_OBJECTS = 4
# generator seeds, chosen so that the oracle alone meets the tests' counts (pair2 decodes
# 3 annotations from uniform 20x23 fields of seed 0, 5 from seed 7)
UNIFORM_SEEDS = {'pair2': 7}
PLANTED_SEED = 0

MULTI_PX = (321, 321)
MULTI_OBJECTS = 4


def case(name):
    k, skeleton = CASES[name]
    return k, [tuple(e) for e in skeleton]


def keypoint_names(k):
    return ['kp%d' % (j + 1) for j in range(k)]


def check_skeleton(k, skeleton):
    """No self-loop, no unordered pair twice, indices within 1..K."""
    seen = set()
    for j1, j2 in skeleton:
        assert 1 <= j1 <= k and 1 <= j2 <= k, (j1, j2)
        assert j1 != j2, (j1, j2)
        key = (min(j1, j2), max(j1, j2))
        assert key not in seen, key
        seen.add(key)


def components(k, skeleton):
    """Connected components of the skeleton as sorted lists of 0-based joints."""
    root = list(range(k))

    def find(a):
        while root[a] != a:
            a = root[a]
        return a
    for j1, j2 in skeleton:
        root[find(j1 - 1)] = find(j2 - 1)
    groups = {}
    for j in range(k):
        groups.setdefault(find(j), []).append(j)
    return sorted(groups.values())


# ---- generators ------------------------------------------------------------------------

def uniform_kc(k, c, h, w, seed=0):
    """synthetic.uniform with k CIF fields in place of 17."""
    rng = np.random.default_rng(seed)
    g = synthetic._grid(h, w)
    cif = rng.random((k, 5, h, w), dtype=np.float32)
    cif[:, 0] **= 4
    cif[:, 1:3] += g - 0.5
    cif[:, 4] = 0.5 + 3 * cif[:, 4]
    caf = rng.random((c, 9, h, w), dtype=np.float32)
    caf[:, 0] **= 4
    caf[:, 1:3] += g - 0.5
    caf[:, 5:7] = g + 4 * (caf[:, 5:7] - 0.5)
    caf[:, 4] = 0.5 + 3 * caf[:, 4]
    caf[:, 8] = 0.5 + 3 * caf[:, 8]
    return cif, caf


def uniform_kc_batch(k, c, n, h, w, first_seed=0):
    cifs, cafs = zip(*(uniform_kc(k, c, h, w, first_seed + i) for i in range(n)))
    return np.stack(cifs), np.stack(cafs)


def template(k):
    """Fixed joint offsets (k, 2) of an object in pose units: rows of five joints, one unit
    apart in x and one and a half in y, centred in y."""
    j = np.arange(k)
    rows = (k - 1) // 5
    return np.stack([j % 5 - 2.0, (j // 5) * 1.5 - 0.75 * rows], axis=1)


def _background(k, c, h, w, rng, noise):
    g = synthetic._grid(h, w)
    cif = np.zeros((k, 5, h, w), dtype=np.float32)
    cif[:, 0] = rng.uniform(0.0, noise, (k, h, w))
    cif[:, 1:3] = g + rng.uniform(-0.5, 0.5, (k, 2, h, w))
    cif[:, 3] = 0.5
    cif[:, 4] = 1.0
    caf = np.zeros((c, 9, h, w), dtype=np.float32)
    caf[:, 0] = rng.uniform(0.0, noise, (c, h, w))
    caf[:, 1:3] = g
    caf[:, 5:7] = g + 4.0 * rng.uniform(-0.5, 0.5, (c, 2, h, w))
    caf[:, 3] = 0.5
    caf[:, 4] = 1.0
    caf[:, 7] = 0.5
    caf[:, 8] = 1.0
    return cif, caf


def _plant(cif, caf, kps, scale, skeleton, rng):
    """synthetic._plant_person for any K: a 4x4 CIF patch per joint and one 4x4 CAF patch at
    each limb's midpoint pointing joint1 -> joint2, confidences 0.7-1.0."""
    h, w = cif.shape[2:]
    for j in range(len(kps)):
        xs, ys = synthetic._patch_cells(kps[j, 0], kps[j, 1], h, w)
        conf = rng.uniform(0.7, 1.0, (len(ys), len(xs))).astype(np.float32)
        if conf.size == 0:
            continue
        sub = cif[j, :, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
        m = conf > sub[0]
        sub[0][m] = conf[m]
        sub[1][m] = kps[j, 0]
        sub[2][m] = kps[j, 1]
        sub[3][m] = 0.5
        sub[4][m] = scale
    for e, (j1, j2) in enumerate(skeleton):
        a, b = kps[j1 - 1], kps[j2 - 1]
        mid = 0.5 * (a + b)
        xs, ys = synthetic._patch_cells(mid[0], mid[1], h, w)
        conf = rng.uniform(0.7, 1.0, (len(ys), len(xs))).astype(np.float32)
        if conf.size == 0:
            continue
        sub = caf[e, :, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
        m = conf > sub[0]
        sub[0][m] = conf[m]
        sub[1][m], sub[2][m] = a[0], a[1]
        sub[3][m] = 0.5
        sub[4][m] = scale
        sub[5][m], sub[6][m] = b[0], b[1]
        sub[7][m] = 0.5
        sub[8][m] = scale


def planted_kc(k, skeleton, h, w, n_objects=PLANTED_OBJECTS, seed=0, noise=0.08):
    """synthetic.planted's recipe for any K: a low-confidence background and n_objects
    copies of template(k), scaled, shifted and jittered."""
    rng = np.random.default_rng(seed)
    cif, caf = _background(k, len(skeleton), h, w, rng, noise)
    t = template(k)
    for _ in range(n_objects):
        u = rng.uniform(1.5, 3.5)
        cx = rng.uniform(8.0, w - 8.0)
        cy = rng.uniform(8.0, h - 8.0)
        kps = np.stack([cx + u * t[:, 0], cy + u * t[:, 1]], axis=1) + rng.normal(0.0, 0.3, (k, 2))
        _plant(cif, caf, kps, 0.4 * u, skeleton, rng)
    return cif, caf


def planted_kc_multi(k, skeleton, h_px, w_px, strides, n_objects=MULTI_OBJECTS, seed=0,
                     noise=0.08):
    """synthetic.planted_multi for any K: the same objects seen at several strides, a list
    of (cif, caf) with fields of (h_px - 1) // stride + 1 rows."""
    rng = np.random.default_rng(seed)
    t = template(k)
    objects = []
    for _ in range(n_objects):
        u = rng.uniform(12.0, 28.0)  # pixels per pose unit
        cx = rng.uniform(0.25 * w_px, 0.75 * w_px)
        cy = rng.uniform(0.25 * h_px, 0.75 * h_px)
        kps = np.stack([cx + u * t[:, 0], cy + u * t[:, 1]], axis=1)
        objects.append((kps + rng.normal(0.0, 2.0, (k, 2)), u * rng.uniform(0.3, 1.2)))
    out = []
    for si, stride in enumerate(strides):
        h, w = (h_px - 1) // stride + 1, (w_px - 1) // stride + 1
        srng = np.random.default_rng(seed * 1000 + si)
        cif, caf = _background(k, len(skeleton), h, w, srng, noise)
        for kps, scale_px in objects:
            _plant(cif, caf, kps / stride, scale_px / stride, skeleton, srng)
        out.append((cif, caf))
    return out


def uniform_kc_multi(k, c, h_px, w_px, strides, seed=0):
    """uniform_kc at several strides: a list of (cif, caf), head si from seed * 1000 + si."""
    return [uniform_kc(k, c, (h_px - 1) // st + 1, (w_px - 1) // st + 1, seed * 1000 + si)
            for si, st in enumerate(strides)]


def multi_case(name, multi='ms2', seed=0):
    """fields list [cif_0, caf_0, cif_1, caf_1, ...] and FieldConfig kwargs of a synthetic
    MULTI_CASES entry with the K and skeleton of case `name`."""
    k, skeleton = case(name)
    strides, mins, dmin, dmax = synthetic.MULTI_CASES[multi]
    fields = []
    for cif, caf in planted_kc_multi(k, skeleton, MULTI_PX[0], MULTI_PX[1], strides, seed=seed):
        fields += [cif, caf]
    n = len(strides)
    kw = dict(cif_indices=[2 * i for i in range(n)], caf_indices=[2 * i + 1 for i in range(n)],
              cif_strides=list(strides), caf_strides=list(strides), cif_min_scales=list(mins),
              caf_min_distances=list(dmin), caf_max_distances=list(dmax))
    return fields, kw


def inputs(name, gen, h, w, seed=None):
    """(cif, caf, skeleton) of a case on `gen` ('uniform' or 'planted') fields; seed None:
    the case's own."""
    k, skeleton = case(name)
    if seed is None:
        seed = UNIFORM_SEEDS.get(name, 0) if gen == 'uniform' else PLANTED_SEED
    if gen == 'uniform':
        cif, caf = uniform_kc(k, len(skeleton), h, w, seed)
    else:
        cif, caf = planted_kc(k, skeleton, h, w, seed=seed)
    return cif, caf, skeleton


def config(mode, **kw):
    return make_config(**dict(EVAL_CONFIG if mode == 'eval' else PREDICT_CONFIG, **kw))


# ---- fixtures (tests/golden/kc_*.npz, written by gen_golden.py's `kc` section) -----------

def fixture_list():
    """(case, tag, mode) of every kc fixture gen_golden writes; tag = <gen><H>x<W> or ms2,
    mode = eval / predict / max / greedy (the last two: eval defaults with that option)."""
    out = []
    for name in NAMES:
        out.append((name, 'u20x23', 'eval'))
        out.append((name, 'p%dx%d' % PLANTED_SIZE, 'predict'))
        if name in VARIANT_CASES:
            out.append((name, 'p%dx%d' % PLANTED_SIZE, 'max'))
            out.append((name, 'p%dx%d' % PLANTED_SIZE, 'greedy'))
    return out


MULTI_FIXTURE = ('k24c64', 'ms2', 'eval')


def fixture_id(fx):
    return '%s_%s_%s' % fx


def fixture_path(fx):
    return os.path.join(GOLDEN, 'kc_%s.npz' % fixture_id(fx))


def load_fixture(fx):
    with np.load(fixture_path(fx), allow_pickle=False) as z:
        return {key: z[key] for key in z.files}


def committed_fixtures():
    return sorted(os.path.basename(p)[3:-4] for p in glob.glob(os.path.join(GOLDEN, 'kc_*.npz')))
