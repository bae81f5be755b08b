"""CIF / CAF target encoders: the cases, their annotations and the fixture loaders shared by
tests/test_encoder_cpu.py, tests/test_gpu_encoder.py and tests/golden/gen_encoder.py.

A case is a scene (pixel size, annotations, meta) and the encoders' options; every case is
encoded at strides 4, 8 and 16.  The scenes are literal or drawn from a seeded generator and
are stored in the fixtures, so a test reads what the reference was given.
"""
import copy
import os

import numpy as np

from openpifpaf_amd import constants, encoder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
STRIDES = (4, 8, 16)
CIF_KEYS = ('cif_intensities', 'cif_reg', 'cif_scale')
CAF_KEYS = ('caf_intensities', 'caf_reg1', 'caf_reg2', 'caf_scale1', 'caf_scale2')

# the COCO keypoint sigmas (the published OKS constants divided as datasets/constants.py
# lists them)
COCO_SIGMAS = [0.026, 0.025, 0.025, 0.035, 0.035, 0.079, 0.079, 0.072, 0.072, 0.062, 0.062,
               0.107, 0.107, 0.087, 0.087, 0.089, 0.089]

CHAIN5_POSE = np.array([[0.0, 0.0, 2.0], [1.0, 2.0, 2.0], [1.0, 2.5, 2.0], [3.0, 1.0, 2.0],
                        [4.0, 3.0, 2.0]])
CHAIN5_SKELETON = [(1, 2), (2, 3), (3, 4), (4, 5)]  # kc_util.CASES['chain5']


def person(cx, cy, size, seed, visible=None, k=17):
    """A COCO person: the upright pose, `size` pixels per pose unit around (cx, cy), y down,
    jittered by a seeded normal; float32 (K, 3) with v = 2, or 0 outside `visible`."""
    rng = np.random.default_rng(seed)
    pose = constants.COCO_UPRIGHT_POSE
    kps = np.zeros((k, 3), np.float32)
    kps[:, 0] = cx + size * pose[:, 0] + rng.normal(0.0, 0.02 * size, k)
    kps[:, 1] = cy - size * (pose[:, 1] - 5.0) + rng.normal(0.0, 0.02 * size, k)
    kps[:, 2] = 2.0
    if visible is not None:
        hide = [j for j in range(k) if j not in visible]
        kps[hide] = 0.0
    return kps


def ann(kps, iscrowd=False, bbox=None):
    kps = np.asarray(kps, np.float32)
    if bbox is None:
        vis = kps[kps[:, 2] > 0]
        if len(vis):
            x0, y0 = vis[:, 0].min(), vis[:, 1].min()
            bbox = (x0, y0, vis[:, 0].max() - x0, vis[:, 1].max() - y0)
        else:
            bbox = (0.0, 0.0, 1.0, 1.0)
    return {'keypoints': kps, 'bbox': np.asarray(bbox, np.float32), 'iscrowd': bool(iscrowd)}


def crowd(bbox, k=17):
    return ann(np.zeros((k, 3), np.float32), True, bbox)


def _overlap():
    a = person(80.0, 60.0, 10.0, 3)
    b = person(82.0, 61.0, 10.0, 4)
    # the two noses mirror each other about the centre of cell (10, 10) at stride 4: a tie,
    # which the first annotation wins; they are half a cell apart, so max_r clips the scale
    a[0, :2] = (41.0, 40.0)
    b[0, :2] = (39.0, 40.0)
    # the left eyes fall into one cell at every stride
    a[1, :2] = (50.0, 37.0)
    b[1, :2] = (51.5, 37.7)
    # a crowd box under the first person's legs: reg_l starts at 1.0 there
    return [ann(a), ann(b), crowd((60.0, 90.0, 50.0, 40.0))]


def _border():
    out = []
    for i, (cx, cy) in enumerate(((2.0, 80.0), (190.0, 80.0), (96.0, 2.0), (96.0, 158.0))):
        out.append(ann(person(cx, cy - 50.0, 10.0, 10 + i)))      # partly inside the padding
        out.append(ann(person(cx, cy - 200.0, 40.0, 20 + i)))     # partly beyond it
    return out


def _few():
    return [ann(person(60.0, 50.0, 9.0, 5, visible=(5, 6))),        # two joints: scale NaN
            ann(person(120.0, 60.0, 30.0, 6, visible=(0, 1, 2))),   # nose and eyes: factor > 5
            ann(person(140.0, 40.0, 8.0, 7))]


def _chain5():
    kps = np.array([[20.0, 30.0, 2.0], [180.0, 60.0, 2.0], [180.0, 60.0, 2.0],
                    [150.0, 120.0, 2.0], [100.0, 140.0, 2.0]], np.float32)
    other = np.array([[30.0, 100.0, 2.0], [60.0, 130.0, 2.0], [64.0, 131.0, 2.0],
                      [0.0, 0.0, 0.0], [120.0, 150.0, 2.0]], np.float32)
    return [ann(kps), ann(other), crowd((150.0, 10.0, 30.0, 30.0), k=5)]


_TWO = [ann(person(70.0, 40.0, 9.0, 1)), ann(person(130.0, 60.0, 7.0, 2)),
        crowd((10.0, 100.0, 60.0, 50.0))]
_TWO_AREA = (12.0, 0.0, 180.0, 140.0)  # inset on the left and at the bottom

# name -> scene and options; 'cif' False: a CAF-only case
CASES = {
    'two': dict(size=(161, 193), anns=_TWO, valid_area=_TWO_AREA),
    'overlap': dict(size=(161, 193), anns=_overlap()),
    'border': dict(size=(161, 193), anns=_border()),
    'few': dict(size=(161, 193), anns=_few()),
    'empty': dict(size=(161, 193), anns=[]),
    'crowd_only': dict(size=(161, 193), anns=[crowd((30.0, 20.0, 80.0, 90.0))],
                       valid_area=(0.0, 0.0, 192.0, 160.0)),
    'tiny': dict(size=(5, 7), anns=[ann(person(3.0, 2.0, 0.5, 8))]),
    'side1': dict(size=(161, 193), anns=_TWO, valid_area=_TWO_AREA, side=1),
    'side3': dict(size=(161, 193), anns=_TWO, side=3),
    'side5': dict(size=(161, 193), anns=_overlap(), side=5),
    'fov': dict(size=(161, 193), anns=_border(), cif=False, only_in_field_of_view=True),
    'dense': dict(size=(161, 193), anns=_TWO, cif=False,
                  skeleton=constants.DENSER_COCO_PERSON_SKELETON,
                  sparse_skeleton=constants.COCO_PERSON_SKELETON),
    'fixed': dict(size=(161, 193), anns=_overlap(), cif=False, fixed_size=True),
    'fixed1': dict(size=(161, 193), anns=_TWO, cif=False, fixed_size=True, side=1),
    'chain5': dict(size=(161, 193), anns=_chain5(), k=5, pose=CHAIN5_POSE, sigmas=None,
                   skeleton=CHAIN5_SKELETON),
}
NAMES = tuple(CASES)
SAME_SIZE = tuple(n for n in NAMES if CASES[n]['size'] == (161, 193))


def case(name):
    """The case with every option filled in; the annotations are copies."""
    c = dict(k=17, pose=constants.COCO_UPRIGHT_POSE, sigmas=COCO_SIGMAS,
             skeleton=constants.COCO_PERSON_SKELETON, sparse_skeleton=None,
             dense_to_sparse_radius=2.0, only_in_field_of_view=False, v_threshold=0, side=None,
             fixed_size=False, cif=True, valid_area=None)
    c.update(CASES[name])
    c['anns'] = copy.deepcopy(c['anns'])
    c['meta'] = {} if c['valid_area'] is None else {'valid_area': np.array(c['valid_area'])}
    return c


def encoders(c, stride, module=encoder):
    """(Cif or None, Caf) of `module` (this package's encoder, or the reference's) for a case;
    side / fixed_size are class attributes there: subclasses carry them."""
    rescaler = module.AnnRescaler(stride, c['k'], np.array(c['pose'], np.float64))
    cif_attrs = {} if c['side'] is None else {'side_length': c['side']}
    caf_attrs = {'fixed_size': c['fixed_size']}
    if c['side'] is not None:
        caf_attrs['min_size'] = c['side']
    cif_cls = type('Cif', (module.Cif,), cif_attrs)
    caf_cls = type('Caf', (module.Caf,), caf_attrs)
    cif = cif_cls(rescaler, sigmas=c['sigmas'], v_threshold=c['v_threshold']) if c['cif'] else None
    caf = caf_cls(rescaler, skeleton=[tuple(e) for e in c['skeleton']], sigmas=c['sigmas'],
                  sparse_skeleton=c['sparse_skeleton'],
                  dense_to_sparse_radius=c['dense_to_sparse_radius'],
                  only_in_field_of_view=c['only_in_field_of_view'],
                  v_threshold=c['v_threshold'])
    return cif, caf


def fixture_path(name):
    return os.path.join(GOLDEN, 'enc_%s.npz' % name)


_LOADED = {}


def load_fixture(name):
    """The fixture's arrays (read once, shared, read-only)."""
    if name not in _LOADED:
        with np.load(fixture_path(name), allow_pickle=False) as z:
            _LOADED[name] = {key: z[key] for key in z.files}
        for v in _LOADED[name].values():
            v.setflags(write=False)
    return _LOADED[name]


def fixture_scene(fx):
    """(size, anns, meta) as the fixture stores what the reference was given."""
    anns = [{'keypoints': kp.copy(), 'bbox': bb.copy(), 'iscrowd': bool(c)}
            for kp, bb, c in zip(fx['ann_keypoints'], fx['ann_bbox'], fx['ann_iscrowd'])]
    meta = {'valid_area': fx['valid_area'].copy()} if 'valid_area' in fx else {}
    return (int(fx['size'][0]), int(fx['size'][1])), anns, meta


def fixture_case(fx):
    """The options of `case` as the fixture stores them (for `encoders`)."""
    return dict(k=int(fx['k']), pose=fx['pose'],
                sigmas=[float(s) for s in fx['sigmas']] if bool(fx['has_sigmas']) else None,
                skeleton=[tuple(int(j) for j in e) for e in fx['skeleton']],
                sparse_skeleton=[tuple(int(j) for j in e) for e in fx['sparse_skeleton']] or None,
                dense_to_sparse_radius=float(fx['dense_to_sparse_radius']),
                only_in_field_of_view=bool(fx['only_in_field_of_view']),
                v_threshold=int(fx['v_threshold']),
                side=None if int(fx['side']) < 0 else int(fx['side']),
                fixed_size=bool(fx['fixed_size']), cif=bool(fx['has_cif']))


def fixture_runs():
    """(case, 'cif' / 'caf', stride) of every tensor set the fixtures hold."""
    return [(name, which, stride) for name in NAMES for which in ('cif', 'caf')
            for stride in STRIDES if which == 'caf' or CASES[name].get('cif', True)]


def expected(fx, which, stride):
    keys = CIF_KEYS if which == 'cif' else CAF_KEYS
    return tuple(fx['s%d_%s' % (stride, key)] for key in keys)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and \
        np.array_equal(a.view(np.uint32), b.view(np.uint32))
