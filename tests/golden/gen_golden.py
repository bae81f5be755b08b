"""Generate the golden fixtures in tests/golden/ by running the REFERENCE itself.

Run in the build container only (needs /root/reference):
    python tests/golden/gen_golden.py

The reference decoder is imported from /root/reference with its Cython primitives
compiled by oracle/build_ref.sh (see oracle/ref_loader.py).  Nothing of the reference is
copied: the fixtures hold inputs (or the parameters + SHA-256 that regenerate them with
openpifpaf_amd.synthetic) and the reference's outputs.

Fixtures:
  primitives.npz       known-answer tests for every openpifpaf.functional primitive
                       (small fields, full inputs and outputs, strided views, edge cases)
  errors.json          the reference's ValueError messages at the boundary
  detm_<case>.npz      CifDet over several heads / min scales (DET_MULTI_CASES): the same
                       records as det_<case>.npz
  det_<case>.npz       CifDet decoder (cifdet.py:27-52): CifDetHr digest + sums, the seed
                       list, and the AnnotationDet list (field, score, bbox)
  inverse.npz          Preprocess.annotations_inverse + json_data on reference-decoded poses
                       and detections under offset / scale, hflip + swap, rotation metas
  multi_<case>.npz     multi-scale FieldConfig decodes (cif_hr.py:59-73 pairs / maxima,
                       per-scale seeds, CafScored masks and concatenation) on planted_multi
  heads.npz            CompositeFieldFused (conv replaced by identity, eval mode) +
                       CifCafCollector / CifdetCollector on random conv outputs, quad 0-2
  nms.npz              nms.Keypoints().annotations on random overlapping Annotation lists
                       (inputs, output order as input indices, mutated data), per config
  nms_scored.npz       the same with fixed_score / suppress_score_index annotations
  api_initial_<mode>.npz  CifCaf.__call__(fields, initial_annotations) (cifcaf.py:95-98):
                       the initial annotations, the output list and which outputs are them
  api_seedmask_<mode>.npz  CifCaf with FieldConfig(seed_mask=...) (cif_seeds.py:28-29)
  api_confscales_<case>.npz  CifCaf(confidence_scales=...) decodes (cifcaf.py:259-260,
                       282-284): the weights, inputs by generator parameters, annotations
  api_stages.npz       CifSeeds.fill_cif min_scale / seed_mask and two heads, CafScored
                       fill_caf distance masks and two calls, CifHr fill_cif min_scale,
                       fill_multiple over three heads and into an existing map
  decode_<case>.npz    per-stage vectors of the full CifCaf decoder: CifHr digest +
                       per-field sums + windows, full seed list, CafScored counts + digests,
                       full annotation lists (data, joint_scales, score, decoding_order,
                       frontier_order)
  kc_<case>_<tag>_<mode>.npz  keypoint counts and skeletons other than COCO's
                       (tests/kc_util.py CASES): the keys of decode_<case>.npz with the arrays
                       sized by the stored K, on uniform_kc / planted_kc fields, and one
                       multi-scale (ms2) decode in the keys of multi_<case>.npz
  meta.json            NumPy / Cython versions and SIMD dispatch of the generating host
"""
import hashlib
import json
import os
import platform
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'oracle'))
sys.path.insert(0, os.path.join(REPO, 'tests'))

import kc_util  # noqa: E402  pylint: disable=wrong-import-position
import ref_loader  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd import constants, synthetic  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd._abi import EVAL_CONFIG, PREDICT_CONFIG  # noqa: E402  pylint: disable=wrong-import-position

MODES = {'eval': EVAL_CONFIG, 'predict': PREDICT_CONFIG}

# (name, generator, H, W, seed, mode, skeleton name, extra)
CASES = [
    ('u10_s0_eval', 'uniform', 10, 10, 0, 'eval', 'coco', {}),
    ('u20_s0_eval', 'uniform', 20, 20, 0, 'eval', 'coco', {}),
    ('u20_s1_eval', 'uniform', 20, 20, 1, 'eval', 'coco', {}),
    ('u20_s2_predict', 'uniform', 20, 20, 2, 'predict', 'coco', {}),
    ('u16x21_s0_eval', 'uniform', 16, 21, 0, 'eval', 'coco', {}),
    ('p31x41_s0_eval', 'planted', 31, 41, 0, 'eval', 'coco', {'n_people': 3}),
    ('p40_s0_eval', 'planted', 40, 40, 0, 'eval', 'coco', {}),
    ('p40_s0_predict', 'planted', 40, 40, 0, 'predict', 'coco', {}),
    ('p40_s3_max', 'planted', 40, 40, 3, 'eval', 'coco', {'connection_method': 'max'}),
    ('p40_s4_greedy', 'planted', 40, 40, 4, 'eval', 'coco', {'greedy': True}),
    ('p80_s0_eval', 'planted', 80, 80, 0, 'eval', 'coco', {}),
    ('p80_s1_eval', 'planted', 80, 80, 1, 'eval', 'coco', {}),
    ('p80_s2_eval', 'planted', 80, 80, 2, 'eval', 'coco', {}),
    ('p80_s3_eval', 'planted', 80, 80, 3, 'eval', 'coco', {}),
    ('p80_s0_predict', 'planted', 80, 80, 0, 'predict', 'coco', {}),
    ('p81_s0_eval', 'planted', 81, 81, 0, 'eval', 'coco', {}),
    ('u80_s0_eval', 'uniform', 80, 80, 0, 'eval', 'coco', {}),
    ('u80_s0_predict', 'uniform', 80, 80, 0, 'predict', 'coco', {}),
    ('p160_s0_dense_eval', 'planted', 160, 160, 0, 'eval', 'dense', {'n_people': 16}),
    ('u160_s0_dense_eval', 'uniform', 160, 160, 0, 'eval', 'dense', {}),
    ('zero20_eval', 'zero', 20, 20, 0, 'eval', 'coco', {}),
]

SKELETONS = {'coco': constants.COCO_PERSON_SKELETON, 'dense': constants.DENSE_DECODE_SKELETON}


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def make_inputs(gen, h, w, seed, skeleton, extra):
    if gen == 'zero':
        return (np.zeros((17, 5, h, w), np.float32), np.zeros((len(skeleton), 9, h, w), np.float32))
    if gen == 'uniform':
        return synthetic.uniform(h, w, n_caf=len(skeleton), seed=seed)
    return synthetic.planted(h, w, n_people=extra.get('n_people', 8), seed=seed,
                             skeleton=skeleton)


def configure(decoder, mode, extra):
    c = MODES[mode]
    decoder.CifHr.v_threshold = 0.1
    decoder.CifSeeds.threshold = c['seed_threshold']
    decoder.CafScored.default_score_th = 0.1
    decoder.CifCaf.force_complete = c['force_complete']
    decoder.CifCaf.keypoint_threshold = c['keypoint_threshold']
    decoder.CifCaf.greedy = extra.get('greedy', False)
    decoder.CifCaf.connection_method = extra.get('connection_method', 'blend')
    decoder.nms.Keypoints.instance_threshold = c['nms_instance_threshold']
    decoder.nms.Keypoints.keypoint_threshold = c['nms_keypoint_threshold']


def ann_arrays(anns, n_caf, k=17):
    """Annotation list -> data, scales, score, decoding / frontier order arrays."""
    out = {}
    n = len(anns)
    out['ann_data'] = np.array([a.data for a in anns], np.float32).reshape(n, k, 3)
    out['ann_joint_scales'] = np.array([a.joint_scales for a in anns], np.float32).reshape(n, k)
    out['ann_score'] = np.array([a.score() for a in anns], np.float64)
    dec_pairs = np.full((n, k, 2), -1, np.int16)
    dec_xyv = np.zeros((n, k, 6), np.float32)
    fr = np.full((n, 4 * n_caf, 2), -1, np.int16)
    for i, a in enumerate(anns):
        for t, (j1, j2, x1, x2) in enumerate(a.decoding_order):
            dec_pairs[i, t] = (j1, j2)
            dec_xyv[i, t, :3] = x1
            dec_xyv[i, t, 3:] = x2
        for t, (j1, j2) in enumerate(a.frontier_order):
            fr[i, t] = (j1, j2)
    out['ann_decoding_pairs'] = dec_pairs
    out['ann_decoding_xyv'] = dec_xyv
    out['ann_frontier_pairs'] = fr
    return out


def run_case(op, name, gen, h, w, seed, mode, skel_name, extra):
    from openpifpaf import decoder  # pylint: disable=import-outside-toplevel
    skeleton = list(SKELETONS[skel_name])
    configure(decoder, mode, extra)
    cif, caf = make_inputs(gen, h, w, seed, skeleton, extra)
    fc = decoder.FieldConfig()
    hr = decoder.CifHr(fc).fill([cif, caf]).accumulated
    seeds = decoder.CifSeeds(hr, fc).fill([cif, caf]).get()
    cs_a = decoder.CafScored(hr, fc, skeleton).fill([cif, caf])
    cs_b = decoder.CafScored(hr, fc, skeleton, score_th=0.0001).fill([cif, caf])
    dec = decoder.CifCaf(fc, keypoints=constants.COCO_KEYPOINTS, skeleton=skeleton,
                         out_skeleton=constants.COCO_PERSON_SKELETON)
    anns = dec([cif, caf])

    out = {
        'generator': np.array(gen), 'H': h, 'W': w, 'seed': seed, 'mode': np.array(mode),
        'skeleton': np.asarray(skeleton, np.int32),
        'n_people': extra.get('n_people', 8),
        'connection_method': np.array(extra.get('connection_method', 'blend')),
        'greedy': int(extra.get('greedy', False)),
        'input_sha': np.array(sha(cif, caf)),
        'cifhr_sha': np.array(sha(hr)),
        'cifhr_field_sums': hr.astype(np.float64).sum(axis=(1, 2)),
        'seeds': np.array([tuple(float(t) for t in s) for s in seeds], np.float32).reshape(-1, 5),
    }
    if h <= 10:
        out['cifhr'] = hr
    # windows: top-left corner of each field's 48x48 window at the densest 8x8 cell block
    wins = []
    for f in (0, 5, 11, 16):
        yy = min(hr.shape[1] - 48, hr.shape[1] // 3)
        xx = min(hr.shape[2] - 48, hr.shape[2] // 3)
        wins.append(hr[f, max(0, yy):max(0, yy) + 48, max(0, xx):max(0, xx) + 48])
    out['cifhr_windows'] = np.stack([np.pad(wd, ((0, 48 - wd.shape[0]), (0, 48 - wd.shape[1])))
                                     for wd in wins])
    for tag, cs in (('a', cs_a), ('b', cs_b)):
        out['caf_%s_fwd_counts' % tag] = np.array([f.shape[1] for f in cs.forward], np.int32)
        out['caf_%s_bwd_counts' % tag] = np.array([b.shape[1] for b in cs.backward], np.int32)
        out['caf_%s_fwd_sha' % tag] = np.array([sha(f) for f in cs.forward])
        out['caf_%s_bwd_sha' % tag] = np.array([sha(b) for b in cs.backward])
        if h <= 10:
            out['caf_%s_fwd_cat' % tag] = np.concatenate(cs.forward, axis=1)
            out['caf_%s_bwd_cat' % tag] = np.concatenate(cs.backward, axis=1)

    out.update(ann_arrays(anns, len(skeleton)))
    np.savez_compressed(os.path.join(HERE, 'decode_%s.npz' % name), **out)
    print('%-22s seeds %5d  caf_a %6d  caf_b %7d  anns %4d' % (
        name, len(seeds), out['caf_a_fwd_counts'].sum(), out['caf_b_fwd_counts'].sum(), len(anns)))


def gen_primitives(op):
    F = sys.modules['openpifpaf.functional']
    rng = np.random.default_rng(1234)
    out = {}

    def points(n, h, w, smin, smax):
        x = rng.uniform(-4, w + 4, n).astype(np.float32)
        y = rng.uniform(-4, h + 4, n).astype(np.float32)
        s = rng.uniform(smin, smax, n).astype(np.float32)
        v = rng.uniform(0.0, 0.8, n).astype(np.float32)
        # integer and half-integer centres exercise the nearest-pixel branch
        x[:6] = np.round(x[:6])
        y[:6] = np.round(y[:6]) + 0.25
        return x, y, s, v

    h, w = 24, 32
    for t, (trunc, maxv) in enumerate([(1.0, 1.0), (2.0, 1.0), (0.5, 0.7), (2.0, 0.3)]):
        field = rng.uniform(0, 0.9, (h, w)).astype(np.float32)
        x, y, s, v = points(40, h, w, 0.3, 6.0)
        out['sqg_max_%d_in' % t] = field.copy()
        out['sqg_max_%d_pts' % t] = np.stack([x, y, s, v])
        out['sqg_max_%d_args' % t] = np.array([trunc, maxv], np.float32)
        F.scalar_square_add_gauss_with_max(field, x, y, s, v, truncate=trunc, max_value=maxv)
        out['sqg_max_%d_out' % t] = field
    # strided view + empty point list
    big = rng.uniform(0, 0.5, (2 * h, 2 * w + 1)).astype(np.float32)
    out['sqg_max_strided_in'] = big.copy()
    x, y, s, v = points(25, h, w, 0.5, 4.0)
    out['sqg_max_strided_pts'] = np.stack([x, y, s, v])
    F.scalar_square_add_gauss_with_max(big[::2, 1::2], x, y, s, v, truncate=1.0)
    out['sqg_max_strided_out'] = big
    field = rng.uniform(0, 0.5, (h, w)).astype(np.float32)
    out['sqg_max_empty_in'] = field.copy()
    e = np.zeros(0, np.float32)
    F.scalar_square_add_gauss_with_max(field, e, e, e, e)
    out['sqg_max_empty_out'] = field

    for t, trunc in enumerate([2.0, 1.0]):
        field = rng.uniform(0, 0.5, (h, w)).astype(np.float32)
        x, y, s, v = points(30, h, w, 0.3, 5.0)
        out['sqg_%d_in' % t] = field.copy()
        out['sqg_%d_pts' % t] = np.stack([x, y, s, v])
        out['sqg_%d_args' % t] = np.array([trunc], np.float32)
        F.scalar_square_add_gauss(field, x, y, s, v, truncate=trunc)
        out['sqg_%d_out' % t] = field

    for t, trunc in enumerate([2.0, 1.0]):
        field = rng.uniform(0, 0.5, (h, w)).astype(np.float32)
        x, y, s, v = points(30, h, w, 0.3, 5.0)
        out['sqmax_%d_in' % t] = field.copy()
        out['sqmax_%d_pts' % t] = np.stack([x, y, s, v])
        out['sqmax_%d_args' % t] = np.array([trunc], np.float32)
        F.scalar_square_max_gauss(field, x, y, s, v, truncate=trunc)
        out['sqmax_%d_out' % t] = field

    field = rng.uniform(0, 0.5, (h, w)).astype(np.float32)
    x, y, s, v = points(30, h, w, 0.3, 5.0)
    out['sqc_in'] = field.copy()
    out['sqc_pts'] = np.stack([x, y, s, v])
    F.scalar_square_add_constant(field, x, y, s, v)
    out['sqc_out'] = field

    cuma = rng.uniform(0, 1, (h, w)).astype(np.float32)
    cumw = rng.uniform(0, 2, (h, w)).astype(np.float32)
    cumw[:4] = 0.0
    x, y, s, v = points(30, h, w, 0.3, 5.0)
    wt = rng.uniform(-0.5, 1.5, 30).astype(np.float32)
    out['cuma_in'] = np.stack([cuma, cumw])
    out['cuma_pts'] = np.stack([x, y, s, v, wt])
    F.cumulative_average(cuma, cumw, x, y, s, v, wt)
    out['cuma_out'] = np.stack([cuma, cumw])

    for t, n in enumerate([7, 50, 1]):
        xw = rng.normal(0, 10, (n, 2)).astype(np.float32)
        y0 = rng.normal(0, 3, 2).astype(np.float32)
        wts = rng.uniform(0.1, 2.0, n).astype(np.float32)
        y = y0.copy()
        _, denom = F.weiszfeld_nd(xw, y, weights=wts)
        out['weisz_%d_x' % t] = xw
        out['weisz_%d_y0' % t] = y0
        out['weisz_%d_w' % t] = wts
        out['weisz_%d_y' % t] = y
        out['weisz_%d_denom' % t] = denom

    field = rng.uniform(0, 1, (h, w)).astype(np.float32)
    px = np.concatenate([rng.uniform(-2, w + 2, 60), [0.0, w - 1.0, w - 0.9, -0.0, 3.9]]).astype(np.float32)
    py = np.concatenate([rng.uniform(-2, h + 2, 60), [0.0, h - 1.0, 2.0, h - 0.5, 1.0]]).astype(np.float32)
    out['lookup_field'] = field
    out['lookup_pts'] = np.stack([px, py])
    out['scalar_values'] = F.scalar_values(field, px, py)
    out['scalar_values_d0'] = F.scalar_values(field, px, py, default=0.0)
    out['scalar_value'] = np.array([F.scalar_value(field, a, b) for a, b in zip(px, py)], np.float32)
    out['scalar_value_clipped'] = np.array(
        [F.scalar_value_clipped(field, a, b) for a, b in zip(px, py)], np.float32)
    occ = rng.integers(0, 3, (h, w)).astype(np.uint8)
    out['lookup_occ'] = occ
    out['scalar_nonzero'] = np.array([F.scalar_nonzero(occ, a, b) for a, b in zip(px, py)], np.uint8)
    out['scalar_nonzero_clipped'] = np.array(
        [F.scalar_nonzero_clipped(occ, a, b) for a, b in zip(px, py)], np.uint8)
    out['scalar_nonzero_red'] = np.array(
        [F.scalar_nonzero_clipped_with_reduction(occ, 2 * a, 2 * b, 2.0) for a, b in zip(px, py)],
        np.uint8)

    caf = rng.uniform(0, 20, (9, 200)).astype(np.float32)
    caf[3] = rng.uniform(0.5, 3, 200)
    out['center_field'] = caf
    qs = np.array([[10.0, 10.0, 3.0], [5.0, 15.0, 1.5], [0.0, 0.0, 2.0], [12.5, 7.25, 6.0]],
                  np.float32)
    out['center_queries'] = qs
    for t, (qx, qy, qs_) in enumerate(qs):
        out['caf_center_s_%d' % t] = F.caf_center_s(caf, qx, qy, qs_)
        out['paf_center_%d' % t] = F.paf_center(caf[:7], qx, qy, qs_)
        out['paf_center_b_%d' % t] = F.paf_center_b(caf[:7], qx, qy, sigma=qs_ / 3)
        out['paf_mask_center_%d' % t] = F.paf_mask_center(caf[:7], qx, qy, sigma=qs_ / 3)
    np.savez_compressed(os.path.join(HERE, 'primitives.npz'), **out)
    print('primitives: %d arrays' % len(out))


def gen_errors():
    F = sys.modules['openpifpaf.functional']
    errs = {}

    def capture(name, fn):
        try:
            fn()
            errs[name] = None
        except Exception as e:  # pylint: disable=broad-except
            errs[name] = [type(e).__name__, str(e)]

    f32 = np.zeros((4, 4), np.float32)
    p = np.zeros(2, np.float32)
    capture('dtype', lambda: F.scalar_square_add_gauss_with_max(np.zeros((4, 4)), p, p, p, p))
    ro = np.zeros((4, 4), np.float32)
    ro.setflags(write=False)
    capture('readonly', lambda: F.scalar_values(ro, p, p))
    capture('ndim', lambda: F.scalar_values(np.zeros((2, 4, 4), np.float32), p, p))
    capture('weiszfeld_none', lambda: F.weiszfeld_nd(np.zeros((3, 2), np.float32),
                                                     np.zeros(2, np.float32)))
    capture('ndim_points', lambda: F.scalar_values(f32, np.zeros((2, 2), np.float32), p))
    with open(os.path.join(HERE, 'errors.json'), 'w') as fh:
        json.dump(errs, fh, indent=1, sort_keys=True)
    print('errors:', errs)


NMS_CASES = [  # (name, n annotations, spread px, seed, keypoint_th, instance_th, suppression)
    ('eval', 60, 160.0, 0, 0.0, 0.0, 0.0),
    ('predict', 60, 160.0, 1, 0.001, 0.1, 0.0),
    ('supp', 80, 120.0, 2, 0.0, 0.0, 0.5),
    ('dense', 300, 200.0, 3, 0.001, 0.1, 0.0),
    ('zeros', 20, 80.0, 4, 0.3, 0.2, 0.0),
]


def gen_nms(op):
    """Random overlapping poses through the reference nms.Keypoints (nms.py:17-57)."""
    from openpifpaf.annotation import Annotation  # pylint: disable=import-outside-toplevel
    from openpifpaf.decoder import nms  # pylint: disable=import-outside-toplevel
    out = {}
    kps, skel = constants.COCO_KEYPOINTS, constants.COCO_PERSON_SKELETON
    for name, n, spread, seed, kt, it, sup in NMS_CASES:
        rng = np.random.default_rng(100 + seed)
        base = rng.uniform(10.0, spread, (n, 1, 2)).astype(np.float32)
        xy = (base + rng.normal(0.0, 12.0, (n, 17, 2))).astype(np.float32)
        v = rng.uniform(0.0, 1.0, (n, 17)).astype(np.float32)
        v[rng.uniform(0.0, 1.0, (n, 17)) < 0.2] = 0.0
        data = np.concatenate([xy, v[:, :, None]], axis=2).astype(np.float32)
        scales = rng.uniform(0.5, 24.0, (n, 17)).astype(np.float32)
        anns = []
        for i in range(n):
            a = Annotation(kps, skel)
            a.data = data[i].copy()
            a.joint_scales = scales[i].copy()
            anns.append(a)
        k = nms.Keypoints()
        k.keypoint_threshold, k.instance_threshold, k.suppression = kt, it, sup
        ids = {id(a): i for i, a in enumerate(anns)}
        res = k.annotations(list(anns))
        out[name + '_data_in'] = data
        out[name + '_scales'] = scales
        out[name + '_cfg'] = np.array([kt, it, sup], np.float32)
        out[name + '_order'] = np.array([ids[id(a)] for a in res], np.int64)
        out[name + '_data_out'] = np.stack([a.data for a in anns]).astype(np.float32)
        out[name + '_score'] = np.array([a.score() for a in res], np.float64)
        print('nms', name, n, '->', len(res))
    np.savez_compressed(os.path.join(HERE, 'nms.npz'), **out)


NMS_SCORED_CASES = [  # (name, n, spread, seed, keypoint_th, instance_th, suppression)
    ('mixed', 160, 150.0, 5, 0.05, 0.15, 0.0),
    ('fixed_ties', 60, 90.0, 6, 0.0, 0.2, 0.3),
]
NO_INDEX = -999  # suppress_score_index None in the fixture


def gen_nms_scored(op):
    """nms.Keypoints over annotations carrying fixed_score and suppress_score_index
    (annotation.py:24-28, 60-71; nms.py:21, 33, 53-54 filter and sort by score())."""
    from openpifpaf.annotation import Annotation  # pylint: disable=import-outside-toplevel
    from openpifpaf.decoder import nms  # pylint: disable=import-outside-toplevel
    out = {}
    kps, skel = constants.COCO_KEYPOINTS, constants.COCO_PERSON_SKELETON
    for name, n, spread, seed, kt, it, sup in NMS_SCORED_CASES:
        rng = np.random.default_rng(200 + seed)
        base = rng.uniform(10.0, spread, (n, 1, 2)).astype(np.float32)
        xy = (base + rng.normal(0.0, 12.0, (n, 17, 2))).astype(np.float32)
        v = rng.uniform(0.0, 1.0, (n, 17)).astype(np.float32)
        v[rng.uniform(0.0, 1.0, (n, 17)) < 0.2] = 0.0
        data = np.concatenate([xy, v[:, :, None]], axis=2).astype(np.float32)
        scales = rng.uniform(0.5, 24.0, (n, 17)).astype(np.float32)
        kind = rng.integers(0, 3, n) if name == 'mixed' else np.full(n, 1)
        fixed = np.full(n, np.nan)
        supp = np.full(n, NO_INDEX, np.int64)
        anns = []
        for i in range(n):
            if kind[i] == 2:  # suppress_score_index, Python indices incl. negative and 0
                supp[i] = [-1, 0, 5, 16, -3][i % 5]
                a = Annotation(kps, skel, suppress_score_index=int(supp[i]))
            else:
                a = Annotation(kps, skel)
            a.data = data[i].copy()
            a.joint_scales = scales[i].copy()
            if kind[i] == 1:  # fixed_score: ties, the threshold itself, below it
                fixed[i] = [it, 0.5, 0.25, 0.9, it * 0.5, float(rng.uniform())][i % 6]
                a.fixed_score = float(fixed[i])
            anns.append(a)
        k = nms.Keypoints()
        k.keypoint_threshold, k.instance_threshold, k.suppression = kt, it, sup
        ids = {id(a): i for i, a in enumerate(anns)}
        res = k.annotations(list(anns))
        out[name + '_data_in'] = data
        out[name + '_scales'] = scales
        out[name + '_cfg'] = np.array([kt, it, sup], np.float64)
        out[name + '_fixed'] = fixed
        out[name + '_supp'] = supp
        out[name + '_order'] = np.array([ids[id(a)] for a in res], np.int64)
        out[name + '_data_out'] = np.stack([a.data for a in anns]).astype(np.float32)
        out[name + '_score'] = np.array([a.score() for a in res], np.float64)
        print('nms scored', name, n, '->', len(res))
    np.savez_compressed(os.path.join(HERE, 'nms_scored.npz'), **out)


def gen_heads(op):
    """Raw head conv output -> decoder fields through the reference modules."""
    import torch  # pylint: disable=import-outside-toplevel
    from openpifpaf.network import heads  # pylint: disable=import-outside-toplevel
    kps, skel = constants.COCO_KEYPOINTS, constants.COCO_PERSON_SKELETON
    metas = {
        'cif': heads.IntensityMeta('cif', kps, [0.05] * 17, None),
        'caf': heads.AssociationMeta('caf', kps, [0.05] * 17, None, skel),
        'cifdet': heads.DetectionMeta('cifdet', ['a', 'b', 'c']),
    }
    out = {}
    rng = np.random.default_rng(11)
    for quad in (0, 1, 2):
        heads.CompositeFieldFused.quad = quad
        res = {}
        for kind, meta in metas.items():
            head = heads.CompositeFieldFused(meta, 4)
            head.conv = torch.nn.Identity()
            head.eval()
            per = {'cif': 5, 'caf': 9, 'cifdet': 7}[kind]
            h, w = 3, 4
            x = (2.0 * rng.standard_normal((1, meta.n_fields * per * 4 ** quad, h, w))).astype(
                np.float32)
            with torch.no_grad():
                res[kind] = head(torch.from_numpy(x))
            out['q%d_%s_conv' % (quad, kind)] = x
        with torch.no_grad():
            cif, caf = heads.CifCafCollector([0], [1])([res['cif'], res['caf']])
            (det,) = heads.CifdetCollector([0])([res['cifdet']])
        out['q%d_cif' % quad] = cif.numpy()
        out['q%d_caf' % quad] = caf.numpy()
        out['q%d_cifdet' % quad] = det.numpy()
        print('heads quad', quad, cif.shape, caf.shape, det.shape)
    heads.CompositeFieldFused.quad = 1
    np.savez_compressed(os.path.join(HERE, 'heads.npz'), **out)


# (name, generator, H, W, seed, seed threshold, n_categories)
DET_CASES = [
    ('dp40_s0', 'planted', 40, 40, 0, 0.5, 3),
    ('dp40_s1', 'planted', 40, 40, 1, 0.2, 3),
    ('dp80_s2', 'planted', 80, 80, 2, 0.5, 3),
    ('dp40_c1', 'planted', 40, 40, 3, 0.5, 1),
    ('du20_s0', 'uniform', 20, 20, 0, 0.05, 3),
    ('du40_s1', 'uniform', 40, 40, 1, 0.1, 2),
]


def inverse_metas(hswap):
    base = {'offset': np.array((3.5, -2.25)), 'scale': np.array((0.5, 0.75)),
            'rotation': {'angle': 0.0, 'width': None, 'height': None}, 'hflip': False,
            'width_height': np.array((641, 427)), 'image_id': 7}
    flip = dict(base, hflip=True, horizontal_swap=hswap)
    rot = dict(base, rotation={'angle': 12.5, 'width': 481, 'height': 361},
               offset=np.array((-1.0, 4.5)), scale=np.array((1.25, 0.8)))
    return {'shift': base, 'flip': flip, 'rot': rot}


def gen_inverse(op):
    """Preprocess.annotations_inverse (preprocess.py:35-95) + json_data on decoded output."""
    import json  # pylint: disable=import-outside-toplevel
    from openpifpaf import transforms  # pylint: disable=import-outside-toplevel
    from openpifpaf.decoder import CifCaf, CifDet, FieldConfig  # pylint: disable=import-outside-toplevel
    from openpifpaf.decoder.cif_seeds import CifSeeds  # pylint: disable=import-outside-toplevel
    from openpifpaf.datasets import constants as dc  # pylint: disable=import-outside-toplevel
    from openpifpaf.transforms.hflip import _HorizontalSwap  # pylint: disable=import-outside-toplevel
    kps, skel = constants.COCO_KEYPOINTS, constants.COCO_PERSON_SKELETON
    metas = inverse_metas(_HorizontalSwap(kps, dc.HFLIP))
    out = {}
    cif, caf = make_inputs('planted', 40, 40, 0, skel, {})
    decoder = __import__('openpifpaf').decoder
    configure(decoder, 'eval', {})
    anns = CifCaf(FieldConfig(), keypoints=kps, skeleton=skel)([cif, caf])
    nd = max(len(a.decoding_order) for a in anns)
    out['pose_data'] = np.stack([a.data for a in anns]).astype(np.float32)
    out['pose_scales'] = np.stack([a.joint_scales for a in anns]).astype(np.float32)
    dxyv = np.zeros((len(anns), nd, 6), np.float32)
    dpairs = np.zeros((len(anns), nd, 2), np.int64)
    for i, a in enumerate(anns):
        for t, (j1, j2, c1, c2) in enumerate(a.decoding_order):
            dxyv[i, t, :3], dxyv[i, t, 3:] = c1[:3], c2[:3]
            dpairs[i, t] = (j1, j2)
    out['pose_dxyv'] = dxyv
    out['pose_dpairs'] = dpairs
    out['pose_nd'] = np.array([len(a.decoding_order) for a in anns], np.int64)
    CifSeeds.threshold = 0.5
    det = synthetic.det_batch('planted', 1, 40, 40, first_seed=0, n_categories=3)[0]
    dets = CifDet(FieldConfig(), ['c0', 'c1', 'c2'])([det])
    CifSeeds.threshold = None
    out['det_field'] = np.array([a.field_i for a in dets], np.int64)
    out['det_score'] = np.array([a.score for a in dets], np.float32)
    out['det_bbox'] = np.stack([a.bbox for a in dets]).astype(np.float32)
    for name, meta in metas.items():
        inv = transforms.Preprocess.annotations_inverse(anns, meta)
        out[name + '_pose_data'] = np.stack([a.data for a in inv]).astype(np.float32)
        out[name + '_pose_scales'] = np.stack([a.joint_scales for a in inv]).astype(np.float32)
        o = np.zeros_like(dxyv)
        for i, a in enumerate(inv):
            for t, (_, __, c1, c2) in enumerate(a.decoding_order):
                o[i, t, :3], o[i, t, 3:] = c1[:3], c2[:3]
        out[name + '_pose_dxyv'] = o
        out[name + '_pose_json'] = np.array(json.dumps([a.json_data() for a in inv]))
        dinv = transforms.Preprocess.annotations_inverse(dets, meta)
        out[name + '_det_bbox'] = np.stack([a.bbox for a in dinv]).astype(np.float32)
        out[name + '_det_json'] = np.array(json.dumps([a.json_data() for a in dinv]))
        print('inverse', name, len(inv), len(dinv))
    np.savez_compressed(os.path.join(HERE, 'inverse.npz'), **out)


def gen_multi(op):
    """Multi-scale decodes through the reference (factory.py:153-180 FieldConfig)."""
    decoder = __import__('openpifpaf').decoder
    from openpifpaf.decoder import CafScored, CifCaf, CifHr, CifSeeds, FieldConfig  # pylint: disable=import-outside-toplevel
    kps, skel = constants.COCO_KEYPOINTS, constants.COCO_PERSON_SKELETON
    for name in synthetic.MULTI_CASES:
        for mode in ('eval', 'predict'):
            fields, kw = synthetic.multi_case(name)
            configure(decoder, mode, {})
            fc = FieldConfig(**kw)
            hr = CifHr(fc).fill(fields).accumulated
            seeds = CifSeeds(hr, fc).fill(fields).get()
            anns = CifCaf(fc, keypoints=kps, skeleton=skel)(fields)
            out = {
                'name': np.array(name), 'mode': np.array(mode),
                'connection_method': np.array('blend'), 'greedy': 0,
                'input_sha': np.array(sha(*fields)),
                'cifhr_sha': np.array(sha(hr)), 'cifhr_shape': np.array(hr.shape),
                'seeds': np.array([[float(t) for t in sd] for sd in seeds],
                                  np.float32).reshape(-1, 5),
            }
            for tag, th in (('a', None), ('b', 0.0001)):
                cs = CafScored(hr, fc, skel, score_th=th).fill(fields)
                out['caf_%s_fwd_counts' % tag] = np.array([f.shape[1] for f in cs.forward])
                out['caf_%s_bwd_counts' % tag] = np.array([b.shape[1] for b in cs.backward])
                out['caf_%s_fwd_sha' % tag] = np.array([sha(f) for f in cs.forward])
                out['caf_%s_bwd_sha' % tag] = np.array([sha(b) for b in cs.backward])
            out.update(ann_arrays(anns, len(skel)))
            np.savez_compressed(os.path.join(HERE, 'multi_%s_%s.npz' % (name, mode)), **out)
            print('multi', name, mode, hr.shape, 'seeds', len(seeds), 'anns', len(anns))


def gen_det_nms(op):
    """nms.Detection().annotations on random overlapping boxes (nms.py:79-102)."""
    from openpifpaf.annotation import AnnotationDet  # pylint: disable=import-outside-toplevel
    from openpifpaf.decoder import nms  # pylint: disable=import-outside-toplevel
    out = {}
    for name, n, spread, seed in (('few', 12, 40.0, 0), ('many', 400, 300.0, 1),
                                  ('ties', 60, 20.0, 2)):
        rng = np.random.default_rng(200 + seed)
        xy = rng.uniform(0.0, spread, (n, 2)).astype(np.float32)
        wh = rng.uniform(4.0, 60.0, (n, 2)).astype(np.float32)
        scores = rng.uniform(0.0, 1.0, n).astype(np.float32)
        if name == 'ties':
            scores = np.round(scores * 4) / 4  # many equal scores: stable-sort ties
            scores = scores.astype(np.float32)
        fields = rng.integers(0, 3, n)
        anns = [AnnotationDet(['a', 'b', 'c']).set(int(f), np.float32(s),
                                                   (xy[i, 0], xy[i, 1], wh[i, 0], wh[i, 1]))
                for i, (f, s) in enumerate(zip(fields, scores))]
        ids = {id(a): i for i, a in enumerate(anns)}
        res = nms.Detection().annotations(list(anns))
        out[name + '_field'] = fields.astype(np.int64)
        out[name + '_score_in'] = scores
        out[name + '_bbox'] = np.concatenate([xy, wh], axis=1)
        out[name + '_order'] = np.array([ids[id(a)] for a in res], np.int64)
        out[name + '_score_out'] = np.array([a.score for a in anns], np.float32)
        print('det nms', name, n, '->', len(res))
    np.savez_compressed(os.path.join(HERE, 'det_nms.npz'), **out)


def gen_det(op):
    """The reference CifDet decoder on synthetic detection fields."""
    from openpifpaf.decoder import CifDet, CifDetHr, FieldConfig  # pylint: disable=import-outside-toplevel
    from openpifpaf.decoder.cif_seeds import CifDetSeeds, CifSeeds  # pylint: disable=import-outside-toplevel
    for name, gen, h, w, seed, th, n_cat in DET_CASES:
        det = synthetic.det_batch(gen, 1, h, w, first_seed=seed, n_categories=n_cat)[0]
        CifSeeds.threshold = th
        fc = FieldConfig()
        hr = CifDetHr(fc).fill([det]).accumulated
        seeds = CifDetSeeds(hr, fc).fill([det]).get()
        anns = CifDet(fc, ['c%d' % i for i in range(n_cat)])([det])
        out = {
            'gen': np.array(gen), 'h': h, 'w': w, 'seed': seed, 'seed_threshold': th,
            'n_categories': n_cat, 'input_sha': np.array(sha(det)),
            'cifhr_sha': np.array(sha(hr)), 'cifhr_sums': hr.sum(axis=(1, 2), dtype=np.float64),
            'seeds': np.array([[float(t) for t in sd] for sd in seeds], np.float32).reshape(-1, 6),
            'ann_field': np.array([a.field_i for a in anns], np.int64),
            'ann_score': np.array([a.score for a in anns], np.float32),
            'ann_bbox': np.array([a.bbox for a in anns], np.float32).reshape(-1, 4),
        }
        np.savez_compressed(os.path.join(HERE, 'det_%s.npz' % name), **out)
        print('det', name, 'seeds', len(seeds), 'anns', len(anns))
    CifSeeds.threshold = None


# CifDet over several heads and / or min scales (cif_hr.py:67-80 and cif_seeds.py:56-64 as
# CifDetHr / CifDetSeeds inherit them, cif_hr.py:84-90, cif_seeds.py:75-77): name, generator,
# seed threshold, categories, heads (H, W, stride, min_scale, generator seed)
DET_MULTI_CASES = [
    ('m2_p', 'planted', 0.5, 3, [(40, 40, 8, 0.0, 0), (20, 20, 16, 0.0, 100)]),
    ('m2_pms', 'planted', 0.2, 3, [(40, 40, 8, 64.0, 1), (20, 20, 16, 96.0, 101)]),
    ('m1_ums', 'uniform', 0.1, 2, [(40, 40, 8, 32.0, 2)]),
]


def gen_det_multi(op):
    """The reference CifDet decoder (and its CifDetHr / CifDetSeeds stages) over
    FieldConfigs of several detection heads and min scales (detm_<case>.npz)."""
    from openpifpaf.decoder import CifDet, CifDetHr, FieldConfig  # pylint: disable=import-outside-toplevel
    from openpifpaf.decoder.cif_seeds import CifDetSeeds, CifSeeds  # pylint: disable=import-outside-toplevel
    for name, gen, th, n_cat, heads in DET_MULTI_CASES:
        fields = [synthetic.det_batch(gen, 1, h, w, first_seed=seed, n_categories=n_cat)[0]
                  for h, w, _, _, seed in heads]
        fc = FieldConfig(cif_indices=list(range(len(heads))),
                         cif_strides=[st for _, _, st, _, _ in heads],
                         cif_min_scales=[ms for _, _, _, ms, _ in heads])
        CifSeeds.threshold = th
        hr = CifDetHr(fc).fill(fields).accumulated
        seeds = CifDetSeeds(hr, fc).fill(fields).get()
        anns = CifDet(fc, ['c%d' % i for i in range(n_cat)])(fields)
        out = {
            'gen': np.array(gen), 'seed_threshold': th, 'n_categories': n_cat,
            'heads': np.array(heads, np.float64),
            'input_sha': np.array([sha(f) for f in fields]),
            'cifhr_sha': np.array(sha(hr)), 'cifhr_sums': hr.sum(axis=(1, 2), dtype=np.float64),
            'seeds': np.array([[float(t) for t in sd] for sd in seeds], np.float32).reshape(-1, 6),
            'ann_field': np.array([a.field_i for a in anns], np.int64),
            'ann_score': np.array([a.score for a in anns], np.float32),
            'ann_bbox': np.array([a.bbox for a in anns], np.float32).reshape(-1, 4),
        }
        np.savez_compressed(os.path.join(HERE, 'detm_%s.npz' % name), **out)
        print('detm', name, 'seeds', len(seeds), 'anns', len(anns))
    CifSeeds.threshold = None


# initial_annotations (cifcaf.py:67-71,95-98): a decode of API_INIT_FIELDS grows three
# annotations derived from a decode of API_INIT_PREV first
API_INIT_FIELDS = dict(h=40, w=40, n_people=8, seed=5)
API_INIT_PREV = dict(h=40, w=40, n_people=8, seed=6)


def api_initial_annotations(prev_anns, annotation_cls, keypoints, skeleton):
    """Four tracking-style initial annotations, three from a previous decode: (0) the first
    annotation cut to joints 0-4, its decoding / frontier orders cut to match; (1) one joint
    of the second annotation, moved; (2) the third annotation shifted 4 px, orders cleared;
    (3) a weak lone joint that predict-mode NMS drops."""
    import copy  # pylint: disable=import-outside-toplevel
    a0 = copy.deepcopy(prev_anns[0])
    a0.data[5:] = 0.0
    a0.joint_scales[5:] = 0.0
    a0.decoding_order = [e for e in a0.decoding_order if e[0] < 5 and e[1] < 5]
    a0.frontier_order = list(a0.frontier_order[:4])
    src = prev_anns[1]
    j = int(np.argmax(src.data[:, 2]))
    a1 = annotation_cls(keypoints, skeleton).add(j, (src.data[j, 0] + 3.0, src.data[j, 1] - 2.0,
                                                     0.6))
    a1.joint_scales[j] = src.joint_scales[j]
    a2 = copy.deepcopy(prev_anns[2])
    a2.data[a2.data[:, 2] > 0, 0] += 4.0
    a2.decoding_order = []
    a2.frontier_order = []
    # (3) a weak lone joint in the corner: score 3 * 0.05 / 23 < the predict-mode
    # instance_threshold, so nms.Keypoints drops it there after editing it in place
    a3 = annotation_cls(keypoints, skeleton).add(0, (1.0, 1.0, 0.05))
    a3.joint_scales[0] = 2.0
    return [a0, a1, a2, a3]


def gen_api(op):
    """Drop-in API surface beyond the default decode: initial_annotations, the stage
    classes' min-scale / seed-mask / distance arguments, repeated fill_caf / fill_cif calls
    and fill_multiple over three heads or into an existing map."""
    from openpifpaf import decoder  # pylint: disable=import-outside-toplevel
    from openpifpaf.annotation import Annotation  # pylint: disable=import-outside-toplevel
    from openpifpaf.decoder import CafScored, CifCaf, CifHr, CifSeeds, FieldConfig  # pylint: disable=import-outside-toplevel
    kps, skel = constants.COCO_KEYPOINTS, list(constants.COCO_PERSON_SKELETON)
    for mode in ('eval', 'predict'):
        configure(decoder, mode, {})
        fc = FieldConfig()
        pc, pa = synthetic.planted(API_INIT_PREV['h'], API_INIT_PREV['w'],
                                   n_people=API_INIT_PREV['n_people'], seed=API_INIT_PREV['seed'])
        prev = CifCaf(fc, keypoints=kps, skeleton=skel)([pc, pa])
        init = api_initial_annotations(prev, Annotation, kps, skel)
        ins = ann_arrays(init, len(skel))  # before the decode mutates them
        ins['ann_n_decoding'] = np.array([len(a.decoding_order) for a in init], np.int64)
        ins['ann_n_frontier'] = np.array([len(a.frontier_order) for a in init], np.int64)
        cif, caf = synthetic.planted(API_INIT_FIELDS['h'], API_INIT_FIELDS['w'],
                                     n_people=API_INIT_FIELDS['n_people'],
                                     seed=API_INIT_FIELDS['seed'])
        ids = {id(a): i for i, a in enumerate(init)}
        anns = CifCaf(fc, keypoints=kps, skeleton=skel)([cif, caf], initial_annotations=init)
        out = {'mode': np.array(mode), 'input_sha': np.array(sha(cif, caf)),
               'prev_sha': np.array(sha(pc, pa)),
               'init_index': np.array([ids.get(id(a), -1) for a in anns], np.int64)}
        out.update({'init_' + k[4:]: v for k, v in ins.items()})
        out.update(ann_arrays(anns, len(skel)))
        # every initial object after the call, also those NMS dropped (the reference edits
        # them in place before filtering, nms.py:20-53)
        fin = ann_arrays(init, len(skel))
        fin['ann_n_decoding'] = np.array([len(a.decoding_order) for a in init], np.int64)
        fin['ann_n_frontier'] = np.array([len(a.frontier_order) for a in init], np.int64)
        out.update({'final_' + k[4:]: v for k, v in fin.items()})
        np.savez_compressed(os.path.join(HERE, 'api_initial_%s.npz' % mode), **out)
        print('api initial', mode, len(prev), '->', len(anns), 'init at',
              out['init_index'][out['init_index'] >= 0].tolist())

    # FieldConfig.seed_mask through the whole decode (cif_seeds.py:28-29, 63)
    mask = [f % 4 != 2 for f in range(17)]
    for mode in ('eval', 'predict'):
        configure(decoder, mode, {})
        cif, caf = synthetic.planted(40, 40, n_people=8, seed=5)
        anns = CifCaf(FieldConfig(seed_mask=mask), keypoints=kps, skeleton=skel)([cif, caf])
        out = {'mode': np.array(mode), 'input_sha': np.array(sha(cif, caf)),
               'seed_mask': np.array(mask)}
        out.update(ann_arrays(anns, len(skel)))
        np.savez_compressed(os.path.join(HERE, 'api_seedmask_%s.npz' % mode), **out)
        print('api seed_mask', mode, len(anns))

    configure(decoder, 'eval', {})
    fc = FieldConfig()
    heads = synthetic.planted_multi(321, 321, [8, 16, 16, 16], n_people=5, seed=21)
    (cif, caf), (c16a, a16), (c16b, _), (c16c, _) = heads
    out = {'input_sha': np.array(sha(*[f for hd in heads for f in hd]))}

    def hr_entry(tag, hr):
        out[tag + '_sha'] = np.array(sha(hr))
        out[tag + '_sums'] = hr.astype(np.float64).sum(axis=(1, 2))
        out[tag + '_shape'] = np.array(hr.shape)

    hr = CifHr(fc).fill_cif(cif, 8).accumulated
    hr_entry('hr_base', hr)
    hr_entry('hr_minscale', CifHr(fc).fill_cif(cif, 8, min_scale=12.0).accumulated)
    h2 = CifHr(fc).fill_cif(cif, 8)
    h2.fill_multiple([c16a, c16b, c16c], 16, min_scale=10.0)
    hr_entry('hr_into', h2.accumulated)
    hr_entry('hr_three', CifHr(fc).fill_multiple([c16a, c16b, c16c], 16).accumulated)

    def seed_arr(seeds):
        return np.array([[float(t) for t in sd] for sd in seeds], np.float32).reshape(-1, 5)

    mask = [f % 3 != 1 for f in range(17)]
    out['seed_mask'] = np.array(mask)
    out['seeds_masked'] = seed_arr(CifSeeds(hr, fc).fill_cif(cif, 8, min_scale=10.0,
                                                             seed_mask=mask).get())
    sd = CifSeeds(hr, fc).fill_cif(cif, 8)
    sd.fill_cif(c16a, 16, min_scale=12.0)
    out['seeds_two'] = seed_arr(sd.get())

    def caf_entry(tag, cs):
        out[tag + '_fwd_counts'] = np.array([f.shape[1] for f in cs.forward], np.int32)
        out[tag + '_bwd_counts'] = np.array([b.shape[1] for b in cs.backward], np.int32)
        out[tag + '_fwd_sha'] = np.array([sha(f) for f in cs.forward])
        out[tag + '_bwd_sha'] = np.array([sha(b) for b in cs.backward])

    caf_entry('caf_dist', CafScored(hr, fc, skel).fill_caf(caf, 8, min_distance=24.0,
                                                           max_distance=80.0))
    cs = CafScored(hr, fc, skel).fill_caf(caf, 8)
    cs.fill_caf(a16, 16, min_distance=20.0)
    caf_entry('caf_two', cs)
    caf_entry('caf_b_two', CafScored(hr, fc, skel, score_th=0.0001).fill_caf(caf, 8).fill_caf(
        a16, 16, max_distance=200.0))
    np.savez_compressed(os.path.join(HERE, 'api_stages.npz'), **out)
    print('api stages: seeds', len(out['seeds_masked']), len(out['seeds_two']),
          'caf', out['caf_two_fwd_counts'].sum())
    CifSeeds.threshold = None


# (name, generator, H, W, seed, mode, skeleton name, n_people, confidence_scales)
CONFSCALE_CASES = [
    ('p40_eval', 'planted', 40, 40, 6, 'eval', 'coco', 8,
     [0.5 + 0.37 * (i % 5) for i in range(19)]),
    ('u20_eval', 'uniform', 20, 20, 3, 'eval', 'coco', 8,
     [0.01 if i % 3 == 0 else 1.0 + 0.1 * i for i in range(19)]),
    # the dense-coupling weights factory.py:184-188 stores on the FieldConfig
    ('dense_p80_eval', 'planted', 80, 80, 7, 'eval', 'dense', 8, [1.0] * 19 + [0.01] * 25),
]


def gen_confscales(op):
    """CifCaf(confidence_scales=...) through the whole decode: the weights scale the
    frontier priorities of the seed loop's and force-complete's _grow."""
    from openpifpaf import decoder  # pylint: disable=import-outside-toplevel
    for name, gen, h, w, seed, mode, skel_name, n_people, scales in CONFSCALE_CASES:
        skeleton = list(SKELETONS[skel_name])
        configure(decoder, mode, {})
        cif, caf = make_inputs(gen, h, w, seed, skeleton, {'n_people': n_people})
        dec = decoder.CifCaf(decoder.FieldConfig(), keypoints=constants.COCO_KEYPOINTS,
                             skeleton=skeleton, out_skeleton=constants.COCO_PERSON_SKELETON,
                             confidence_scales=scales)
        anns = dec([cif, caf])
        out = {'generator': np.array(gen), 'H': h, 'W': w, 'seed': seed, 'mode': np.array(mode),
               'skeleton': np.asarray(skeleton, np.int32), 'n_people': n_people,
               'confidence_scales': np.array(scales, np.float64),
               'connection_method': np.array('blend'), 'greedy': 0,
               'input_sha': np.array(sha(cif, caf))}
        out.update(ann_arrays(anns, len(skeleton)))
        np.savez_compressed(os.path.join(HERE, 'api_confscales_%s.npz' % name), **out)
        print('api confidence_scales', name, len(anns))
    decoder.CifSeeds.threshold = None


def caf_entries(out, tag, cs):
    out['caf_%s_fwd_counts' % tag] = np.array([f.shape[1] for f in cs.forward], np.int32)
    out['caf_%s_bwd_counts' % tag] = np.array([b.shape[1] for b in cs.backward], np.int32)
    out['caf_%s_fwd_sha' % tag] = np.array([sha(f) for f in cs.forward])
    out['caf_%s_bwd_sha' % tag] = np.array([sha(b) for b in cs.backward])


def gen_kc(op):
    """The reference decoder at keypoint counts and skeletons other than COCO's
    (tests/kc_util.py): per case one uniform 20x23 eval fixture and one planted predict
    fixture, 'max' and 'greedy' variants for two cases, and one ms2 multi-scale decode."""
    decoder = __import__('openpifpaf').decoder
    for fx in kc_util.fixture_list():
        name, tag, mode = fx
        k, skeleton = kc_util.case(name)
        kps = kc_util.keypoint_names(k)
        gen = {'u': 'uniform', 'p': 'planted'}[tag[0]]
        h, w = (int(t) for t in tag[1:].split('x'))
        extra = {'max': {'connection_method': 'max'}, 'greedy': {'greedy': True}}.get(mode, {})
        configure(decoder, mode if mode == 'predict' else 'eval', extra)
        seed = kc_util.UNIFORM_SEEDS.get(name, 0) if gen == 'uniform' else kc_util.PLANTED_SEED
        cif, caf, _ = kc_util.inputs(name, gen, h, w, seed)
        fc = decoder.FieldConfig()
        hr = decoder.CifHr(fc).fill([cif, caf]).accumulated
        seeds = decoder.CifSeeds(hr, fc).fill([cif, caf]).get()
        anns = decoder.CifCaf(fc, keypoints=kps, skeleton=skeleton)([cif, caf])
        out = {
            'case': np.array(name), 'K': k, 'generator': np.array(gen), 'H': h, 'W': w,
            'seed': seed, 'mode': np.array(mode if mode == 'predict' else 'eval'),
            'skeleton': np.asarray(skeleton, np.int32),
            'n_people': kc_util.PLANTED_OBJECTS,
            'connection_method': np.array(extra.get('connection_method', 'blend')),
            'greedy': int(extra.get('greedy', False)),
            'input_sha': np.array(sha(cif, caf)),
            'cifhr_sha': np.array(sha(hr)),
            'cifhr_field_sums': hr.astype(np.float64).sum(axis=(1, 2)),
            'seeds': np.array([tuple(float(t) for t in s) for s in seeds],
                              np.float32).reshape(-1, 5),
        }
        for t, th in (('a', None), ('b', 0.0001)):
            caf_entries(out, t, decoder.CafScored(hr, fc, skeleton, score_th=th).fill([cif, caf]))
        out.update(ann_arrays(anns, len(skeleton), k))
        np.savez_compressed(kc_util.fixture_path(fx), **out)
        print('kc %-28s seeds %5d  caf_a %6d  anns %4d  max frontier %3d' % (
            kc_util.fixture_id(fx), len(seeds), out['caf_a_fwd_counts'].sum(), len(anns),
            max([len(a.frontier_order) for a in anns], default=0)))

    name, multi, mode = kc_util.MULTI_FIXTURE
    k, skeleton = kc_util.case(name)
    fields, kw = kc_util.multi_case(name, multi)
    configure(decoder, mode, {})
    fc = decoder.FieldConfig(**kw)
    hr = decoder.CifHr(fc).fill(fields).accumulated
    seeds = decoder.CifSeeds(hr, fc).fill(fields).get()
    anns = decoder.CifCaf(fc, keypoints=kc_util.keypoint_names(k), skeleton=skeleton)(fields)
    out = {
        'case': np.array(name), 'K': k, 'name': np.array(multi), 'mode': np.array(mode),
        'skeleton': np.asarray(skeleton, np.int32),
        'connection_method': np.array('blend'), 'greedy': 0,
        'input_sha': np.array(sha(*fields)),
        'cifhr_sha': np.array(sha(hr)), 'cifhr_shape': np.array(hr.shape),
        'seeds': np.array([[float(t) for t in sd] for sd in seeds], np.float32).reshape(-1, 5),
    }
    for t, th in (('a', None), ('b', 0.0001)):
        caf_entries(out, t, decoder.CafScored(hr, fc, skeleton, score_th=th).fill(fields))
    out.update(ann_arrays(anns, len(skeleton), k))
    np.savez_compressed(kc_util.fixture_path(kc_util.MULTI_FIXTURE), **out)
    print('kc multi', name, multi, mode, hr.shape, 'seeds', len(seeds), 'anns', len(anns))
    decoder.CifSeeds.threshold = None


def main():
    op = ref_loader.load()
    import Cython  # pylint: disable=import-outside-toplevel
    meta = {
        'reference': '/root/reference openpifpaf ' + op.__version__,
        'numpy': np.__version__,
        'cython': Cython.__version__,
        'python': platform.python_version(),
        'machine': platform.processor() or platform.machine(),
        'numpy_simd': str(np.lib.introspect.opt_func_info(func_name='exp', signature='float32')
                          if hasattr(np.lib, 'introspect') else ''),
        'note': 'outputs of the reference decoder (functional.pyx built by oracle/build_ref.sh)',
    }
    with open(os.path.join(HERE, 'meta.json'), 'w') as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
    only = sys.argv[1:]
    if only == ['nms']:
        gen_nms(op)
        gen_nms_scored(op)
        return
    if only == ['heads']:
        gen_heads(op)
        return
    if only == ['inverse']:
        gen_inverse(op)
        return
    if only == ['multi']:
        gen_multi(op)
        return
    if only == ['api']:
        gen_api(op)
        gen_confscales(op)
        return
    if only == ['confscales']:
        gen_confscales(op)
        return
    if only == ['det']:
        gen_det(op)
        gen_det_nms(op)
        gen_det_multi(op)
        return
    if only == ['detm']:
        gen_det_multi(op)
        return
    if only == ['kc']:
        gen_kc(op)
        return
    gen_primitives(op)
    gen_errors()
    gen_nms(op)
    gen_nms_scored(op)
    gen_heads(op)
    gen_det(op)
    gen_det_nms(op)
    gen_det_multi(op)
    gen_inverse(op)
    gen_multi(op)
    gen_api(op)
    gen_confscales(op)
    gen_kc(op)
    for case in CASES:
        if only and case[0] not in only:
            continue
        run_case(op, *case)


if __name__ == '__main__':
    main()
