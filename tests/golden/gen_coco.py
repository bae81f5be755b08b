"""Writes tests/golden/coco_records.npz: EvalCoco.from_predictions (eval_coco.py:108-158) of
the reference over reference-decoded poses and detections (data only).

  python tests/golden/gen_coco.py        (needs the reference; see oracle/ref_loader.py)

Two groups of images, one swap table each (a batch shares one):
  coco    planted 33x40, uniform 20x23 and all-zero 20x23 eval decodes (COCO skeleton)
  chain5  a uniform 20x23 eval decode of tests/kc_util.py's chain5 (K = 5)
Every source image appears once per meta of gen_golden.inverse_metas (shift, flip with
_HorizontalSwap, rot), each with its own image_id.  Per group the file holds the source
records (data, joint scales, score), the batch (source index, meta fields, image ids, swap
table) and, per parameter set (max_per_image 20 / 3 / 1 x small_threshold 0 / one of the
reference's scale(v_th=0.01) results over the group's uniform image, see gen_group), json.dumps of the list
from_predictions appended over the batch.  `route` says how that list was made: 'EvalCoco'
when the reference's eval_coco module imports here (with stub modules for what this host
lacks), else 'per-annotation' (the reference's annotations_inverse, scale and json_data per
annotation, filter / cap / dummy restated).  Detections: the det_* arrays of inverse.npz are
the inputs; their expected records for caps 20 and 1 under the three metas are stored here.
The generator checks that the reference alone meets the conditions the tests rely on.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden  # noqa: E402  pylint: disable=wrong-import-position
from gen_golden import configure, inverse_metas, kc_util, make_inputs, ref_loader  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd import constants  # noqa: E402  pylint: disable=wrong-import-position

CAPS = (20, 3, 1)
META_NAMES = ('shift', 'flip', 'rot')
CHAIN5_HFLIP = {'kp1': 'kp5', 'kp5': 'kp1', 'kp2': 'kp4', 'kp4': 'kp2'}


def dumps(preds):
    """json.dumps without the spaces after the separators (the fixture stays small)."""
    return json.dumps(preds, separators=(',', ':'))


def import_eval_coco():
    """The reference's eval_coco module, or None: thop, PIL and the matplotlib-bound show /
    visualizer modules are stubbed when missing (from_predictions touches none of them)."""
    for name in ('thop', 'PIL', 'PIL.Image', 'matplotlib', 'matplotlib.pyplot', 'scipy',
                 'scipy.ndimage'):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    try:
        from openpifpaf import eval_coco  # pylint: disable=import-outside-toplevel
        return eval_coco
    except Exception as e:  # pylint: disable=broad-except
        print('openpifpaf.eval_coco does not import here:', type(e).__name__, e)
        return None


def per_annotation(anns, meta, small_threshold, max_per_image):
    """from_predictions' list from the reference's annotations_inverse, scale and json_data
    per annotation (the route without the eval_coco module)."""
    from openpifpaf import transforms  # pylint: disable=import-outside-toplevel
    preds = transforms.Preprocess.annotations_inverse(anns, meta)
    if small_threshold:
        preds = [p for p in preds if p.scale(v_th=0.01) >= small_threshold]
    preds = preds[:max_per_image]
    out = []
    for p in preds:
        d = p.json_data()
        d['image_id'] = int(meta['image_id'])
        out.append({k: v for k, v in d.items()
                    if k in ('category_id', 'score', 'keypoints', 'bbox', 'image_id')})
    if not out:
        out.append({'image_id': int(meta['image_id']), 'category_id': 1,
                    'keypoints': np.zeros((17 * 3,)).tolist(), 'bbox': [0, 0, 1, 1],
                    'score': 0.001})
    return out


def batch_predictions(eval_coco, images, small_threshold, max_per_image):
    """images: [(annotations, meta)] -> (the list from_predictions appended, route)."""
    if eval_coco is not None:
        ec = eval_coco.EvalCoco(None, None, max_per_image=max_per_image,
                                small_threshold=small_threshold)
        for anns, meta in images:
            ec.from_predictions(anns, meta)
        return ec.predictions, 'EvalCoco'
    out = []
    for anns, meta in images:
        out += per_annotation(anns, meta, small_threshold, max_per_image)
    return out, 'per-annotation'


def meta_arrays(metas):
    rot = [m['rotation'] for m in metas]
    return {
        'offset': np.array([m['offset'] for m in metas], np.float64),
        'scale': np.array([m['scale'] for m in metas], np.float64),
        'rotation_angle': np.array([r['angle'] for r in rot], np.float64),
        'rotation_width': np.array([r['width'] or 0.0 for r in rot], np.float64),
        'rotation_height': np.array([r['height'] or 0.0 for r in rot], np.float64),
        'width': np.array([m['width_height'][0] for m in metas], np.float64),
        'hflip': np.array([int(m['hflip']) for m in metas], np.int32),
        'image_id': np.array([m['image_id'] for m in metas], np.int64),
    }


def swap_table(swap, k):
    probe = np.repeat(np.arange(1, k + 1, dtype=np.float64)[:, None], 3, axis=1)
    out = np.asarray(swap(probe))
    table = np.zeros(k, np.int32)
    for t in range(k):
        table[int(round(out[t, 0])) - 1] = t
    return table


def gen_group(out, conds, eval_coco, tag, k, sources, swap, uniform_i, first_id):
    """sources: [annotation list]; every source under every meta is one batch image."""
    from openpifpaf import transforms  # pylint: disable=import-outside-toplevel
    metas_by_name = inverse_metas(swap)
    images, src_of = [], []
    for mi, name in enumerate(META_NAMES):
        for si, anns in enumerate(sources):
            images.append((anns, dict(metas_by_name[name],
                                      image_id=first_id + 10 * mi + si)))
            src_of.append(si)
    cap = max(1, max(len(a) for a in sources))
    data = np.zeros((len(sources), cap, k, 3), np.float32)
    scales = np.zeros((len(sources), cap, k), np.float32)
    score = np.zeros((len(sources), cap), np.float64)
    for si, anns in enumerate(sources):
        for r, a in enumerate(anns):
            data[si, r], scales[si, r], score[si, r] = a.data, a.joint_scales, a.score()
    out[tag + '_K'] = k
    out[tag + '_src_data'], out[tag + '_src_scales'], out[tag + '_src_score'] = data, scales, score
    out[tag + '_src_counts'] = np.array([len(a) for a in sources], np.int32)
    out[tag + '_img_src'] = np.array(src_of, np.int32)
    for key, v in meta_arrays([m for _, m in images]).items():
        out[tag + '_meta_' + key] = v
    out[tag + '_hswap'] = swap_table(swap, k)
    # the threshold: one of the reference's own scales of the group's uniform image under
    # the shift meta.  coco: the largest, so that this image keeps one pose under the shift
    # meta and none under the rot meta, whose scale factors shrink it (the dummy record);
    # chain5: the middle one of the non-zero scales (many poses have a single joint above
    # 0.01 and so the scale 0.0), which no image loses every pose to
    inv = transforms.Preprocess.annotations_inverse(sources[uniform_i], metas_by_name['shift'])
    pos = np.sort([s for s in (a.scale(v_th=0.01) for a in inv) if s > 0])
    threshold = float(pos[-1] if k == 17 else pos[len(pos) // 2])
    out[tag + '_small_threshold'] = threshold
    for th_i, th in enumerate((0.0, threshold)):
        for cap_ in CAPS:
            preds, route = batch_predictions(eval_coco, images, th, cap_)
            out['%s_json_t%d_m%d' % (tag, th_i, cap_)] = np.array(dumps(preds))
            out['route'] = np.array(route)
        for anns, meta in images:  # the conditions, from the reference alone
            inv = transforms.Preprocess.annotations_inverse(anns, meta)
            left = [a for a in inv if not th or a.scale(v_th=0.01) >= th]
            if th and 0 < len(left) < len(inv):
                conds['some'] += 1
            if th and inv and not left:
                conds['all'] += 1
                assert k == 17, 'the dummy of a K != 17 image differs from the reference'
            if len(left) > min(CAPS):
                conds['cap'] += 1
            if meta['hflip'] and inv:
                conds['flip'] += 1
            if meta['rotation']['angle'] and inv:
                conds['rot'] += 1
    print(tag, 'images', len(images), 'records', [len(a) for a in sources], 'threshold',
          threshold)


def main():
    op = ref_loader.load()
    from openpifpaf.decoder import CifCaf, FieldConfig  # pylint: disable=import-outside-toplevel
    from openpifpaf.datasets import constants as dc  # pylint: disable=import-outside-toplevel
    from openpifpaf.transforms.hflip import _HorizontalSwap  # pylint: disable=import-outside-toplevel
    from openpifpaf.annotation import AnnotationDet  # pylint: disable=import-outside-toplevel
    eval_coco = import_eval_coco()
    configure(op.decoder, 'eval', {})
    kps, skel = constants.COCO_KEYPOINTS, list(constants.COCO_PERSON_SKELETON)
    sources = []
    for gen, h, w in (('planted', 33, 40), ('uniform', 20, 23), ('zero', 20, 23)):
        cif, caf = make_inputs(gen, h, w, 0, skel, {})
        sources.append(CifCaf(FieldConfig(), keypoints=kps, skeleton=skel)([cif, caf]))
    out, conds = {}, dict(some=0, all=0, cap=0, flip=0, rot=0)
    gen_group(out, conds, eval_coco, 'coco', 17, sources, _HorizontalSwap(kps, dc.HFLIP), 1, 1000)
    k5, skel5 = kc_util.case('chain5')
    cif, caf, _ = kc_util.inputs('chain5', 'uniform', 20, 23)
    kps5 = kc_util.keypoint_names(k5)
    anns5 = CifCaf(FieldConfig(), keypoints=kps5, skeleton=skel5)([cif, caf])
    gen_group(out, conds, eval_coco, 'chain5', k5, [anns5], _HorizontalSwap(kps5, CHAIN5_HFLIP),
              0, 2000)
    assert all(conds.values()), conds
    print('conditions', conds, 'route', out['route'])

    # detections: inverse.npz's det_* records under the three metas
    with np.load(os.path.join(HERE, 'inverse.npz')) as z:
        field, dscore, bbox = z['det_field'], z['det_score'], z['det_bbox']
    dets = [AnnotationDet(['c0', 'c1', 'c2']).set(int(f), np.float32(s), b.astype(np.float32))
            for f, s, b in zip(field, dscore, bbox)]
    metas = inverse_metas(None)
    images = [(dets, dict(metas[name], image_id=3000 + i)) for i, name in enumerate(META_NAMES)]
    images.append(([], dict(metas['shift'], image_id=3003)))
    for key, v in meta_arrays([m for _, m in images]).items():
        out['det_meta_' + key] = v
    out['det_counts'] = np.array([len(a) for a, _ in images], np.int32)
    for cap_ in (20, 1):
        preds, _ = batch_predictions(eval_coco, images, 0.0, cap_)
        out['det_json_m%d' % cap_] = np.array(dumps(preds))
    op.decoder.CifSeeds.threshold = None
    path = os.path.join(HERE, 'coco_records.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    assert gen_golden.HERE == HERE
    main()
