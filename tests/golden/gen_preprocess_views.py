"""Writes tests/golden/preprocess_views.npz: the reference's eval preprocessing with its options
(eval_coco.preprocess_factory with extended_scale and orientation_invariant) and the reduced
and mirrored inputs nets.ShellMultiScale.forward makes, over seeded random uint8 images (data
only).

  python tests/golden/gen_preprocess_views.py     (needs the reference; oracle/ref_loader.py)

The reference's own NormalizeAnnotations, RescaleAbsolute, CenterPad / CenterPadTight,
DeterministicEqualChoice and RotateBy90 run on PIL images, chained as eval_coco.py:357-384
chains them.  ShellMultiScale.forward (nets.py:111-143) runs with an identity base_net, head
modules that only record their input and pass-through hflip modules, so that the recorded
tensors are the ten inputs the base net would see, in the order it would see them.  As in
gen_preprocess.py, torchvision's pad, ToTensor and Normalize are restated (tv_pad, to_tensor,
normalize, imported from it).  nets.py:118-123 indexes with torch.ByteTensor masks, which the
installed torch may refuse; then those lines are restated with bool masks (`restated_masks` in
the file says which happened).

Keys.  `pyr_names`: prefixes p<i>_ of the pyramid cases (CenterPad at L): src, long_edge, u8
(the L x L x 3 canvas), v0 .. v9 (float32 (3, n, n) views).  The turn / extended-scale cases are stacked, one row per
case: turn_long_edge, turn_tight, turn_ext, turn_ori, turn_image_id, turn_offset, turn_scale,
turn_valid_area, turn_width_height, turn_rotation (angle, width, height; 0, -1, -1 when not
turned), turn_u8_shape and turn_u8 (the canvases after the turn, flattened one after the
other), turn_f32 (the float32 tensors of the cases with long_edge turn_f32_edge, likewise);
the sources are shared per long_edge (s<L>_src).
`all_`: all three modes at L = 29: src, image_id, u8, v0 .. v9 and the meta keys.
anns_*: two input annotations, their results through a turned case (`anns_turned_*`) and a half-scale case (`anns_half_*`), and for the same metas the
reference's Preprocess.annotations_inverse of two decoded-style annotations (inv_in_*,
inv_turned_*, inv_half_*).  The generator asserts what the tests rely on from the reference
alone.
"""
import os
import sys
import types

import numpy as np
import PIL.Image
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, os.path.join(REPO, 'oracle'))
sys.path.insert(0, HERE)

import ref_loader  # noqa: E402  pylint: disable=wrong-import-position
from gen_preprocess import normalize, save_npz, to_tensor, tv_pad  # noqa: E402  pylint: disable=wrong-import-position

# long_edge -> source (h, w): L mod 3 = 0, 1, 2, L mod 5 = 0 and != 0, even and odd, canvases
# of 1, 2 and 3 workgroup tiles; (8, 2) -> 26 is gen_preprocess.py's black-last-row source
PYRAMID = [(16, (11, 7)), (17, (9, 14)), (26, (8, 2)), (29, (13, 20)), (30, (21, 10)),
           (33, (37, 64)), (47, (31, 22))]
TURN_EDGES = {16: (11, 7), 17: (9, 14), 33: (37, 64)}
IDS = range(1, 9)
# (extended_scale, orientation_invariant, tight_padding)
RUNS = [(0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 0)]
ALL_EDGE, ALL_SRC, ALL_ID = 29, (13, 20), 2
ANNS_EDGE, ANNS_ID = 33, 2
F32_EDGE = 16  # turn cases whose float32 tensor is stored too
META_KEYS = ('offset', 'scale', 'valid_area', 'width_height')


def chain(transforms, long_edge, tight, ext, ori):
    """eval_coco.py:357-384 without EVAL_TRANSFORM."""
    pre = [transforms.NormalizeAnnotations()]
    if ext:
        pre.append(transforms.DeterministicEqualChoice([
            transforms.RescaleAbsolute(long_edge),
            transforms.RescaleAbsolute((long_edge - 1) // 2 + 1)], salt=1))
    else:
        pre.append(transforms.RescaleAbsolute(long_edge))
    pre.append(transforms.CenterPadTight(16) if tight else transforms.CenterPad(long_edge))
    if ori:
        pre.append(transforms.DeterministicEqualChoice([
            None, transforms.RotateBy90(fixed_angle=90), transforms.RotateBy90(fixed_angle=180),
            transforms.RotateBy90(fixed_angle=270)], salt=3))
    return pre


def run(pre, src, anns, meta):
    image = PIL.Image.fromarray(src)
    for t in pre:
        image, anns, meta = t(image, anns, meta)
    return image, anns, meta


class Recorder(torch.nn.Module):
    def __init__(self, meta, seen):
        super().__init__()
        self.meta, self.seen = meta, seen

    def forward(self, x):  # pylint: disable=arguments-differ
        self.seen.append(x)
        return (x,)


class PassThrough(torch.nn.Module):
    def forward(self, *args):  # pylint: disable=arguments-differ
        return args


def pyramid(op, tensor, restated):
    """The ten inputs ShellMultiScale.forward hands its base net for a (1, 3, L, L) input."""
    nets = op.network.nets
    kps, skel = op.datasets.constants.COCO_KEYPOINTS, op.datasets.constants.COCO_PERSON_SKELETON
    seen = []
    meta = types.SimpleNamespace(keypoints=kps, skeleton=skel)
    shell = nets.ShellMultiScale(torch.nn.Identity(), [Recorder(meta, seen) for _ in range(3)],
                                 include_hflip=True)
    shell.pif_hflip = shell.paf_hflip = shell.paf_hflip_dense = PassThrough()
    try:
        shell(tensor)
    except (IndexError, RuntimeError, TypeError):
        # nets.py:118-123 with bool masks where torch no longer indexes with uint8 masks
        restated.append(True)
        del seen[:]
        for hflip in (False, True):
            for reduction in [1, 1.5, 2, 3, 5]:
                if reduction == 1.5:
                    x_red = torch.tensor([i % 3 != 2 for i in range(tensor.shape[3])])
                    y_red = torch.tensor([i % 3 != 2 for i in range(tensor.shape[2])])
                    reduced = tensor[:, :, y_red, :]
                    reduced = reduced[:, :, :, x_red]
                else:
                    reduced = tensor[:, :, ::reduction, ::reduction]
                if hflip:
                    reduced = torch.flip(reduced, dims=[3])
                seen.extend([reduced] * 3)
    assert len(seen) == 30
    views = [seen[3 * v] for v in range(10)]
    for v in range(10):
        assert all(torch.equal(seen[3 * v + k], views[v]) for k in range(3))
    return [v[0].contiguous().numpy() for v in views]


def rotation_triple(meta):
    r = meta['rotation']
    if r['angle'] == 0.0:
        assert r['width'] is None and r['height'] is None
        return np.array((0.0, -1.0, -1.0))
    return np.array((r['angle'], r['width'], r['height']), np.float64)


def store_meta(out, pre, meta):
    for k in META_KEYS:
        out[pre + k] = np.asarray(meta[k])
    out[pre + 'rotation'] = rotation_triple(meta)
    assert meta['hflip'] is False


def main():
    op = ref_loader.load()
    transforms = op.transforms
    sys.modules['torchvision.transforms.functional'].pad = tv_pad
    rng = np.random.default_rng(20252)
    out, restated = {}, []

    # ---- pyramid ----
    names, lefts, tops, black_view = [], 0, 0, 0
    for i, (long_edge, (h, w)) in enumerate(PYRAMID):
        pre = 'p%d_' % i
        src = rng.integers(1, 256, (h, w, 3), dtype=np.uint8)
        image, _, meta = run(chain(transforms, long_edge, 0, 0, 0), src, [], None)
        u8 = np.asarray(image).copy()
        assert u8.shape == (long_edge, long_edge, 3)
        views = pyramid(op, normalize(to_tensor(image))[None], restated)
        out[pre + 'src'], out[pre + 'long_edge'], out[pre + 'u8'] = src, np.int32(long_edge), u8
        for v, arr in enumerate(views):
            assert arr.dtype == np.float32
            out[pre + 'v%d' % v] = arr
        left, top = (int(round(-v)) for v in meta['offset'])
        lefts += left > 0
        tops += top > 0
        th, tw = (int(round(meta['valid_area'][k])) + 1 for k in (3, 2))
        last = top + th - 1
        if (u8[last, left:left + tw] == 0).all():
            # the black last rescaled row in a reduced view that keeps it
            zero = normalize(torch.zeros(3, 1, 1)).numpy().reshape(3, 1)
            for v, r in ((2, 2), (3, 3), (4, 5)):
                xs = np.array([x for x in range(left, left + tw) if x % r == 0])
                if last % r == 0 and len(xs):
                    black_view += int((views[v][:, last // r, xs // r] == zero).all())
        names.append(pre)
        print(pre, long_edge, (h, w), 'ltrb', left, top, [a.shape[1] for a in views[:5]])
    out['pyr_names'] = np.asarray(names)
    edges = [e for e, _ in PYRAMID]
    assert {e % 3 for e in edges} == {0, 1, 2} and any(e % 5 == 0 for e in edges)
    assert any(e % 5 for e in edges) and {e % 2 for e in edges} == {0, 1}
    assert {-(-e * e // 1024) for e in edges} == {1, 2, 3}
    assert lefts and tops and black_view, (lefts, tops, black_view)

    # ---- turns and extended scale ----
    angles, scales_seen, same = set(), set(), 0
    sources = {}
    for long_edge, (h, w) in TURN_EDGES.items():
        sources[long_edge] = rng.integers(1, 256, (h, w, 3), dtype=np.uint8)
        out['s%d_src' % long_edge] = sources[long_edge]
    rows = {k: [] for k in ('long_edge', 'tight', 'ext', 'ori', 'image_id', 'u8_shape', 'u8',
                            'f32', 'rotation') + META_KEYS}
    for long_edge in TURN_EDGES:
        src = sources[long_edge]
        for ext, ori, tight in RUNS:
            for image_id in IDS:
                image, _, meta = run(chain(transforms, long_edge, tight, ext, ori), src, [],
                                     {'image_id': image_id})
                u8 = np.asarray(image).copy()
                for k, v in (('long_edge', long_edge), ('tight', tight), ('ext', ext),
                             ('ori', ori), ('image_id', image_id), ('u8_shape', u8.shape),
                             ('u8', u8.reshape(-1)), ('rotation', rotation_triple(meta))):
                    rows[k].append(v)
                if long_edge == F32_EDGE:
                    rows['f32'].append(normalize(to_tensor(image)).numpy().reshape(-1))
                for k in META_KEYS:
                    rows[k].append(np.asarray(meta[k]))
                assert meta['hflip'] is False
                angle = meta['rotation']['angle']
                if ori and not ext:
                    angles.add(int(angle))
                if ext:
                    scales_seen.add(int(round(max(meta['valid_area'][2:]))) + 1)
                if angle:
                    flat, _, _ = run(chain(transforms, long_edge, tight, ext, 0), src, [],
                                     {'image_id': image_id})
                    same += int(np.array_equal(np.asarray(flat), u8))
                    assert meta['rotation']['width'] == meta['rotation']['height'] == long_edge
        half = (long_edge - 1) // 2 + 1
        assert {long_edge, half} <= scales_seen, (long_edge, scales_seen)
    for k in ('long_edge', 'tight', 'ext', 'ori', 'image_id', 'u8_shape'):
        out['turn_' + k] = np.asarray(rows[k], np.int32)
    for k in ('rotation',) + META_KEYS:
        out['turn_' + k] = np.stack(rows[k])
        assert out['turn_' + k].dtype == (np.int64 if k == 'width_height' else np.float64), k
    out['turn_u8'] = np.concatenate(rows['u8'])
    out['turn_f32'] = np.concatenate(rows['f32'])
    out['turn_f32_edge'] = np.int32(F32_EDGE)
    assert angles == {0, 90, 180, 270}, angles
    assert same == 0  # no turned canvas equals its unturned one

    # ---- all three modes ----
    src = rng.integers(1, 256, ALL_SRC + (3,), dtype=np.uint8)
    image, _, meta = run(chain(transforms, ALL_EDGE, 0, 1, 1), src, [], {'image_id': ALL_ID})
    assert meta['rotation']['angle'] == 90 and max(meta['valid_area'][2:]) < ALL_EDGE // 2 + 1
    out['all_src'], out['all_image_id'] = src, np.int32(ALL_ID)
    out['all_long_edge'] = np.int32(ALL_EDGE)
    out['all_u8'] = np.asarray(image).copy()
    for v, arr in enumerate(pyramid(op, normalize(to_tensor(image))[None], restated)):
        out['all_v%d' % v] = arr
    store_meta(out, 'all_', meta)

    # ---- annotations forward and inverse ----
    kps = rng.uniform(0, 30, (2, 17, 3)).astype(np.float64)
    kps[:, :, 2] = rng.integers(0, 3, (2, 17))
    boxes = rng.uniform(1, 25, (2, 4))
    out['anns_in_keypoints'], out['anns_in_bbox'] = kps, boxes
    Annotation = op.annotation.Annotation
    c = op.datasets.constants
    inv_data = rng.uniform(0, ANNS_EDGE - 1, (2, 17, 3)).astype(np.float32)
    inv_scales = rng.uniform(0.5, 4, (2, 17)).astype(np.float32)
    inv_dxyv = rng.uniform(0, ANNS_EDGE - 1, (2, 3, 6)).astype(np.float32)
    out['inv_in_data'], out['inv_in_scales'], out['inv_in_dxyv'] = inv_data, inv_scales, inv_dxyv
    src = sources[ANNS_EDGE]
    for label, (ext, ori) in (('turned', (0, 1)), ('half', (1, 0))):
        anns = [{'keypoints': kps[a].reshape(-1).tolist(), 'bbox': boxes[a].tolist(),
                 'segmentation': [[0.0, 1.0]]} for a in range(2)]
        _, got, meta = run(chain(transforms, ANNS_EDGE, 0, ext, ori), src, anns,
                           {'image_id': ANNS_ID})
        if ori:
            assert meta['rotation']['angle'] == 90
        else:
            assert max(meta['valid_area'][2:]) < ANNS_EDGE // 2 + 1
        for key in ('keypoints', 'bbox', 'bbox_original'):
            out['anns_%s_%s' % (label, key)] = np.stack([a[key] for a in got])
        assert out['anns_%s_keypoints' % label].dtype == np.float32
        assert out['anns_%s_bbox' % label].dtype == np.float32
        store_meta(out, 'anns_%s_' % label, meta)
        decoded = []
        for a in range(2):
            ann = Annotation(c.COCO_KEYPOINTS, c.COCO_PERSON_SKELETON)
            ann.data = inv_data[a].copy()
            ann.joint_scales = inv_scales[a].copy()
            ann.decoding_order = [(t, t + 1, inv_dxyv[a, t, :3].copy(), inv_dxyv[a, t, 3:].copy())
                                  for t in range(3)]
            decoded.append(ann)
        inv = transforms.Preprocess.annotations_inverse(decoded, meta)
        out['inv_%s_data' % label] = np.stack([a.data for a in inv])
        out['inv_%s_scales' % label] = np.stack([a.joint_scales for a in inv])
        o = np.zeros_like(inv_dxyv)
        for a, ann in enumerate(inv):
            for t, (_, __, c1, c2) in enumerate(ann.decoding_order):
                o[a, t, :3], o[a, t, 3:] = c1[:3], c2[:3]
        out['inv_%s_dxyv' % label] = o
        assert out['inv_%s_data' % label].dtype == np.float32
    out['anns_long_edge'], out['anns_image_id'] = np.int32(ANNS_EDGE), np.int32(ANNS_ID)
    out['restated_masks'] = np.bool_(bool(restated))

    path = os.path.join(HERE, 'preprocess_views.npz')
    save_npz(path, out)
    size = os.path.getsize(path)
    print('wrote', path, size, 'bytes; masks restated:', bool(restated))
    assert size <= os.path.getsize(os.path.join(HERE, 'preprocess.npz'))


if __name__ == '__main__':
    main()
