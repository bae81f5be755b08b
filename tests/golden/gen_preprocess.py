"""Writes tests/golden/preprocess.npz: the reference's eval preprocessing chain
(eval_coco.preprocess_factory: NormalizeAnnotations, RescaleAbsolute, CenterPad or
CenterPadTight, then EVAL_TRANSFORM) over seeded random uint8 images (data only).

  python tests/golden/gen_preprocess.py     (needs the reference; see oracle/ref_loader.py)

The reference's own NormalizeAnnotations, RescaleAbsolute (scipy.ndimage.zoom) and CenterPad /
CenterPadTight classes run on PIL images.  torchvision is not installed where this runs and
oracle/ref_loader.py stubs it, so THREE PIECES ARE RESTATED HERE, not run from torchvision
(nobody could compare them with torchvision itself; DESIGN.md says so):
  * torchvision.transforms.functional.pad(image, ltrb, fill): a constant-fill paste (tv_pad),
    installed into the stub module before the pad classes are called;
  * ToTensor: permute to (3, H, W), .float().div(255);
  * Normalize: .sub_(mean).div_(std) with float32 tensors.

Per case c<i>_: src (h, w, 3) uint8, long_edge (0: None), tight (0 / 1), u8 the padded image
before ToTensor, f32 the normalised tensor (3, H, W), and the meta's offset, scale, valid_area,
width_height.  anns_*: two input annotations of case ANNS_CASE and their transformed keypoints
and boxes.  `names` lists the case prefixes; row0 / col0 flag the cases whose last rescaled row
/ column is all 0 although the source holds no 0.  The generator asserts what the tests rely
on from the reference alone.
"""
import io
import os
import sys
import zipfile

import numpy as np
import PIL.Image
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, os.path.join(REPO, 'oracle'))

import ref_loader  # noqa: E402  pylint: disable=wrong-import-position

# source (h, w) -> long_edge; the last three were added for the conditions asserted below:
# a zero last row, a zero last column, and exact .5 ties (zoom 2 halves neighbours)
SIZES = [((43, 47), 98), ((11, 58), 127), ((85, 30), 17), ((26, 9), 121), ((16, 16), 16),
         ((2, 2), 33), ((37, 64), 33), ((8, 2), 26), ((2, 8), 26), ((9, 9), 17)]
NONE_CASE = (21, 35)  # tight padding with long_edge=None
ANNS_CASE = 'c0_'
MEAN = [0.485, 0.456, 0.406]
STD = [0.229, 0.224, 0.225]


def tv_pad(image, padding, fill=0):
    """torchvision.transforms.functional.pad for a PIL image, constant mode, (l, t, r, b)."""
    left, top, right, bottom = padding
    w, h = image.size
    out = PIL.Image.new(image.mode, (w + left + right, h + top + bottom), tuple(fill))
    out.paste(image, (left, top))
    return out


def to_tensor(image):
    """torchvision.transforms.ToTensor for a uint8 RGB PIL image."""
    return torch.from_numpy(np.asarray(image).copy()).permute(2, 0, 1).contiguous().float().div(255)


def normalize(tensor):
    """torchvision.transforms.Normalize(mean, std)."""
    mean = torch.as_tensor(MEAN, dtype=torch.float32)[:, None, None]
    std = torch.as_tensor(STD, dtype=torch.float32)[:, None, None]
    return tensor.clone().sub_(mean).div_(std)


def exact_ties(src, th, tw):
    """Interior pixels of the rescaled image whose exact rational bilinear value is k + 1/2."""
    h, w = src.shape[:2]
    dy, dx = th - 1, tw - 1
    ny = np.arange(th, dtype=np.int64) * (h - 1)
    nx = np.arange(tw, dtype=np.int64) * (w - 1)
    y0, ry = ny // dy, ny % dy
    x0, rx = nx // dx, nx % dx
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    s = src.astype(np.int64)
    wy0, wy1 = (dy - ry)[:, None, None], ry[:, None, None]
    wx0, wx1 = (dx - rx)[None, :, None], rx[None, :, None]
    num = (s[y0][:, x0] * wy0 * wx0 + s[y0][:, x1] * wy0 * wx1 +
           s[y1][:, x0] * wy1 * wx0 + s[y1][:, x1] * wy1 * wx1)
    den = dy * dx
    tie = ((2 * num) % den == 0) & (((2 * num) // den) % 2 == 1)
    return int(tie[1:-1, 1:-1].sum())


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (reproducible bytes)."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name, arr in arrays.items():
            buf = io.BytesIO()
            np.save(buf, np.asarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    op = ref_loader.load()
    transforms = op.transforms
    sys.modules['torchvision.transforms.functional'].pad = tv_pad

    rng = np.random.default_rng(20251)
    out, names, row0, col0 = {}, [], [], []
    ties = 0
    lefts = tops = 0
    cases = [(hw, le, tight) for hw, le in SIZES for tight in (0, 1)] + [(NONE_CASE, 0, 1)]
    sources = {}
    for i, ((h, w), long_edge, tight) in enumerate(cases):
        if ((h, w), long_edge) not in sources:  # CenterPad and CenterPadTight share the image
            sources[((h, w), long_edge)] = rng.integers(1, 256, (h, w, 3), dtype=np.uint8)
        src = sources[((h, w), long_edge)]
        chain = [transforms.NormalizeAnnotations()]
        if long_edge:
            chain.append(transforms.RescaleAbsolute(long_edge))
        chain.append(transforms.CenterPadTight(16) if tight else transforms.CenterPad(long_edge))
        pre = 'c%d_' % i
        anns = []
        if pre == ANNS_CASE:
            kps = rng.uniform(0, 40, (2, 17, 3)).astype(np.float64)
            kps[:, :, 2] = rng.integers(0, 3, (2, 17))
            boxes = rng.uniform(1, 30, (2, 4))
            anns = [{'keypoints': kps[a].reshape(-1).tolist(), 'bbox': boxes[a].tolist(),
                     'segmentation': [[0.0, 1.0]]} for a in range(2)]
            out['anns_in_keypoints'], out['anns_in_bbox'] = kps, boxes
        image, meta = PIL.Image.fromarray(src), None
        for t in chain:
            image, anns, meta = t(image, anns, meta)
        u8 = np.asarray(image).copy()
        f32 = normalize(to_tensor(image)).numpy()
        if pre == ANNS_CASE:
            assert all('segmentation' not in a for a in anns)
            out['anns_keypoints'] = np.stack([a['keypoints'] for a in anns])
            out['anns_bbox'] = np.stack([a['bbox'] for a in anns])
            out['anns_bbox_original'] = np.stack([a['bbox_original'] for a in anns])
            assert out['anns_keypoints'].dtype == np.float32 and out['anns_bbox'].dtype == np.float32
        out[pre + 'src'] = src
        out[pre + 'long_edge'] = np.int32(long_edge)
        out[pre + 'tight'] = np.int32(tight)
        out[pre + 'u8'] = u8
        out[pre + 'f32'] = f32
        for k in ('offset', 'scale', 'valid_area', 'width_height'):
            out[pre + k] = np.asarray(meta[k])
        assert meta['hflip'] is False and meta['rotation'] == {'angle': 0.0, 'width': None,
                                                               'height': None}
        names.append(pre)
        # what the tests rely on
        left, top = (int(round(-v)) for v in meta['offset'])
        va = meta['valid_area']
        th, tw = int(round(va[3])) + 1, int(round(va[2])) + 1
        region = u8[top:top + th, left:left + tw]
        r0 = bool((region[-1] == 0).all())
        c0 = bool((region[:, -1] == 0).all())
        assert src.min() > 0
        row0.append(r0)
        col0.append(c0)
        lefts += left > 0
        tops += top > 0
        if long_edge and not tight:
            ties += exact_ties(src, th, tw)
        print(pre, (h, w), long_edge, 'tight' if tight else 'pad', u8.shape, 'ltrb', left, top,
              'row0' if r0 else '', 'col0' if c0 else '')
    out['names'] = np.asarray(names)
    out['row0'] = np.asarray(row0)
    out['col0'] = np.asarray(col0)
    assert any(row0) and any(col0) and any(not r and not c for r, c in zip(row0, col0))
    assert ties >= 20, ties
    assert lefts and tops
    path = os.path.join(HERE, 'preprocess.npz')
    save_npz(path, out)
    print('wrote', path, os.path.getsize(path), 'bytes;', ties, 'exact ties')


if __name__ == '__main__':
    main()
