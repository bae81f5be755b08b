"""eval_coco.preprocess_factory with its options, and the input pyramid of a multi-scale
model, on the device in one launch (pp_preprocess_views, csrc/preprocess.hip):

  * extended_scale (eval_coco.py:359-366): every image is rescaled to long_edge or to
    (long_edge - 1) // 2 + 1, chosen from its image id (DeterministicEqualChoice, salt 1);
  * orientation_invariant (eval_coco.py:376-384): the square padded image is turned by 0, 90,
    180 or 270 degrees, chosen from its image id (salt 3) and recorded in meta['rotation']
    (transforms/rotate.py:16-81 RotateBy90 with a fixed angle);
  * multi_scale / multi_scale_hflip (network/nets.py:111-131 ShellMultiScale.forward): the
    normalised input reduced by 1, 1.5, 2, 3 and 5 and the mirror images of those.

`EvalViews.batch` returns the input tensors (or the list of 5 or 10 view tensors, in the
order nets.py:115-116 runs them) and the reference's meta dicts; `batch_cpu` is the host twin
and is only ever used when called by name.  With every option off the results are
`EvalPreprocess.batch`'s.  The choices, the metas and the annotations are host work in Python
and NumPy float64 / float32 with exactly the reference's operations.
"""
import copy
import math

import numpy as np
import torch

from . import _device
from ._abi import PP_VIEW_ALL, PP_VIEW_R1
from ._lib import call, load
from .preprocess import _BILINEAR, _EvalChain, _Plan, _vp

SALT_SCALE, SALT_TURN = 1, 3  # eval_coco.py:365, 383


def equal_choice(meta, salt, n):
    """transforms/random.py:25-28 DeterministicEqualChoice: Python's own hash."""
    assert meta is not None and 'image_id' in meta and meta['image_id'] > 0
    return hash(meta['image_id'] + salt) % n


def view_sizes(n):
    """Edge of the five reduced inputs of an n x n input (nets.py:116-125): 1, 1.5, 2, 3, 5."""
    return [n, n - n // 3, -(-n // 2), -(-n // 3), -(-n // 5)]


def rotate_box(bbox, width, height, angle_degrees):
    """transforms/utils.py:5-28, operation for operation (cos and sin of the angle are not
    exactly 0 or 1 and are not simplified)."""
    cangle = math.cos(angle_degrees / 180.0 * math.pi)
    sangle = math.sin(angle_degrees / 180.0 * math.pi)
    four_corners = np.array([
        [bbox[0], bbox[1]],
        [bbox[0] + bbox[2], bbox[1]],
        [bbox[0], bbox[1] + bbox[3]],
        [bbox[0] + bbox[2], bbox[1] + bbox[3]],
    ])
    x_old = four_corners[:, 0].copy() - width/2
    y_old = four_corners[:, 1].copy() - height/2
    four_corners[:, 0] = width/2 + cangle * x_old + sangle * y_old
    four_corners[:, 1] = height/2 - sangle * x_old + cangle * y_old
    x = np.min(four_corners[:, 0])
    y = np.min(four_corners[:, 1])
    xmax = np.max(four_corners[:, 0])
    ymax = np.max(four_corners[:, 1])
    return np.array([x, y, xmax - x, ymax - y])


def turn_meta(meta, angle, w, h):
    """rotate.py:36-39 and 70-78 on a meta of a w x h image (a deep copy)."""
    meta = copy.deepcopy(meta)
    assert meta['rotation']['angle'] == 0.0
    meta['rotation']['angle'] = angle
    meta['rotation']['width'] = w
    meta['rotation']['height'] = h
    meta['valid_area'] = rotate_box(meta['valid_area'], w - 1, h - 1, angle)
    original_valid_area = meta['valid_area'].copy()
    meta['valid_area'][0] = np.clip(meta['valid_area'][0], 0, w)
    meta['valid_area'][1] = np.clip(meta['valid_area'][1], 0, h)
    new_rb_corner = original_valid_area[:2] + original_valid_area[2:]
    new_rb_corner[0] = np.clip(new_rb_corner[0], 0, w)
    new_rb_corner[1] = np.clip(new_rb_corner[1], 0, h)
    meta['valid_area'][2:] = new_rb_corner - meta['valid_area'][:2]
    return meta


def turn_anns(anns, angle, w, h):
    """rotate.py:59-67 on normalised annotations of a w x h image (a deep copy)."""
    anns = copy.deepcopy(anns)
    cangle = math.cos(angle / 180.0 * math.pi)
    sangle = math.sin(angle / 180.0 * math.pi)
    for ann in anns:
        xy = ann['keypoints'][:, :2]
        x_old = xy[:, 0].copy() - (w - 1)/2
        y_old = xy[:, 1].copy() - (h - 1)/2
        xy[:, 0] = (w - 1)/2 + cangle * x_old + sangle * y_old
        xy[:, 1] = (h - 1)/2 - sangle * x_old + cangle * y_old
        ann['bbox'] = rotate_box(ann['bbox'], w - 1, h - 1, angle)
    return anns


class _ViewPlan(_Plan):
    """One image through the chain: its sizes and its turn (`rot`, 0..3 quarter turns)."""

    def __init__(self, h, w, long_edge, tight, rescale_edge, rot):
        super().__init__(h, w, long_edge, tight, rescale_edge)
        self.rot = rot

    def meta(self, meta):
        meta = super().meta(meta)
        return turn_meta(meta, 90 * self.rot, self.W, self.H) if self.rot else meta

    def anns(self, anns):
        anns = super().anns(anns)
        return turn_anns(anns, 90 * self.rot, self.W, self.H) if self.rot else anns


class EvalViews(_EvalChain):
    """eval_coco.preprocess_factory(long_edge, tight_padding=..., extended_scale=...,
    orientation_invariant=...) for uint8 RGB images, and with multi_scale the reduced (and
    with multi_scale_hflip mirrored) inputs ShellMultiScale.forward makes of its result.

    dtype and channels_last as EvalPreprocess.  With extended_scale or orientation_invariant
    every meta needs an 'image_id' > 0 (the reference asserts it)."""

    def __init__(self, long_edge, *, tight_padding=False, extended_scale=False,
                 orientation_invariant=False, multi_scale=False, multi_scale_hflip=True,
                 dtype=torch.float32, channels_last=False, fast=False, resample=_BILINEAR):
        super().__init__(long_edge, tight_padding, dtype, channels_last, fast, resample)
        if orientation_invariant and tight_padding:
            raise NotImplementedError(
                'orientation_invariant with tight_padding: a non-square image is turned by '
                'scipy.ndimage.rotate (a spline), which is not restated')
        if multi_scale and tight_padding:
            raise NotImplementedError(
                'multi_scale with tight_padding: the reference never builds it '
                '(eval_coco.py:393)')
        if extended_scale:
            assert long_edge  # eval_coco.py:360
        self.extended_scale = bool(extended_scale)
        self.orientation_invariant = bool(orientation_invariant)
        self.multi_scale = bool(multi_scale)
        self.multi_scale_hflip = bool(multi_scale and multi_scale_hflip)
        self.reductions = PP_VIEW_ALL if self.multi_scale else PP_VIEW_R1
        if self.multi_scale:
            self._view_edges = view_sizes(self.long_edge) * (2 if self.multi_scale_hflip else 1)

    def _view_plan(self, h, w, meta):
        edge = None
        if self.extended_scale:
            edges = (self.long_edge, (self.long_edge - 1) // 2 + 1)
            edge = edges[equal_choice(meta, SALT_SCALE, 2)]
        rot = equal_choice(meta, SALT_TURN, 4) if self.orientation_invariant else 0
        return _ViewPlan(h, w, self.long_edge, self.tight_padding, edge, rot)

    def _args(self, src, src_bytes, rows, offsets, out, out_elems):
        return (src, src_bytes, _vp(rows), _vp(offsets), len(rows), self.reductions,
                1 if self.multi_scale_hflip else 0, out, out_elems, *self._format())

    def _launch(self, rows, offsets, src_bytes, out, out_elems):
        """pp_preprocess_views over the gathered source buffer on _device.stream()."""
        tables_bytes = load().pp_preprocess_views_tables_size(len(rows), self.n_views)
        call('pp_preprocess_views',
             *self._args(_device.ptr(self._sources.src), src_bytes, rows, offsets,
                         _device.ptr(out), out_elems),
             *self._table_buffer(tables_bytes, out.device), _device.stream())

    def _twin(self, src, src_bytes, rows, offsets, out, out_elems):
        call('pp_preprocess_views_cpu', *self._args(src, src_bytes, rows, offsets, out, out_elems))
