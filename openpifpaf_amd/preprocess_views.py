"""eval_coco.preprocess_factory with its options, and the input pyramid of a multi-scale
model, on the device in one launch (pp_preprocess_views, csrc/preprocess_views.hip):

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
import ctypes
import math

import numpy as np
import torch

from . import _device
from ._abi import PP_VIEW_ALL, PP_VIEW_R1, VIEW_IMAGE_DTYPE
from ._lib import call, load
from .preprocess import _BILINEAR, _DTYPES, EvalPreprocess, _gather_sources, _grown, _Plan

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


class _ViewPlan:
    """One image through the chain: its sizes (`plan`) and its turn (0..3 quarter turns)."""

    def __init__(self, plan, rot):
        self.plan, self.rot = plan, rot

    def meta(self, meta):
        meta = self.plan.meta(meta)
        if self.rot:
            meta = turn_meta(meta, 90 * self.rot, self.plan.W, self.plan.H)
        return meta

    def anns(self, anns):
        anns = self.plan.anns(anns)
        if self.rot:
            anns = turn_anns(anns, 90 * self.rot, self.plan.W, self.plan.H)
        return anns


class EvalViews:
    """eval_coco.preprocess_factory(long_edge, tight_padding=..., extended_scale=...,
    orientation_invariant=...) for uint8 RGB images, and with multi_scale the reduced (and
    with multi_scale_hflip mirrored) inputs ShellMultiScale.forward makes of its result.

    dtype and channels_last as EvalPreprocess.  With extended_scale or orientation_invariant
    every meta needs an 'image_id' > 0 (the reference asserts it)."""

    def __init__(self, long_edge, *, tight_padding=False, extended_scale=False,
                 orientation_invariant=False, multi_scale=False, multi_scale_hflip=True,
                 dtype=torch.float32, channels_last=False, fast=False, resample=_BILINEAR):
        # everything EvalPreprocess refuses is refused here; its buffers stage the sources
        self._base = EvalPreprocess(long_edge, tight_padding=tight_padding, dtype=dtype,
                                    channels_last=channels_last, fast=fast, resample=resample)
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
        self.long_edge = self._base.long_edge
        self.tight_padding = self._base.tight_padding
        self.dtype = dtype
        self.channels_last = self._base.channels_last
        self.extended_scale = bool(extended_scale)
        self.orientation_invariant = bool(orientation_invariant)
        self.multi_scale = bool(multi_scale)
        self.multi_scale_hflip = bool(multi_scale and multi_scale_hflip)
        self.reductions = PP_VIEW_ALL if self.multi_scale else PP_VIEW_R1
        self.n_views = (10 if self.multi_scale_hflip else 5) if self.multi_scale else 1
        self._tables = self._out = None

    # ---------------------------------------------------------------- host-side planning
    def _view_plan(self, h, w, meta):
        edge = None
        if self.extended_scale:
            edges = (self.long_edge, (self.long_edge - 1) // 2 + 1)
            edge = edges[equal_choice(meta, SALT_SCALE, 2)]
        plan = _Plan(h, w, self.long_edge, self.tight_padding, edge)
        rot = equal_choice(meta, SALT_TURN, 4) if self.orientation_invariant else 0
        return _ViewPlan(plan, rot)

    def _plan(self, images, metas):
        if metas is None:
            metas = [None] * len(images)
        if len(metas) != len(images):
            raise ValueError('{} metas for {} images'.format(len(metas), len(images)))
        images = [self._base._shape(im) for im in images]
        vplans = [self._view_plan(h, w, m) for (_, (h, w)), m in zip(images, metas)]
        n = len(vplans)
        descs = np.zeros(n, VIEW_IMAGE_DTYPE)
        src_off = 0
        for d, vp in zip(descs, vplans):
            p = vp.plan
            d['src_offset'] = src_off
            d['h'], d['w'], d['th'], d['tw'] = p.h, p.w, p.th, p.tw
            d['left'], d['top'], d['H'], d['W'] = p.ltrb[0], p.ltrb[1], p.H, p.W
            d['rot'] = vp.rot
            src_off += p.h * p.w * 3
        offsets = np.zeros((n, self.n_views), np.int64)
        if self.multi_scale:
            sizes = view_sizes(self.long_edge) * (2 if self.multi_scale_hflip else 1)
            base = 0
            for v, s in enumerate(sizes):
                offsets[:, v] = base + 3 * s * s * np.arange(n, dtype=np.int64)
                base += 3 * s * s * n
            out_elems = base
        else:
            out_off = 0
            for i, vp in enumerate(vplans):
                offsets[i, 0] = out_off
                out_off += vp.plan.H * vp.plan.W * 3
            out_elems = out_off
        out_metas = [vp.meta(m) for vp, m in zip(vplans, metas)]
        return [im for im, _ in images], vplans, descs, offsets, src_off, out_elems, out_metas

    def _results(self, flat, vplans, offsets):
        """Views of the flat output.  Without multi_scale what EvalPreprocess returns; with
        it a list of n_views (B, 3, n_v, n_v) arrays ((B, n_v, n_v, 3) for uint8)."""
        if not self.multi_scale:
            return self._base._results(flat, [vp.plan for vp in vplans],
                                       [{'out_offset': o} for o in offsets[:, 0]])
        n = len(vplans)
        sizes = view_sizes(self.long_edge) * (2 if self.multi_scale_hflip else 1)
        out, base = [], 0
        for s in sizes:
            o = flat[base:base + 3 * s * s * n]
            base += 3 * s * s * n
            if self.dtype == torch.uint8:
                out.append(o.reshape(n, s, s, 3))
            elif not self.channels_last:
                out.append(o.reshape(n, 3, s, s))
            else:
                o = o.reshape(n, s, s, 3)
                out.append(o.permute(0, 3, 1, 2) if isinstance(o, torch.Tensor)
                           else o.transpose(0, 3, 1, 2))
        return out

    def _args(self, src, src_bytes, descs, offsets, out, out_elems):
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        b = self._base
        return (src, src_bytes, vp(descs), vp(offsets), len(descs), self.reductions,
                1 if self.multi_scale_hflip else 0, out, out_elems, _DTYPES[self.dtype][0],
                b._layout(), vp(b._mean), vp(b._std), vp(b._fill))

    def _launch(self, descs, offsets, src_bytes, out, out_elems):
        """pp_preprocess_views over the gathered source buffer on _device.stream()."""
        tables_bytes = load().pp_preprocess_views_tables_size(len(descs), self.n_views)
        self._tables = _grown(self._tables, tables_bytes,
                              lambda m: torch.empty(m, dtype=torch.uint8, device=out.device))
        call('pp_preprocess_views',
             *self._args(_device.ptr(self._base._src), src_bytes, descs, offsets,
                         _device.ptr(out), out_elems),
             _device.ptr(self._tables), tables_bytes, _device.stream())

    # ---------------------------------------------------------------------- entry points
    def batch(self, images, metas=None, fresh=False):
        """(views, metas) of a list of (h, w, 3) uint8 images, host or device, as
        EvalPreprocess.batch takes them.  Without multi_scale `views` is its result (one
        (B, 3, L, L) tensor, or per-image tensors under tight padding); with it a list of 5 or
        10 tensors (B, 3, n_v, n_v), all views of one allocation, which the next call
        overwrites unless fresh=True."""
        dev = _device.require()
        images, vplans, descs, offsets, src_bytes, out_elems, out_metas = self._plan(images, metas)
        if fresh:
            out = torch.empty(out_elems, dtype=self.dtype, device=dev)
        else:
            out = self._out = _grown(
                self._out, out_elems, lambda m: torch.empty(m, dtype=self.dtype, device=dev))
        flat = out[:out_elems]
        if vplans:
            _gather_sources(self._base, images, descs, src_bytes, dev)
            self._launch(descs, offsets, src_bytes, out, out_elems)
        return self._results(flat, vplans, offsets), out_metas

    def batch_cpu(self, images, metas=None):
        """`batch` through the host twin (pp_preprocess_views_cpu): NumPy arrays of the same
        shapes; bfloat16 results are their bit patterns as uint16.  Device tensors are not
        accepted.  Nothing falls back to this."""
        images, vplans, descs, offsets, src_bytes, out_elems, out_metas = self._plan(images, metas)
        src = np.empty(max(src_bytes, 1), np.uint8)
        for d, im in zip(descs, images):
            if isinstance(im, torch.Tensor):
                im = im.numpy()
            src[int(d['src_offset']):int(d['src_offset']) + im.size] = im.reshape(-1)
        out = np.empty(out_elems, _DTYPES[self.dtype][1])
        call('pp_preprocess_views_cpu',
             *self._args(src.ctypes.data_as(ctypes.c_void_p), src_bytes, descs, offsets,
                         out.ctypes.data_as(ctypes.c_void_p), out_elems))
        return self._results(out, vplans, offsets), out_metas

    def __call__(self, image, anns, meta):
        """The reference signature for one image: (tensor (3, H, W), anns, meta); with
        multi_scale the first entry is the list of the image's (3, n_v, n_v) views."""
        _, (h, w) = self._base._shape(image)
        vplan = self._view_plan(h, w, meta)
        views, metas = self.batch([image], [meta], fresh=True)
        if self.multi_scale:
            first = [v[0] for v in views]
        else:
            first = views[0]  # CenterPad: the batch's only image
            if self.tight_padding and self.dtype != torch.uint8:
                first = first[0]
        return first, vplan.anns(anns), metas[0]
