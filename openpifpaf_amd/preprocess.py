"""eval_coco.preprocess_factory (eval_coco.py:350-389) on the device: NormalizeAnnotations,
RescaleAbsolute(long_edge), CenterPad(long_edge) or CenterPadTight(16) and EVAL_TRANSFORM
(ToTensor, Normalize) for whole batches of images of different sizes in one launch
(pp_preprocess_images, csrc/preprocess.hip).

`EvalPreprocess.batch` returns the normalised input tensors and the reference's meta dicts
(the ones `Preprocess.annotations_inverse`, `eval_coco.metas_device` and `coco_records`
consume); `EvalPreprocess.__call__` has the reference's per-image signature; `batch_cpu` runs
the host twin and is only ever used when called by name.  The metas and the annotations are
host NumPy work in float64 / float32 with exactly the chain's operations.

The planner, the source staging, the buffers and the entry points are `_EvalChain`'s, which
preprocess_views.EvalViews (the chain's options and the input pyramid) shares.
"""
import copy
import ctypes
import math

import numpy as np
import torch

from . import _device
from ._abi import (IMAGE_DESC_DTYPE, PP_PRE_BF16, PP_PRE_CHANNELS_LAST, PP_PRE_F16, PP_PRE_F32,
                   PP_PRE_PLANAR, PP_PRE_U8, VIEW_IMAGE_DTYPE)
from ._lib import call, load

# transforms/__init__.py:24-25 and pad.py:51
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
FILL = (124, 116, 104)
PAD_MULTIPLE = 16  # eval_coco.py:371

_DTYPES = {torch.float32: (PP_PRE_F32, np.float32), torch.float16: (PP_PRE_F16, np.float16),
           torch.bfloat16: (PP_PRE_BF16, np.uint16), torch.uint8: (PP_PRE_U8, np.uint8)}
_BILINEAR = 2  # PIL.Image.BILINEAR


def rescaled_size(h, w, long_edge):
    """(th, tw) of RescaleAbsolute.__call__ (scale.py:119-134), Python float arithmetic."""
    s = long_edge / max(h, w)
    if h > w:
        tw, th = int(w * s), int(long_edge)
    else:
        tw, th = int(long_edge), int(h * s)
    # scipy.ndimage.zoom sizes its output as round(size * zoom); scale.py:43-44 asserts
    assert int(round(w * (tw / w))) == tw
    assert int(round(h * (th / h))) == th
    return th, tw


def center_pad(th, tw, target_w, target_h):
    """pad.py:30-46 / 79-97: (left, top, right, bottom)."""
    left = max(int((target_w - tw) / 2.0), 0)
    top = max(int((target_h - th) / 2.0), 0)
    right = max(target_w - tw - left, 0)
    bottom = max(target_h - th - top, 0)
    return left, top, right, bottom


def normalize_annotations(anns):
    """annotations.py:14-28."""
    anns = copy.deepcopy(anns)
    for ann in anns:
        if 'keypoints' not in ann:
            ann['keypoints'] = []
        ann['keypoints'] = np.asarray(ann['keypoints'], dtype=np.float32).reshape(-1, 3)
        ann['bbox'] = np.asarray(ann['bbox'], dtype=np.float32)
        if 'bbox_original' not in ann:
            ann['bbox_original'] = np.copy(ann['bbox'])
        if 'segmentation' in ann:
            del ann['segmentation']
    return anns


class _Plan:
    """Sizes of one image through the chain."""

    rot = 0  # quarter turns (preprocess_views._ViewPlan)

    def __init__(self, h, w, long_edge, tight, rescale_edge=None):
        """rescale_edge: the image's own RescaleAbsolute edge where it is not long_edge
        (eval_coco.py:359-366 extended_scale); the pad target stays long_edge."""
        if h < 2 or w < 2:
            raise ValueError('image edges must be at least 2 pixels, got {}x{}'.format(h, w))
        self.h, self.w = h, w
        edge = long_edge if rescale_edge is None else rescale_edge
        self.rescale = bool(edge)
        self.th, self.tw = rescaled_size(h, w, edge) if edge else (h, w)
        if self.th < 2 or self.tw < 2:
            raise ValueError('rescaled edges must be at least 2 pixels, got {}x{}'
                             .format(self.th, self.tw))
        if tight:
            target_w = math.ceil((self.tw - 1) / PAD_MULTIPLE) * PAD_MULTIPLE + 1
            target_h = math.ceil((self.th - 1) / PAD_MULTIPLE) * PAD_MULTIPLE + 1
        else:
            target_w = target_h = long_edge
        self.ltrb = center_pad(self.th, self.tw, target_w, target_h)
        self.H = self.ltrb[1] + self.th + self.ltrb[3]
        self.W = self.ltrb[0] + self.tw + self.ltrb[2]

    def scales(self):
        """scale.py:47-48."""
        return (self.tw - 1) / (self.w - 1), (self.th - 1) / (self.h - 1)

    def meta(self, meta):
        """annotations.py:33-48, scale.py:58-63, pad.py:24-25."""
        meta = {} if meta is None else dict(meta)
        defaults = {
            'offset': np.array((0.0, 0.0)),
            'scale': np.array((1.0, 1.0)),
            'rotation': {'angle': 0.0, 'width': None, 'height': None},
            'valid_area': np.array((0.0, 0.0, self.w - 1, self.h - 1)),
            'hflip': False,
            'width_height': np.array((self.w, self.h)),
        }
        for k, v in defaults.items():
            if k not in meta:
                meta[k] = v
        meta = copy.deepcopy(meta)
        if self.rescale:
            scale_factors = np.array(self.scales())
            meta['offset'] *= scale_factors
            meta['scale'] *= scale_factors
            meta['valid_area'][:2] *= scale_factors
            meta['valid_area'][2:] *= scale_factors
        meta['offset'] -= self.ltrb[:2]
        meta['valid_area'][:2] += self.ltrb[:2]
        return meta

    def anns(self, anns):
        """annotations.py:14-28, scale.py:49-55, pad.py:54-58."""
        anns = normalize_annotations(anns)
        if self.rescale:
            x_scale, y_scale = self.scales()
            for ann in anns:
                ann['keypoints'][:, 0] = ann['keypoints'][:, 0] * x_scale
                ann['keypoints'][:, 1] = ann['keypoints'][:, 1] * y_scale
                ann['bbox'][0] *= x_scale
                ann['bbox'][1] *= y_scale
                ann['bbox'][2] *= x_scale
                ann['bbox'][3] *= y_scale
        for ann in anns:
            ann['keypoints'][:, 0] += self.ltrb[0]
            ann['keypoints'][:, 1] += self.ltrb[1]
            ann['bbox'][0] += self.ltrb[0]
            ann['bbox'][1] += self.ltrb[1]
        return anns


def _grown(buf, n, make):
    """`buf` if it holds n elements, else a new buffer of at least n (half as much again)."""
    if buf is not None and buf.numel() >= n:
        return buf
    return make(max(n + n // 2, 1024))


def _vp(array):
    return array.ctypes.data_as(ctypes.c_void_p)


class _Sources:
    """The source images of a batch packed into one device buffer (`src`) at their rows'
    src_offset: host images through a pinned staging buffer in one copy, device images
    gathered on the device."""

    def __init__(self):
        self.src = self._staging = None
        self._staged = None  # event: the last copy out of the staging buffer

    def gather(self, images, descs, src_bytes, dev):
        self.src = _grown(self.src, src_bytes,
                          lambda m: torch.empty(m, dtype=torch.uint8, device=dev))
        host = [i for i, im in enumerate(images) if not _device.is_device(im)]
        if host:
            self._staging = _grown(self._staging, src_bytes,
                                   lambda m: torch.empty(m, dtype=torch.uint8, pin_memory=True))
            if self._staged is not None:
                self._staged.synchronize()  # the previous batch has left the staging buffer
            stage = self._staging.numpy()
            for i in host:
                o = int(descs[i]['src_offset'])
                im = images[i].numpy() if isinstance(images[i], torch.Tensor) else images[i]
                stage[o:o + im.size] = im.reshape(-1)
            # one copy from the first to the last host image (device images in between are
            # written after it)
            lo, last = int(descs[host[0]]['src_offset']), descs[host[-1]]
            hi = int(last['src_offset']) + int(last['h']) * int(last['w']) * 3
            self.src[lo:hi].copy_(self._staging[lo:hi], non_blocking=True)
            self._staged = torch.cuda.Event()
            self._staged.record()
        if not host:  # every image on the device: one gather launch
            torch.cat([im.reshape(-1) for im in images], out=self.src[:src_bytes])
        else:
            for i, im in enumerate(images):
                if _device.is_device(im):
                    o = int(descs[i]['src_offset'])
                    self.src[o:o + im.numel()].view(im.shape).copy_(im)


class _EvalChain:
    """What EvalPreprocess and preprocess_views.EvalViews share: the refusals of both, the
    planner, the output and table buffers and the entry points.  A subclass gives the plan of
    one image (`_view_plan(h, w, meta)`: a _Plan), the device call (`_launch`) and the twin
    call (`_twin`); with `_view_edges` set (the edges of the pyramid's views) a batch is a
    list of views, without it one canvas per image."""

    _view_edges = None

    @property
    def n_views(self):
        return len(self._view_edges) if self._view_edges else 1

    def __init__(self, long_edge, tight_padding, dtype, channels_last, fast, resample):
        if fast:
            raise NotImplementedError('fast=True (PIL resize)')
        if resample not in (_BILINEAR, 'bilinear'):
            raise NotImplementedError('resample other than bilinear')
        if isinstance(long_edge, (tuple, list)):
            raise NotImplementedError('random long_edge range')
        if not tight_padding:
            assert long_edge  # eval_coco.py:373
        if long_edge and int(long_edge) != long_edge:
            raise NotImplementedError('long_edge that is not an integer')
        if dtype not in _DTYPES:
            raise ValueError('dtype must be one of {}'.format(sorted(str(d) for d in _DTYPES)))
        self.long_edge = int(long_edge) if long_edge else None
        self.tight_padding = bool(tight_padding)
        self.dtype = dtype
        self.channels_last = bool(channels_last)
        self._mean = np.asarray(MEAN, np.float32)
        self._std = np.asarray(STD, np.float32)
        self._fill = np.asarray(FILL, np.uint8)
        self._sources = _Sources()
        self._tables = self._out = None

    # ---------------------------------------------------------------- host-side planning
    @staticmethod
    def _shape(image):
        """(image as given or as an array, (h, w)); raises for anything but uint8 (h, w, 3)."""
        if not isinstance(image, torch.Tensor):
            image = np.asarray(image)
        if image.ndim != 3 or image.shape[2] != 3 or image.dtype not in (np.uint8, torch.uint8):
            raise NotImplementedError('images that are not 3-channel uint8 (got shape {}, {})'
                                      .format(tuple(image.shape), image.dtype))
        return image, (int(image.shape[0]), int(image.shape[1]))

    def _plan(self, images, metas):
        """(images, plans, rows, offsets, src_bytes, out_elems, metas): the VIEW_IMAGE_DTYPE
        rows and the (n, n_views) first elements of every image in every view.  The output
        holds view after view, each with its images in order."""
        if metas is None:
            metas = [None] * len(images)
        if len(metas) != len(images):
            raise ValueError('{} metas for {} images'.format(len(metas), len(images)))
        images = [self._shape(im) for im in images]
        plans = [self._view_plan(h, w, m) for (_, (h, w)), m in zip(images, metas)]
        n = len(plans)
        names = ('h', 'w', 'th', 'tw', 'left', 'top', 'H', 'W', 'rot')
        cols = np.array([(p.h, p.w, p.th, p.tw, p.ltrb[0], p.ltrb[1], p.H, p.W, p.rot)
                         for p in plans], np.int64).reshape(n, len(names)).T
        rows = np.zeros(n, VIEW_IMAGE_DTYPE)
        for name, col in zip(names, cols):
            rows[name] = col
        src_sizes = 3 * cols[0] * cols[1]
        rows['src_offset'] = np.cumsum(src_sizes) - src_sizes
        if self._view_edges:
            sizes = np.repeat(3 * np.square(np.array(self._view_edges, np.int64)), n)
        else:
            sizes = 3 * cols[6] * cols[7]
        offsets = np.ascontiguousarray((np.cumsum(sizes) - sizes).reshape(self.n_views, n).T)
        out_metas = [p.meta(m) for p, m in zip(plans, metas)]
        return ([im for im, _ in images], plans, rows, offsets, int(src_sizes.sum()),
                int(sizes.sum()), out_metas)

    def _results(self, flat, plans, offsets):
        """The results as views of the flat output (a torch tensor or a NumPy array of
        exactly the batch's elements): CenterPad, one (B, 3, L, L) array (every image is
        L x L and the regions are adjacent); tight padding, a (1, 3, H_i, W_i) view per image;
        a pyramid, a list of (B, 3, n_v, n_v) arrays.  uint8: (B, L, L, 3), (H_i, W_i, 3) per
        image, (B, n_v, n_v, 3)."""
        def shaped(o, lead, h, w):
            if self.dtype == torch.uint8:
                return o.reshape(lead + (h, w, 3))
            if not self.channels_last:
                return o.reshape(lead + (3, h, w))
            o = o.reshape(lead + (h, w, 3))
            k = len(lead)
            axes = tuple(range(k)) + (k + 2, k, k + 1)
            return o.permute(*axes) if isinstance(o, torch.Tensor) else o.transpose(*axes)

        n = len(plans)
        if self._view_edges:
            ends = np.cumsum([3 * s * s * n for s in self._view_edges]).tolist()
            return [shaped(flat[e - 3 * s * s * n:e], (n,), s, s)
                    for s, e in zip(self._view_edges, ends)]
        if not self.tight_padding:
            return shaped(flat, (n,), self.long_edge, self.long_edge)
        lead = () if self.dtype == torch.uint8 else (1,)
        return [shaped(flat[o:o + 3 * p.H * p.W], lead, p.H, p.W)
                for o, p in zip(offsets[:, 0].tolist(), plans)]

    def _format(self):
        """dtype, layout, mean, std, fill as every entry takes them."""
        return (_DTYPES[self.dtype][0],
                PP_PRE_CHANNELS_LAST if self.channels_last else PP_PRE_PLANAR,
                _vp(self._mean), _vp(self._std), _vp(self._fill))

    def _table_buffer(self, nbytes, dev):
        """(d_tables, tables_bytes) of a device entry."""
        self._tables = _grown(self._tables, nbytes,
                              lambda m: torch.empty(m, dtype=torch.uint8, device=dev))
        return _device.ptr(self._tables), nbytes

    # ---------------------------------------------------------------------- entry points
    def batch(self, images, metas=None, fresh=False):
        """(tensors, metas) of a list of (h, w, 3) uint8 images: anything np.asarray accepts
        (PIL images among them) or torch uint8 tensors on the host or the device.  CenterPad
        gives one (B, 3, L, L) tensor, tight padding a list of (1, 3, H_i, W_i) tensors, a
        pyramid a list of 5 or 10 tensors (B, 3, n_v, n_v); all are views of one allocation,
        which the next call overwrites unless fresh=True."""
        dev = _device.require()
        images, plans, rows, offsets, src_bytes, out_elems, out_metas = self._plan(images, metas)
        if fresh:
            out = torch.empty(out_elems, dtype=self.dtype, device=dev)
        else:
            out = self._out = _grown(
                self._out, out_elems, lambda m: torch.empty(m, dtype=self.dtype, device=dev))
        if plans:
            self._sources.gather(images, rows, src_bytes, dev)
            self._launch(rows, offsets, src_bytes, out, out_elems)
        return self._results(out[:out_elems], plans, offsets), out_metas

    def batch_cpu(self, images, metas=None):
        """`batch` through the host twin: NumPy arrays of the same shapes; bfloat16 results
        are their bit patterns as uint16.  Device tensors are not accepted.  Nothing falls
        back to this."""
        images, plans, rows, offsets, src_bytes, out_elems, out_metas = self._plan(images, metas)
        src = np.empty(max(src_bytes, 1), np.uint8)
        for o, im in zip(rows['src_offset'].tolist(), images):
            if isinstance(im, torch.Tensor):
                im = im.numpy()
            src[o:o + im.size] = im.reshape(-1)
        out = np.empty(out_elems, _DTYPES[self.dtype][1])
        self._twin(_vp(src), src_bytes, rows, offsets, _vp(out), out_elems)
        return self._results(out, plans, offsets), out_metas

    def __call__(self, image, anns, meta):
        """The reference signature for one image: (tensor (3, H, W), anns, meta); with a
        pyramid the first entry is the list of the image's (3, n_v, n_v) views."""
        _, (h, w) = self._shape(image)
        plan = self._view_plan(h, w, meta)
        views, metas = self.batch([image], [meta], fresh=True)
        if self._view_edges:
            first = [v[0] for v in views]
        else:
            first = views[0]  # CenterPad: the batch's only image
            if self.tight_padding and self.dtype != torch.uint8:
                first = first[0]
        return first, plan.anns(anns), metas[0]


def image_descs(rows, offsets):
    """IMAGE_DESC_DTYPE rows of single-view VIEW_IMAGE_DTYPE rows and their offsets."""
    descs = np.zeros(len(rows), IMAGE_DESC_DTYPE)
    for name in ('src_offset', 'h', 'w', 'th', 'tw', 'left', 'top', 'H', 'W'):
        descs[name] = rows[name]
    descs['out_offset'] = offsets[:, 0]
    return descs


class EvalPreprocess(_EvalChain):
    """eval_coco.preprocess_factory(long_edge, tight_padding=...) for uint8 RGB images.

    dtype: torch.float32, float16 or bfloat16 (the float32 tensor's `.to(dtype)`), or
    torch.uint8 for the padded (H, W, 3) image the reference holds before ToTensor.
    channels_last: the (3, H, W) tensors are views of (H, W, 3) memory."""

    def __init__(self, long_edge, *, tight_padding=False, dtype=torch.float32,
                 channels_last=False, extended_scale=False, orientation_invariant=False,
                 fast=False, resample=_BILINEAR):
        if extended_scale:
            raise NotImplementedError('extended_scale')
        if orientation_invariant:
            raise NotImplementedError('orientation_invariant')
        super().__init__(long_edge, tight_padding, dtype, channels_last, fast, resample)

    def _view_plan(self, h, w, meta):  # pylint: disable=unused-argument
        return _Plan(h, w, self.long_edge, self.tight_padding)

    def _launch(self, rows, offsets, src_bytes, out, out_elems):
        self._launch_descs(image_descs(rows, offsets), src_bytes, out, out_elems)

    def _launch_descs(self, descs, src_bytes, out, out_elems):
        """pp_preprocess_images over the gathered source buffer on _device.stream()."""
        n = len(descs)
        call('pp_preprocess_images', _device.ptr(self._sources.src), src_bytes, _vp(descs), n,
             _device.ptr(out), out_elems, *self._format(),
             *self._table_buffer(load().pp_preprocess_tables_size(n), out.device),
             _device.stream())

    def _twin(self, src, src_bytes, rows, offsets, out, out_elems):
        descs = image_descs(rows, offsets)
        call('pp_preprocess_images_cpu', src, src_bytes, _vp(descs), len(descs), out, out_elems,
             *self._format())


