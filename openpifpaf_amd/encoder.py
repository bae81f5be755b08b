"""openpifpaf.encoder's Cif and Caf (encoder/cif.py, caf.py, annrescaler.py) on the device:
annotations to CIF / CAF target fields for whole batches in one launch per encoder
(pp_encode_cif / pp_encode_caf, csrc/encode.hip), bit for bit the reference's tensors.

`Cif(...)(image, anns, meta)` and `Caf(...)` keep the reference's signature and return device
tensors; `.batch` encodes a list of images at once; `.batch_cpu` runs the host twin and is
only ever used when called by name.  Python only marshals the annotations into the
library's host tables: every number of the reference is computed by the library.
"""
import ctypes
import dataclasses
from typing import Any, ClassVar

import numpy as np
import torch

from . import _device
from ._abi import (ENC_ANN_DTYPE, ENC_IMAGE_DTYPE, PP_ENC_HAS_BBOX, PP_ENC_HAS_KEYPOINTS,
                   PP_MAX_EDGES, PP_MAX_KP, Encoder)
from ._lib import call, load
from .preprocess import _grown


class AnnRescaler:
    """annrescaler.py:8-26: the stride, the pose and its copy turned by 45 degrees, with
    their bounding-box areas.  The rescaling itself (keypoint_sets, bg_mask, valid_area,
    scale) is the library's."""

    def __init__(self, stride, n_keypoints, pose):
        self.stride = stride
        self.n_keypoints = n_keypoints
        self.pose = pose
        self.pose_total_area = self._area(pose)
        turn = np.deg2rad(45)
        rotate = np.array(((np.cos(turn), -np.sin(turn)), (np.sin(turn), np.cos(turn))))
        self.pose_45 = np.copy(pose)
        self.pose_45[:, :2] = np.einsum('ij,kj->ki', rotate, self.pose_45[:, :2])
        self.pose_45_total_area = self._area(self.pose_45)

    @staticmethod
    def _area(pose):
        return ((np.max(pose[:, 0]) - np.min(pose[:, 0])) *
                (np.max(pose[:, 1]) - np.min(pose[:, 1])))


class AnnRescalerDet:
    def __init__(self, *args, **kwargs):
        raise NotImplementedError('CifDet encoder')


class CifDet:
    def __init__(self, *args, **kwargs):
        raise NotImplementedError('CifDet encoder')


def _pixel_size(item):
    """(height, width) in pixels of an image (C, H, W) or of a (height, width) pair."""
    shape = getattr(item, 'shape', None)
    if shape is not None and len(shape) == 3:
        return int(shape[1]), int(shape[2])
    if shape is None and len(item) == 2:
        return int(item[0]), int(item[1])
    raise ValueError('an image (C, H, W) or a (height, width) pair, got {!r}'.format(shape))


class _Encoder:
    """Marshalling and buffers shared by Cif and Caf."""
    _name = None      # 'cif' / 'caf'
    _shapes = None    # per output tensor: 6 for a (F, 6, h, w) tensor, 1 for (F, h, w)

    # -------------------------------------------------------------------- the encoder
    def _n_fields(self):
        raise NotImplementedError

    def _config(self):
        """(pp_encoder, the arrays it points to)."""
        r = self.rescaler
        stride = r.stride
        if int(stride) != stride or stride < 1:
            raise NotImplementedError('a stride that is not a positive integer')
        k = int(r.n_keypoints)
        pose = np.ascontiguousarray(np.asarray(r.pose, np.float64)[:, :2])
        pose_45 = np.ascontiguousarray(np.asarray(r.pose_45, np.float64)[:, :2])
        if pose.shape != (k, 2) or pose_45.shape != (k, 2):
            raise ValueError('pose must have n_keypoints rows')
        keep = [pose, pose_45]
        enc = Encoder()
        enc.pose, enc.pose_45 = pose.ctypes.data, pose_45.ctypes.data
        if self.sigmas is not None:
            sigmas = np.ascontiguousarray([float(s) for s in self.sigmas], np.float64)
            if sigmas.shape != (k,):
                raise ValueError('sigmas must have n_keypoints entries')
            keep.append(sigmas)
            enc.sigmas = sigmas.ctypes.data
        enc.v_threshold = float(self.v_threshold)
        enc.stride, enc.K = int(stride), k
        enc.padding = int(self.padding)
        self._config_fields(enc, keep)
        return enc, keep

    def _config_fields(self, enc, keep):
        raise NotImplementedError

    # -------------------------------------------------------------------- the tables
    def _tables(self, sizes_or_images, anns_batch, metas):
        n = len(sizes_or_images)
        if len(anns_batch) != n or len(metas) != n:
            raise ValueError('{} images, {} annotation lists, {} metas'
                             .format(n, len(anns_batch), len(metas)))
        k = int(self.rescaler.n_keypoints)
        stride = int(self.rescaler.stride)
        n_ann = sum(len(a) for a in anns_batch)
        images = np.zeros(n, ENC_IMAGE_DTYPE)
        anns = np.zeros(n_ann, ENC_ANN_DTYPE)
        keypoints = np.zeros((n_ann, k, 3), np.float32)
        at = 0
        for im, item, image_anns, meta in zip(images, sizes_or_images, anns_batch, metas):
            im['height'], im['width'] = _pixel_size(item)
            im['h'] = (im['height'] - 1) // stride + 1
            im['w'] = (im['width'] - 1) // stride + 1
            if meta is not None and 'valid_area' in meta:
                im['has_valid_area'] = 1
                im['valid_area'] = [float(v) for v in meta['valid_area']]
            im['ann0'], im['n_ann'] = at, len(image_anns)
            for ann in image_anns:
                a = anns[at]
                a['iscrowd'] = 1 if ann['iscrowd'] else 0
                if 'keypoints' in ann:
                    a['flags'] |= PP_ENC_HAS_KEYPOINTS
                    if not a['iscrowd']:
                        kp = ann['keypoints']
                        if isinstance(kp, np.ndarray) and kp.dtype != np.float32:
                            raise NotImplementedError('keypoints that are not float32 (got {})'
                                                      .format(kp.dtype))
                        kp = np.asarray(kp, np.float32)
                        if kp.shape != (k, 3):
                            raise ValueError('keypoints must be ({}, 3), got {}'
                                             .format(k, kp.shape))
                        keypoints[at] = kp
                if 'bbox' in ann:
                    bbox = ann['bbox']
                    if isinstance(bbox, np.ndarray) and bbox.dtype != np.float32:
                        raise NotImplementedError('a bbox that is not float32 (got {})'
                                                  .format(bbox.dtype))
                    a['flags'] |= PP_ENC_HAS_BBOX
                    a['bbox'] = np.asarray(bbox, np.float32).reshape(4)
                if 'mask' in ann and (a['iscrowd'] or not np.any(keypoints[at, :, 2] > 0)):
                    raise NotImplementedError('crowd masks (annrescaler.py:72 asserts too)')
                at += 1
        return images, anns, keypoints

    def _layout(self, images):
        """Sets every image's out_offset; returns (elements, stacked): tensors of one size
        lie image after image per tensor, so that each tensor of the batch is one (B, ...)
        array; images of different sizes hold their tensors one after another."""
        f = self._n_fields()
        stacked = len(images) > 0 and len({(int(m['h']), int(m['w'])) for m in images}) == 1
        at = 0
        if stacked:
            hw = int(images[0]['h']) * int(images[0]['w'])
            for t, planes in enumerate(self._shapes):
                for m in images:
                    m['out_offset'][t] = at
                    at += planes * f * hw
            return at, True
        for m in images:
            hw = int(m['h']) * int(m['w'])
            for t, planes in enumerate(self._shapes):
                m['out_offset'][t] = at
                at += planes * f * hw
        return at, False

    def _results(self, flat, images, stacked):
        f = self._n_fields()

        def shape(planes, h, w, lead=()):
            return lead + ((f, h, w) if planes == 1 else (f, planes, h, w))

        if stacked:
            h, w, b = int(images[0]['h']), int(images[0]['w']), len(images)
            out = []
            for t, planes in enumerate(self._shapes):
                o = int(images[0]['out_offset'][t])
                out.append(flat[o:o + b * planes * f * h * w].reshape(shape(planes, h, w, (b,))))
            return tuple(out)
        out = []
        for m in images:
            h, w = int(m['h']), int(m['w'])
            out.append(tuple(
                flat[int(m['out_offset'][t]):int(m['out_offset'][t]) + planes * f * h * w]
                .reshape(shape(planes, h, w)) for t, planes in enumerate(self._shapes)))
        return out

    @staticmethod
    def _vp(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    # ------------------------------------------------------------------ entry points
    def batch(self, sizes_or_images, anns_batch, metas, fresh=False, out=None):
        """The target tensors of a batch on the device, asynchronously on the current
        stream.  sizes_or_images: per image the (C, H, W) image (read for its shape only) or
        its (height, width) in pixels.  All sizes equal: the tuple of stacked (B, ...)
        tensors; otherwise a list of per-image tuples, views of one allocation.  The tensors
        are overwritten by the next call unless fresh=True.  out: a flat float32 device
        tensor to encode into instead (it must hold the batch's elements)."""
        dev = _device.require()
        enc, keep = self._config()
        images, anns, keypoints = self._tables(sizes_or_images, anns_batch, metas)
        n = len(images)
        elems, stacked = self._layout(images)
        if out is not None:
            if not _device.is_device(out) or out.dtype != torch.float32 or out.dim() != 1 \
                    or not out.is_contiguous() or out.numel() < elems:
                raise ValueError('out must be a flat float32 device tensor of at least {} '
                                 'elements'.format(elems))
        elif fresh:
            out = torch.empty(max(elems, 1), dtype=torch.float32, device=dev)
        else:
            out = self._out = _grown(getattr(self, '_out', None), elems,
                                     lambda m: torch.empty(m, dtype=torch.float32, device=dev))
        if n == 0:
            return []
        size = getattr(load(), 'pp_encode_{}_tables_size'.format(self._name))
        tables_bytes = size(n, len(anns), self._n_fields())
        self._tab = _grown(getattr(self, '_tab', None), tables_bytes,
                           lambda m: torch.empty(m, dtype=torch.uint8, device=dev))
        call('pp_encode_' + self._name, ctypes.byref(enc), self._vp(images), n, self._vp(anns),
             self._vp(keypoints), len(anns), _device.ptr(out), out.numel(),
             _device.ptr(self._tab), self._tab.numel(), _device.stream())
        del keep
        return self._results(out, images, stacked)

    def batch_cpu(self, sizes_or_images, anns_batch, metas, n_threads=1):
        """`batch` through the host twin: NumPy arrays of the same shapes.  Nothing falls
        back to this."""
        enc, keep = self._config()
        images, anns, keypoints = self._tables(sizes_or_images, anns_batch, metas)
        n = len(images)
        elems, stacked = self._layout(images)
        if n == 0:
            return []
        out = np.empty(elems, np.float32)
        call('pp_encode_{}_cpu'.format(self._name), ctypes.byref(enc), self._vp(images), n,
             self._vp(anns), self._vp(keypoints), len(anns), self._vp(out), elems,
             int(n_threads))
        del keep
        return self._results(out, images, stacked)

    def __call__(self, image, anns, meta):
        """The reference's signature for one image: the tuple of its target tensors (device)."""
        fields = tuple(t[0] for t in self.batch([image], [anns], [meta], fresh=True))
        if self.visualizer is not None:
            stride = self.rescaler.stride
            sets = [ann['keypoints'] for ann in anns if not ann['iscrowd']]
            if sets:
                keypoint_sets = np.stack(sets)
                keypoint_sets[:, :, :2] /= stride
            else:
                keypoint_sets = np.zeros((0, self.rescaler.n_keypoints, 3))
            self.visualizer.processed_image(image)
            self.visualizer.targets(fields, keypoint_sets=keypoint_sets)
        return fields


@dataclasses.dataclass
class Cif(_Encoder):
    rescaler: AnnRescaler
    sigmas: list
    v_threshold: int = 0
    visualizer: Any = None

    side_length: ClassVar[int] = 4
    padding: ClassVar[int] = 10

    _name = 'cif'
    _shapes = (1, 6, 1)

    def _n_fields(self):
        return int(self.rescaler.n_keypoints)

    def _config_fields(self, enc, keep):
        if not 1 <= enc.K <= PP_MAX_KP:
            raise NotImplementedError('more than {} keypoints'.format(PP_MAX_KP))
        enc.side = int(self.side_length)


@dataclasses.dataclass
class Caf(_Encoder):
    rescaler: AnnRescaler
    skeleton: list
    sigmas: list
    sparse_skeleton: list = None
    dense_to_sparse_radius: float = 2.0
    only_in_field_of_view: bool = False
    v_threshold: int = 0
    visualizer: Any = None

    min_size: ClassVar[int] = 3
    fixed_size: ClassVar[bool] = False
    aspect_ratio: ClassVar[float] = 0.0
    padding: ClassVar[int] = 10

    _name = 'caf'
    _shapes = (1, 6, 6, 1, 1)

    def _n_fields(self):
        return len(self.skeleton)

    def _config_fields(self, enc, keep):
        if self.aspect_ratio != 0.0:
            raise NotImplementedError('aspect_ratio')
        if not 1 <= len(self.skeleton) <= PP_MAX_EDGES:
            raise NotImplementedError('more than {} skeleton edges'.format(PP_MAX_EDGES))
        skeleton = np.ascontiguousarray(self.skeleton, np.int32).reshape(-1, 2)
        keep.append(skeleton)
        enc.skeleton, enc.C = skeleton.ctypes.data, len(skeleton)
        if self.sparse_skeleton:  # caf.py:40-42: an empty list is no sparse skeleton
            sparse = np.ascontiguousarray(self.sparse_skeleton, np.int32).reshape(-1, 2)
            keep.append(sparse)
            enc.sparse_skeleton, enc.n_sparse = sparse.ctypes.data, len(sparse)
        enc.dense_to_sparse_radius = float(self.dense_to_sparse_radius)
        enc.only_in_field_of_view = 1 if self.only_in_field_of_view else 0
        enc.fixed_size = 1 if self.fixed_size else 0
        enc.aspect_ratio = float(self.aspect_ratio)
        enc.side = int(self.min_size)
