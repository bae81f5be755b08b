"""Batched device decode: fields resident in HBM -> packed annotation records.

The engine owns the per-shape workspace (zeroed once at allocation, see the workspace
contract in include/pifpaf_amd.h) and drives pp_decode_stages on torch's current stream.
Records come back as a NumPy structured array (openpifpaf_amd._abi.ANN_DTYPE) packed over
the whole batch plus per-image offsets; decoder/generator/cifcaf.py turns them into
Annotation objects.
"""
import collections
import ctypes
import logging

import numpy as np
import torch

from . import _device
from ._abi import (ANN_DTYPE, DET_DTYPE, PACK_ALL, PP_ST_ANN_OVERFLOW, PP_ST_DEC_OVERFLOW,
                   PP_ST_NMS_OVERFLOW, packed_dtype, scale_list, skeleton_array)
from ._lib import PPError, call, load

LOG = logging.getLogger(__name__)

STAGE_CIFHR, STAGE_SEEDS, STAGE_CAF, STAGE_GROW = 1, 2, 4, 8
STAGE_ALL = 15
# PP_STAGE_COMPLETE_SETS_EARLY: the force-complete column sets with the CAF stage
STAGE_COMPLETE_EARLY = 16
# PP_STAGE_SEED_LOOP_ONLY / PP_STAGE_AFTER_SEED_LOOP: stage 8 in two calls (same slot)
STAGE_SEED_LOOP_ONLY, STAGE_AFTER_SEED_LOOP = 32, 64
# PP_STAGE_COMPLETE_ONLY / PP_STAGE_NMS_ONLY: the after-seed-loop part in two calls
STAGE_COMPLETE_ONLY, STAGE_NMS_ONLY = 128, 256
# PP_STAGE_NMS_WIDE: NMS in 8-wave workgroups (dense batches; the 4-wave default fits beside
# a seed loop on a CU)
STAGE_NMS_WIDE = 512
# PP_STAGE_NMS_BITMAP: NMS planes as LDS bitmaps, one wave per (image, plane) (opt-in)
STAGE_NMS_BITMAP = 1024


def default_ann_capacity(h, w):
    """Annotations per image the first attempt reserves (doubles on overflow)."""
    return int(min(8192, max(128, (h * w) // 8)))


class DecodeBuffers:
    """Workspace + outputs for one (batch shape, config) combination.  `heads` (a HeadSet)
    selects the multi-scale entry points."""

    def __init__(self, key, n, k, c, h, w, cfg, cap, device, heads=None):
        lib = load()
        self.key = key
        self.n, self.k, self.c, self.cap = n, k, c, cap
        if heads is None:
            size = lib.pp_decode_workspace_size(n, k, c, h, w, ctypes.byref(cfg), cap)
            zero_off = lib.pp_decode_workspace_zero_offset(n, k, c, h, w, ctypes.byref(cfg), cap)
            self.work_off = lib.pp_decode_work_offset(n, k, c, h, w, ctypes.byref(cfg), cap)
            stride = cfg.stride
        else:
            args = (heads.arr, len(heads.arr), heads.pairs, n, k, c, ctypes.byref(cfg), cap)
            size = lib.pp_decode_multi_workspace_size(*args)
            zero_off = lib.pp_decode_multi_workspace_zero_offset(*args)
            self.work_off = lib.pp_decode_multi_work_offset(*args)
            stride = heads.stride0
        if size == 0:
            raise PPError('pp_decode_workspace_size rejected the shape: ' +
                          lib.pp_last_error().decode())
        self.ws = torch.empty(size, dtype=torch.uint8, device=device)
        self.ws[zero_off:].zero_()
        # two output slots (records, counts, status): a decode with the grow stage writes the
        # slot after the previous one, so records of decode i can still be packed / fetched
        # while decode i + 1 runs (DecodeEngine.fetch_async)
        self._slots = [(torch.empty(n * cap * ANN_DTYPE.itemsize, dtype=torch.uint8, device=device),
                        torch.zeros(n, dtype=torch.int32, device=device),
                        torch.zeros(n, dtype=torch.int32, device=device)) for _ in range(2)]
        self._cur = 0
        self._free = [None, None]  # per slot: event after which its records were packed
        self.hh = (h - 1) * stride + 1
        self.ww = (w - 1) * stride + 1
        self.pitch = int(lib.pp_cifhr_pitch(self.ww))
        self.cifhr = None
        self.out_index = None  # pp_decode_initial's (n, cap) positions before NMS

    def work_records(self, img, positions):
        """pp_decode_work_offset: image img's annotations at `positions` of its list before
        NMS, in the state NMS left them (ANN_DTYPE, host), after a decode with the grow
        stage and before the next decode into this workspace."""
        rows = self.ws[self.work_off:self.work_off + self.n * self.cap * ANN_DTYPE.itemsize]
        rows = rows.view(self.n * self.cap, ANN_DTYPE.itemsize)
        idx = torch.as_tensor([img * self.cap + int(p) for p in positions], dtype=torch.int64,
                              device=rows.device)
        return rows.index_select(0, idx).cpu().numpy().reshape(-1).view(ANN_DTYPE)

    anns = property(lambda self: self._slots[self._cur][0])
    counts = property(lambda self: self._slots[self._cur][1])
    status = property(lambda self: self._slots[self._cur][2])

    def next_slot(self):
        """Switch to the other output slot; the current stream waits until that slot's
        previous records have been packed (fetch_async packs on a side stream)."""
        self._cur ^= 1
        if self._free[self._cur] is not None:
            torch.cuda.current_stream().wait_event(self._free[self._cur])
            self._free[self._cur] = None

    def cifhr_buffer(self):
        if self.cifhr is None:
            self.cifhr = torch.empty((self.n, self.k, self.hh, self.pitch), dtype=torch.float32,
                                     device=self.ws.device)
        return self.cifhr


class InitialAnnotations:
    """Per-image initial annotations (CifCaf.__call__'s initial_annotations,
    cifcaf.py:67-71) as device pp_ann records for pp_decode_initial: `records` (n, cap)
    ANN_DTYPE rows, `counts` (n) int32.  `per_image`: one list of ANN_DTYPE record arrays
    per image."""

    def __init__(self, per_image, device):
        self.n = len(per_image)
        self.cap = max(1, max((len(r) for r in per_image), default=0))
        host = np.zeros((self.n, self.cap), ANN_DTYPE)
        for i, r in enumerate(per_image):
            host[i, :len(r)] = r
        self.records = torch.from_numpy(host.view(np.uint8).reshape(-1)).to(device)
        self.counts = torch.tensor([len(r) for r in per_image], dtype=torch.int32,
                                   device=device)


class HeadSet:
    """The CIF and CAF heads of a FieldConfig for one batch of device fields
    (field_config.py:7-13): `fields` is the head-network output list with a leading batch
    dimension on every tensor.  Builds the pp_scale list of pp_decode_multi."""

    def __init__(self, fields, fc):
        self.cifs = [fields[i] for i in fc.cif_indices]
        self.cafs = [fields[i] for i in fc.caf_indices]
        for t in self.cifs + self.cafs:
            if not _device.is_device(t) or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError('multi-scale fields must be contiguous float32 device tensors')
            if t.dim() != 5:
                raise ValueError('expected batched fields (B, n_fields, channels, H, W)')
        if any(t.shape[2] != 5 for t in self.cifs) or any(t.shape[2] != 9 for t in self.cafs):
            raise ValueError('expected CIF heads (B, K, 5, H, W) and CAF heads (B, C, 9, H, W)')
        self.n = self.cifs[0].shape[0]
        self.k = self.cifs[0].shape[1]
        self.c = self.cafs[0].shape[1]
        if any(t.shape[0] != self.n for t in self.cifs + self.cafs):
            raise ValueError('heads have different batch sizes')
        if any(t.shape[1] != self.k for t in self.cifs) or any(t.shape[1] != self.c for t in self.cafs):
            raise ValueError('heads have different field counts')
        self.h, self.w = self.cifs[0].shape[3], self.cifs[0].shape[4]
        self.stride0 = int(fc.cif_strides[0])
        self.pairs = int(len(fc.cif_indices) == 10)  # cif_hr.py:63
        self.arr = scale_list([(t.data_ptr(), t.shape[3], t.shape[4]) for t in self.cifs],
                              [(t.data_ptr(), t.shape[3], t.shape[4]) for t in self.cafs],
                              fc.cif_strides, fc.caf_strides, fc.cif_min_scales,
                              fc.caf_min_distances, fc.caf_max_distances)
        self.shape_key = (self.pairs,) + tuple(
            (s.H, s.W, s.stride, s.role) for s in self.arr)


class RaggedFields:
    """A batch of images of different field sizes (pp_fields_pack_ragged): `fields` is a list
    of per-image (cif, caf) device tensors, float32 and contiguous, (K, 5, h_i, w_i) and
    (C, 9, h_i, w_i) with K and C the same for every image.  Packs them on the current stream
    into the containers `cif` (n, K, 5, H, W) and `caf` (n, C, 9, H, W), (H, W) the largest
    size, zero outside each image's extent, and owns them with the extent table (`extents`,
    device (n, 2) int32; `extents_host` the same on the host).  The images' tensors may be
    freed once the pack has run.  A list of equal shapes takes the same route.
    RaggedFields.from_conv builds the same object from the heads' conv outputs, without
    per-image fields and without the pack."""

    def __init__(self, fields):
        lib = load()
        fields = [tuple(f) for f in fields]
        if not fields:
            raise ValueError('a ragged batch needs at least one image')
        for f in fields:
            if len(f) != 2 or not all(_device.is_device(t) and t.dtype == torch.float32 and
                                      t.is_contiguous() and t.dim() == 4 for t in f):
                raise ValueError('ragged fields must be (cif, caf) pairs of contiguous float32 '
                                 'device tensors (K, 5, h, w) and (C, 9, h, w)')
            if f[0].shape[1] != 5 or f[1].shape[1] != 9 or f[0].shape[2:] != f[1].shape[2:]:
                raise ValueError('expected cif (K, 5, h, w) and caf (C, 9, h, w) of one spatial '
                                 'shape per image, got {} and {}'.format(tuple(f[0].shape),
                                                                         tuple(f[1].shape)))
        self.n = n = len(fields)
        self.k, self.c = fields[0][0].shape[0], fields[0][1].shape[0]
        if any(f[0].shape[0] != self.k or f[1].shape[0] != self.c for f in fields):
            raise ValueError('the images of a ragged batch differ in K or C: ' + ', '.join(
                sorted({'K={} C={}'.format(f[0].shape[0], f[1].shape[0]) for f in fields})))
        self.extents_host = np.array([f[0].shape[2:] for f in fields], np.int32).reshape(n, 2)
        self.h, self.w = (int(v) for v in self.extents_host.max(axis=0))
        dev = fields[0][0].device
        self.cif = torch.empty((n, self.k, 5, self.h, self.w), dtype=torch.float32, device=dev)
        self.caf = torch.empty((n, self.c, 9, self.h, self.w), dtype=torch.float32, device=dev)
        # pinned host tables (pointers, then extents, per field kind): the copies are
        # asynchronous, so the tables live as long as this object
        size, ext_off = lib.pp_ragged_tables_size(n), lib.pp_ragged_extents_offset(n)
        self._host = torch.empty((2, size), dtype=torch.uint8, pin_memory=True)
        self._tables = torch.empty((2, size), dtype=torch.uint8, device=dev)
        for kind in range(2):
            host = self._host[kind].numpy()
            host[:ext_off].view(np.uint64)[:] = [f[kind].data_ptr() for f in fields]
            host[ext_off:].view(np.int32)[:] = self.extents_host.reshape(-1)
        self.extents = self._tables[0][ext_off:].view(torch.int32).view(n, 2)
        self.pack()

    _ingests = ()  # from_conv: the heads.RaggedIngest of each head, CIF first

    @classmethod
    def from_conv(cls, cif_convs, caf_convs, n_cif, n_caf, quad=1, conv_extents=None,
                  cif_hflip=None, caf_hflip=None, caf_parts=None):
        """The same object from the heads' conv outputs, one HIP pass per head straight into
        the containers (heads.fields_from_conv_ragged has the forms `cif_convs` / `caf_convs`
        and `conv_extents` take; NCHW and channels-last conv outputs and their slices are read
        where they lie): no per-image fields and no pack.  `caf_parts`, a list of
        (convs, n_fields, hflip), replaces caf_convs / n_caf / caf_hflip: the parts are
        written side by side into one CAF container (CAF and dense CAF of the
        dense-connection layout).  pack() runs the ingest launches again."""
        from .heads import RaggedIngest  # pylint: disable=import-outside-toplevel
        if caf_parts is None:
            caf_parts = [(caf_convs, n_caf, caf_hflip)]
        heads = [cif_convs] + [p[0] for p in caf_parts]
        sizes = {len(c) for c in heads}
        if len(sizes) != 1:
            raise ValueError('the heads of a ragged batch have different numbers of images: ' +
                             ', '.join(str(s) for s in sorted(sizes)))
        cif = RaggedIngest(cif_convs, n_cif, 'cif', quad, cif_hflip, conv_extents)
        total, parts = sum(p[1] for p in caf_parts), []
        for convs, n_fields, hflip in caf_parts:
            done = sum(p[1] for p in caf_parts[:len(parts)])
            parts.append(RaggedIngest(convs, n_fields, 'caf', quad, hflip, conv_extents,
                                      shape=(cif.h, cif.w) if not parts else None,
                                      out=parts[0].out if parts else None, out_field0=done,
                                      out_fields=total))
        if any(not np.array_equal(p.extents_host, cif.extents_host) for p in parts):
            raise ValueError('the CIF and CAF conv outputs of a ragged batch differ in size')
        self = cls.__new__(cls)
        self.n, self.k, self.c, self.h, self.w = cif.n, n_cif, total, cif.h, cif.w
        self.cif, self.caf = cif.out, parts[0].out
        self.extents, self.extents_host = cif.extents, cif.extents_host
        self._ingests = [cif] + parts
        self.pack()
        return self

    def pack(self):
        """The two pack launches (CIF, then CAF) on the current stream, from the tables built
        at construction: again after the images' tensors were rewritten in place.  After
        from_conv: the ingest launches."""
        for ingest in self._ingests:
            ingest.launch()
        if self._ingests:
            return
        size, ext_off = self._host.shape[1], load().pp_ragged_extents_offset(self.n)
        for kind, (out, planes, ch) in enumerate(((self.cif, self.k, 5), (self.caf, self.c, 9))):
            call('pp_fields_pack_ragged', ctypes.c_void_p(self._host[kind].data_ptr()),
                 ctypes.c_void_p(self._host[kind].data_ptr() + ext_off), self.n, planes, ch,
                 self.h, self.w, _device.ptr(out), _device.ptr(self._tables[kind]),
                 ctypes.c_size_t(size), _device.stream())


class RaggedDetFields:
    """RaggedFields for the detection decoder (pp_cifdet_decode_ragged): `fields` is a list of
    per-image CifDet device tensors, float32 and contiguous, (K, 7, h_i, w_i) with K the same
    for every image.  Packs them on the current stream into the container `det`
    (n, K, 7, H, W), (H, W) the largest size, zero outside each image's extent, and owns it
    with the extent table (`extents`, device (n, 2) int32; `extents_host` the same on the
    host).  The images' tensors may be freed once the pack has run.  A list of equal shapes
    takes the same route.  RaggedDetFields.from_conv builds the same object from the head's
    conv outputs, without per-image fields and without the pack."""

    def __init__(self, fields):
        lib = load()
        fields = list(fields)
        if not fields:
            raise ValueError('a ragged batch needs at least one image')
        for f in fields:
            if not (isinstance(f, torch.Tensor) and _device.is_device(f) and
                    f.dtype == torch.float32 and f.is_contiguous() and f.dim() == 4):
                raise ValueError('ragged detection fields must be contiguous float32 device '
                                 'tensors (K, 7, h, w)')
            if f.shape[1] != 7:
                raise ValueError('expected CifDet fields (K, 7, h, w) per image, got {}'.format(
                    tuple(f.shape)))
        self.n = n = len(fields)
        self.k = fields[0].shape[0]
        if any(f.shape[0] != self.k for f in fields):
            raise ValueError('the images of a ragged batch differ in K: ' + ', '.join(
                sorted({'K={}'.format(f.shape[0]) for f in fields})))
        self.extents_host = np.array([f.shape[2:] for f in fields], np.int32).reshape(n, 2)
        self.h, self.w = (int(v) for v in self.extents_host.max(axis=0))
        dev = fields[0].device
        self.det = torch.empty((n, self.k, 7, self.h, self.w), dtype=torch.float32, device=dev)
        # pinned host tables (pointers, then extents): the copies are asynchronous, so the
        # tables live as long as this object
        size, ext_off = lib.pp_ragged_tables_size(n), lib.pp_ragged_extents_offset(n)
        self._host = torch.empty(size, dtype=torch.uint8, pin_memory=True)
        self._tables = torch.empty(size, dtype=torch.uint8, device=dev)
        host = self._host.numpy()
        host[:ext_off].view(np.uint64)[:] = [f.data_ptr() for f in fields]
        host[ext_off:].view(np.int32)[:] = self.extents_host.reshape(-1)
        self.extents = self._tables[ext_off:].view(torch.int32).view(n, 2)
        self.pack()

    _ingest = None  # from_conv: the head's heads.RaggedIngest

    @classmethod
    def from_conv(cls, convs, n_categories, quad=1, conv_extents=None, hflip=None):
        """The same object from the detection head's conv outputs, one HIP pass straight into
        the container (heads.fields_from_conv_ragged has the forms `convs` and `conv_extents`
        take; `hflip`: heads.HFlip() for a mirrored pass): no per-image fields and no pack.
        pack() runs the ingest launch again."""
        from .heads import RaggedIngest  # pylint: disable=import-outside-toplevel
        ingest = RaggedIngest(convs, n_categories, 'cifdet', quad, hflip, conv_extents)
        self = cls.__new__(cls)
        self.n, self.k, self.h, self.w = ingest.n, n_categories, ingest.h, ingest.w
        self.det = ingest.out
        self.extents, self.extents_host = ingest.extents, ingest.extents_host
        self._ingest = ingest
        self.pack()
        return self

    def pack(self):
        """The pack launch on the current stream, from the tables built at construction: again
        after the images' tensors were rewritten in place.  After from_conv: the ingest
        launch."""
        if self._ingest is not None:
            self._ingest.launch()
            return
        size, ext_off = self._host.numel(), load().pp_ragged_extents_offset(self.n)
        call('pp_fields_pack_ragged', ctypes.c_void_p(self._host.data_ptr()),
             ctypes.c_void_p(self._host.data_ptr() + ext_off), self.n, self.k, 7, self.h, self.w,
             _device.ptr(self.det), _device.ptr(self._tables), ctypes.c_size_t(size),
             _device.stream())


def check_head_lists(fc):
    """A multi-scale FieldConfig for a ragged batch names every head in every per-head list.
    The reference walks the lists with zip (cif_hr.py:69-78, cif_seeds.py:57-59,
    caf_scored.py:88-98), so a list shorter than cif_indices / caf_indices silently drops the
    heads behind it there: the default min-scale and distance lists of one entry beside two
    heads decode head 0 alone.  That truncation is not built for ragged batches."""
    nc, na = len(fc.cif_indices), len(fc.caf_indices)
    short = [name for name, want in (('cif_strides', nc), ('cif_min_scales', nc),
                                     ('caf_strides', na), ('caf_min_distances', na),
                                     ('caf_max_distances', na))
             if len(getattr(fc, name)) != want]
    if nc == 0 or na == 0 or short:
        raise NotImplementedError(
            'a ragged batch needs a single-scale FieldConfig, or a multi-scale one with one '
            'entry per head in every list: {} CIF and {} CAF heads, but {}'.format(
                nc, na, ', '.join('{} has {}'.format(name, len(getattr(fc, name)))
                                  for name in short) or 'no head of one kind'))


class RaggedHeadSet:
    """A batch of images of different field sizes under a multi-scale FieldConfig
    (pp_fields_pack_ragged_heads, pp_decode_multi_ragged): `fields_list` is one head list per
    image (what Generator.fields_batch returns), each head a float32 contiguous device tensor
    at its own size, CIF heads (K, 5, h, w) and CAF heads (C, 9, h, w), K and C the same for
    every head and image; `field_config` names the heads.  Packs all heads in one launch on
    the current stream into one container per head, (n, K, 5, H_m, W_m) / (n, C, 9, H_m, W_m)
    with (H_m, W_m) head m's largest size, zero outside each image's extent, and owns them
    (`cifs`, `cafs`) with the pp_scale array `arr` over them, the pinned host tables and the
    entry-major extent table (`extents`, device (n_heads, n, 2) int32, CIF heads first;
    `extents_host` the same on the host).  `shape_key` names the containers' shapes for the
    engine's buffer cache.  The images' tensors may be freed once the pack has run.
    RaggedHeadSet.from_conv builds the same object from the heads' conv outputs, without
    per-image fields and without the pack."""

    def __init__(self, fields_list, field_config):
        lib = load()
        fc = field_config
        fields_list = [list(f) for f in fields_list]
        if not fields_list:
            raise ValueError('a ragged batch needs at least one image')
        check_head_lists(fc)
        nc, na = len(fc.cif_indices), len(fc.caf_indices)
        index = list(fc.cif_indices) + list(fc.caf_indices)
        top = max(index)
        if any(len(f) <= top for f in fields_list):
            raise ValueError('an image has {} heads, the FieldConfig reads head {}'.format(
                min(len(f) for f in fields_list), top))
        # heads[m][i]: head m (CIF heads, then CAF heads: the pp_scale entry order) of image i.
        # One pass over the n_heads * n tensors collects what the tables need; the shapes are
        # then checked as one array
        heads = [[f[j] for f in fields_list] for j in index]
        f32, tensor = torch.float32, torch.Tensor
        shapes, ptrs = [], []
        for row in heads:
            for t in row:
                if not (isinstance(t, tensor) and t.is_cuda and t.dtype == f32
                        and t.is_contiguous()):
                    raise ValueError('ragged heads must be contiguous float32 device tensors '
                                     '(K, 5, h, w) and (C, 9, h, w)')
                shapes.append(t.shape)
                ptrs.append(t.data_ptr())
        self.n = n = len(fields_list)
        n_heads = nc + na
        if any(len(sh) != 4 for sh in shapes):
            raise ValueError('ragged heads must be contiguous float32 device tensors '
                             '(K, 5, h, w) and (C, 9, h, w)')
        shapes = np.array(shapes, np.int64).reshape(n_heads, n, 4)
        if (shapes[:nc, :, 1] != 5).any() or (shapes[nc:, :, 1] != 9).any():
            raise ValueError('expected CIF heads (K, 5, h, w) and CAF heads (C, 9, h, w)')
        self.k, self.c = int(shapes[0, 0, 0]), int(shapes[nc, 0, 0])
        if (shapes[:nc, :, 0] != self.k).any() or (shapes[nc:, :, 0] != self.c).any():
            raise ValueError('the heads of a ragged batch differ in K or C: K in {}, C in {}'.format(
                sorted(set(shapes[:nc, :, 0].reshape(-1).tolist())),
                sorted(set(shapes[nc:, :, 0].reshape(-1).tolist()))))
        self.extents_host = np.ascontiguousarray(shapes[:, :, 2:], np.int32)
        sizes = self.extents_host.max(axis=1)  # (n_heads, 2): the containers' (H, W)
        dev = heads[0][0].device
        outs = [torch.empty((n, row[0].shape[0], row[0].shape[1], int(hw[0]), int(hw[1])),
                            dtype=torch.float32, device=dev) for row, hw in zip(heads, sizes)]
        self.cifs, self.cafs = outs[:nc], outs[nc:]
        self.h, self.w = int(sizes[0][0]), int(sizes[0][1])
        self.stride0 = int(fc.cif_strides[0])
        self.pairs = int(nc == 10)  # cif_hr.py:63
        self.arr = scale_list([(t.data_ptr(), t.shape[3], t.shape[4]) for t in self.cifs],
                              [(t.data_ptr(), t.shape[3], t.shape[4]) for t in self.cafs],
                              fc.cif_strides, fc.caf_strides, fc.cif_min_scales,
                              fc.caf_min_distances, fc.caf_max_distances)
        self.shape_key = ('ragged', self.pairs) + tuple(
            (s.H, s.W, s.stride, s.role) for s in self.arr)
        # one pinned host block: pointers, extents (both copied to the device in one piece),
        # then the per-head planes, container sizes and container pointers the call reads;
        # the copy is asynchronous, so the block lives as long as this object
        size = lib.pp_ragged_heads_tables_size(n, n_heads)
        ext_off = lib.pp_ragged_heads_extents_offset(n, n_heads)
        self._size, self._ext_off, self._n_heads = size, ext_off, n_heads
        self._host = torch.empty(size + 20 * n_heads, dtype=torch.uint8, pin_memory=True)
        self._tables = torch.empty(size, dtype=torch.uint8, device=dev)
        host = self._host.numpy()
        host[:ext_off].view(np.uint64)[:] = ptrs
        host[ext_off:size].view(np.int32)[:] = self.extents_host.reshape(-1)
        tail = host[size:]
        tail[:8 * n_heads].view(np.uint64)[:] = [t.data_ptr() for t in outs]
        tail[8 * n_heads:12 * n_heads].view(np.int32)[:] = [t.shape[1] * t.shape[2] for t in outs]
        tail[12 * n_heads:].view(np.int32)[:] = sizes.reshape(-1)
        self.extents = self._tables[ext_off:].view(torch.int32).view(n_heads, n, 2)
        self.pack()

    _ingests = ()  # from_conv: the heads.RaggedIngest of each part, or one RaggedHeadsIngest
    _extents_pinned = None  # from_conv by a call per head: the host's extent table, pinned

    @staticmethod
    def _entry_parts(entry):
        """One item of from_conv's `entries` as a list of parts (convs, n_fields, hflip)."""
        from .heads import HFlip  # pylint: disable=import-outside-toplevel
        if isinstance(entry, torch.Tensor):
            return [(entry, None, None)]
        if (isinstance(entry, tuple) and len(entry) == 2 and
                (entry[1] is None or isinstance(entry[1], HFlip))):
            return [(entry[0], None, entry[1])]
        if (isinstance(entry, (list, tuple)) and entry and
                all(isinstance(p, tuple) and len(p) == 3 for p in entry)):
            return list(entry)
        return [(entry, None, None)]

    @classmethod
    def from_conv(cls, entries, field_config, quad=1, conv_extents=None, one_launch=False):
        """The same object from the heads' conv outputs, ingested straight into the containers:
        no per-image fields and no pack.

        `entries` is the model's head list, indexed as `field_config.cif_indices` /
        `caf_indices` index it.  An item is the head's convs, or (convs, hflip) with a
        heads.HFlip (heads.cif_hflip / caf_hflip) for a head of a mirrored pass; a CAF item may
        also be a list of parts (convs, n_fields, hflip) written side by side into one
        container (CAF and dense CAF).  `convs` is a list of per-image device tensors
        (ch, h_i, w_i) / (1, ch, h_i, w_i), or one batched (n, ch, hmax, wmax) tensor with
        `conv_extents` (n, 2), the forms heads.fields_from_conv_ragged takes.  float32, float16
        and bfloat16 are read as they lie, NCHW views and their channel, batch and row slices
        in place.  Every head has its own sizes; the images have the same K and C.

        The default is one pp_fields_from_conv_ragged call per head (heads.RaggedIngest),
        which measured faster than the one-launch form (DESIGN.md "Ragged multi-scale
        ingest"); it reads channels-last heads in place as well.  `one_launch` takes
        pp_fields_from_conv_ragged_heads (heads.RaggedHeadsIngest): one pinned host block and
        one library call for all heads.  There a channels-last view (or any view whose columns
        are not adjacent) is copied once into NCHW, that tensor only: the one-launch form has
        no channels-last kernel.  pack() runs the launches again, for use after the convs were
        rewritten in place."""
        from .heads import RaggedHeadsIngest, RaggedIngest  # pylint: disable=import-outside-toplevel
        fc = field_config
        check_head_lists(fc)
        entries = list(entries)
        nc = len(fc.cif_indices)
        index = list(fc.cif_indices) + list(fc.caf_indices)
        if len(entries) <= max(index):
            raise ValueError('the model has {} heads, the FieldConfig reads head {}'.format(
                len(entries), max(index)))
        groups = [cls._entry_parts(entries[j]) for j in index]
        self = cls.__new__(cls)
        if one_launch:
            ingest = RaggedHeadsIngest(
                [(convs, n_fields, 'cif' if g < nc else 'caf', hflip, g)
                 for g, parts in enumerate(groups) for convs, n_fields, hflip in parts],
                quad, conv_extents)
            self._ingests = [ingest]
            outs, self.extents, self.extents_host = ingest.outs, ingest.extents, ingest.extents_host
        else:
            self._ingests, outs = [], []
            for g, parts in enumerate(groups):
                kind, per_field = ('cif', 5 * 4 ** quad) if g < nc else ('caf', 9 * 4 ** quad)
                counts = [p[1] if p[1] is not None else cls._channels(p[0]) // per_field
                          for p in parts]
                first, done = None, 0
                for (convs, _, hflip), n_fields in zip(parts, counts):
                    ing = RaggedIngest(convs, n_fields, kind, quad, hflip, conv_extents,
                                       out=first.out if first else None, out_field0=done,
                                       out_fields=sum(counts))
                    if first is None:
                        first = ing
                        outs.append(ing.out)
                    elif not np.array_equal(ing.extents_host, first.extents_host):
                        raise ValueError('the parts of one container differ in conv size')
                    done += n_fields
                    # launched at once: the device works while the host builds the next head
                    self._ingests.append(ing.launch())
            sizes = sorted({i.n for i in self._ingests})
            if len(sizes) != 1:
                raise ValueError('the heads of a ragged batch have different numbers of '
                                 'images: ' + ', '.join(str(s) for s in sizes))
            firsts = [i for i in self._ingests if i.out_field0 == 0]
            self.extents_host = np.ascontiguousarray(np.stack([i.extents_host for i in firsts]))
            # the per-head calls write a table each: the joint one comes from the host's
            self._extents_pinned = torch.from_numpy(self.extents_host).pin_memory()
            self.extents = torch.empty(self.extents_host.shape, dtype=torch.int32,
                                       device=outs[0].device)
            self.extents.copy_(self._extents_pinned, non_blocking=True)
        self.n = self._ingests[0].n
        self.cifs, self.cafs = outs[:nc], outs[nc:]
        self.k, self.c = self.cifs[0].shape[1], self.cafs[0].shape[1]
        if any(t.shape[1] != self.k for t in self.cifs) or any(t.shape[1] != self.c
                                                               for t in self.cafs):
            raise ValueError('the heads of a ragged batch differ in K or C: K in {}, C in {}'.format(
                sorted({t.shape[1] for t in self.cifs}), sorted({t.shape[1] for t in self.cafs})))
        self.h, self.w = self.cifs[0].shape[3], self.cifs[0].shape[4]
        self.stride0 = int(fc.cif_strides[0])
        self.pairs = int(nc == 10)  # cif_hr.py:63
        self.arr = scale_list([(t.data_ptr(), t.shape[3], t.shape[4]) for t in self.cifs],
                              [(t.data_ptr(), t.shape[3], t.shape[4]) for t in self.cafs],
                              fc.cif_strides, fc.caf_strides, fc.cif_min_scales,
                              fc.caf_min_distances, fc.caf_max_distances)
        self.shape_key = ('ragged', self.pairs) + tuple(
            (s.H, s.W, s.stride, s.role) for s in self.arr)
        if one_launch:
            self.pack()
        return self

    @staticmethod
    def _channels(convs):
        """The channel count of a head's convs (a batched tensor or a list of per-image ones)."""
        if isinstance(convs, torch.Tensor):
            return convs.shape[1] if convs.dim() == 4 else 0
        convs = list(convs)
        ok = convs and isinstance(convs[0], torch.Tensor) and convs[0].dim() >= 3
        return convs[0].shape[-3] if ok else 0

    def pack(self):
        """The pack launch on the current stream, from the tables built at construction: again
        after the images' tensors were rewritten in place.  After from_conv: the ingest
        launches."""
        for ingest in self._ingests:
            ingest.launch()
        if self._ingests:
            if self._extents_pinned is not None:
                self.extents.copy_(self._extents_pinned, non_blocking=True)
            return
        base, size, nh = self._host.data_ptr(), self._size, self._n_heads
        call('pp_fields_pack_ragged_heads', ctypes.c_void_p(base),
             ctypes.c_void_p(base + self._ext_off), self.n, nh,
             ctypes.c_void_p(base + size + 8 * nh), ctypes.c_void_p(base + size + 12 * nh),
             ctypes.c_void_p(base + size), _device.ptr(self._tables), ctypes.c_size_t(size),
             _device.stream())


def _buffer_key(n, k, c, shape, cap, cfg):
    return (n, k, c, shape, cap, cfg.force_complete, cfg.stride, cfg.occupancy_reduction)


class DecodeEngine:
    def __init__(self):
        self._bufs = None
        # annotations per image of the last checked decode: dense batches (>= 32) get the
        # 8-wave NMS (PP_STAGE_NMS_WIDE) in the next one, as DecodePipeline does
        self.density = 0.0

    def buffers(self, n, k, c, h, w, cfg, cap, heads=None):
        shape = (h, w) if heads is None else heads.shape_key
        key = _buffer_key(n, k, c, shape, cap, cfg)
        if self._bufs is None or self._bufs.key != key:
            self._bufs = None  # free the previous workspace first
            self._bufs = DecodeBuffers(key, n, k, c, h, w, cfg, cap, _device.require(), heads)
        return self._bufs

    def _prepare(self, skeleton, n, k, c, h, w, cfg, cap, stages, heads=None):
        """What every launch starts with: the skeleton as an array of c pairs, the annotation
        capacity, the buffers of this shape and, for a call that starts stage 8, their next
        slot.  Returns (skel, cap, buffers)."""
        skel = skeleton_array(skeleton)
        if len(skel) != c:
            raise ValueError('skeleton has {} edges but caf has {} fields'.format(len(skel), c))
        cap = cap or default_ann_capacity(h, w)
        b = self.buffers(n, k, c, h, w, cfg, cap, heads)
        if stages & STAGE_GROW and not stages & STAGE_AFTER_SEED_LOOP:
            b.next_slot()
        return skel, cap, b

    def launch(self, cif, caf, skeleton, cfg, cap=None, keep_cifhr=False, stages=STAGE_ALL,
               initial=None):
        """Enqueue the decode on the current stream; returns the DecodeBuffers.  `initial`
        (InitialAnnotations) selects pp_decode_initial."""
        if cif.dim() != 5 or caf.dim() != 5 or cif.shape[2] != 5 or caf.shape[2] != 9:
            raise ValueError('expected cif (B, K, 5, H, W) and caf (B, C, 9, H, W)')
        n, k, _, h, w = cif.shape
        c = caf.shape[1]
        if caf.shape[0] != n or caf.shape[3:] != cif.shape[3:]:
            raise ValueError('cif and caf batch / spatial shapes differ')
        skel, cap, b = self._prepare(skeleton, n, k, c, h, w, cfg, cap, stages)
        hr = b.cifhr_buffer() if keep_cifhr else None
        if initial is not None:
            arr = scale_list([(cif.data_ptr(), h, w)], [(caf.data_ptr(), h, w)], [cfg.stride],
                             [cfg.stride])
            self._launch_initial(b, arr, 0, n, k, c, skel, cfg, hr, cap, initial, stages)
            return b
        call('pp_decode_stages', _device.ptr(cif), _device.ptr(caf), n, k, c, h, w,
             skel.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cfg), _device.ptr(hr),
             _device.ptr(b.anns), cap, _device.ptr(b.counts), _device.ptr(b.status),
             _device.ptr(b.ws), ctypes.c_size_t(b.ws.numel()), ctypes.c_uint32(stages),
             _device.stream())
        return b

    @staticmethod
    def _launch_initial(b, arr, pairs, n, k, c, skel, cfg, hr, cap, initial, stages):
        if initial.n != n:
            raise ValueError('initial annotations for {} images, batch has {}'.format(
                initial.n, n))
        # out_index is exactly (n * cap) long, image i's rows at [i * cap, (i + 1) * cap) as
        # the kernel writes them (the store behind it only grows)
        store = getattr(b, '_out_index_store', None)
        if store is None or store.numel() < n * cap:
            store = b._out_index_store = torch.empty(n * cap, dtype=torch.int32,
                                                     device=b.ws.device)
        b.out_index = store[:n * cap]
        b.out_index_cap = cap
        call('pp_decode_initial', arr, len(arr), pairs, n, k, c,
             skel.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cfg), _device.ptr(hr),
             _device.ptr(b.anns), cap, _device.ptr(b.counts), _device.ptr(b.status),
             _device.ptr(initial.records), _device.ptr(initial.counts), initial.cap,
             _device.ptr(b.out_index), _device.ptr(b.ws), ctypes.c_size_t(b.ws.numel()),
             ctypes.c_uint32(stages), _device.stream())

    def launch_ragged(self, ragged, skeleton, cfg, cap=None, stages=STAGE_ALL):
        """pp_decode_ragged over a RaggedFields, with launch's buffers at the container's
        shape; returns the DecodeBuffers."""
        n, k, c, h, w = ragged.n, ragged.k, ragged.c, ragged.h, ragged.w
        skel, cap, b = self._prepare(skeleton, n, k, c, h, w, cfg, cap, stages)
        call('pp_decode_ragged', _device.ptr(ragged.cif), _device.ptr(ragged.caf), n, k, c, h, w,
             _device.ptr(ragged.extents), ragged.extents_host.ctypes.data_as(ctypes.c_void_p),
             skel.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cfg), ctypes.c_void_p(0),
             _device.ptr(b.anns), cap, _device.ptr(b.counts), _device.ptr(b.status),
             _device.ptr(b.ws), ctypes.c_size_t(b.ws.numel()), ctypes.c_uint32(stages),
             _device.stream())
        return b

    def launch_ragged_multi(self, ragged, skeleton, cfg, cap=None, stages=STAGE_ALL):
        """pp_decode_multi_ragged over a RaggedHeadSet, with launch_multi's buffers at the
        containers' shapes; returns the DecodeBuffers."""
        n, k, c = ragged.n, ragged.k, ragged.c
        skel, cap, b = self._prepare(skeleton, n, k, c, ragged.h, ragged.w, cfg, cap, stages,
                                     ragged)
        call('pp_decode_multi_ragged', ragged.arr, len(ragged.arr), ragged.pairs, n, k, c,
             _device.ptr(ragged.extents), ragged.extents_host.ctypes.data_as(ctypes.c_void_p),
             skel.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cfg), ctypes.c_void_p(0),
             _device.ptr(b.anns), cap, _device.ptr(b.counts), _device.ptr(b.status),
             _device.ptr(b.ws), ctypes.c_size_t(b.ws.numel()), ctypes.c_uint32(stages),
             _device.stream())
        return b

    def launch_multi(self, heads, skeleton, cfg, cap=None, keep_cifhr=False, stages=STAGE_ALL,
                     initial=None):
        """pp_decode_multi over a HeadSet (pp_decode_initial with `initial`); returns the
        DecodeBuffers."""
        skel, cap, b = self._prepare(skeleton, heads.n, heads.k, heads.c, heads.h, heads.w, cfg,
                                     cap, stages, heads)
        hr = b.cifhr_buffer() if keep_cifhr else None
        if initial is not None:
            self._launch_initial(b, heads.arr, heads.pairs, heads.n, heads.k, heads.c, skel, cfg,
                                 hr, cap, initial, stages)
            return b
        call('pp_decode_multi', heads.arr, len(heads.arr), heads.pairs, heads.n, heads.k,
             heads.c, skel.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cfg), _device.ptr(hr),
             _device.ptr(b.anns), cap, _device.ptr(b.counts), _device.ptr(b.status),
             _device.ptr(b.ws), ctypes.c_size_t(b.ws.numel()), ctypes.c_uint32(stages),
             _device.stream())
        return b

    def launch_checked(self, cif, caf, skeleton, cfg, cap=None, keep_cifhr=False, heads=None,
                       initial=None, ragged=None):
        """launch / launch_multi / launch_ragged / launch_ragged_multi with overflow retry (the
        annotation capacity doubles until no image overflows); returns the DecodeBuffers of a
        decode whose records are complete.  Raises PPError on the overflows a retry cannot
        fix.  With a RaggedFields or RaggedHeadSet `ragged`, cif / caf are ignored."""
        if ragged is not None:
            if heads is not None:
                raise NotImplementedError('a ragged batch carries its own heads (a '
                                          'RaggedHeadSet as `ragged`), no HeadSet beside it')
            if initial is not None:
                raise NotImplementedError('a ragged batch takes no initial annotations')
            if keep_cifhr:
                raise NotImplementedError('a ragged batch keeps no dense CifHr map (no layout '
                                          'is defined for one)')
            h, w = ragged.h, ragged.w
        else:
            h, w = (cif.shape[3], cif.shape[4]) if heads is None else (heads.h, heads.w)
        cap = cap or default_ann_capacity(h, w)
        stages = STAGE_ALL | (STAGE_NMS_WIDE if self.density >= _B_FIRST_DENSITY else 0)
        while True:
            if isinstance(ragged, RaggedHeadSet):
                b = self.launch_ragged_multi(ragged, skeleton, cfg, cap=cap, stages=stages)
            elif ragged is not None:
                b = self.launch_ragged(ragged, skeleton, cfg, cap=cap, stages=stages)
            elif heads is None:
                b = self.launch(cif, caf, skeleton, cfg, cap=cap, keep_cifhr=keep_cifhr,
                                stages=stages, initial=initial)
            else:
                b = self.launch_multi(heads, skeleton, cfg, cap=cap, keep_cifhr=keep_cifhr,
                                      stages=stages, initial=initial)
            status = b.status.cpu().numpy()
            if len(status):
                self.density = float(b.counts[:len(status)].float().mean())
            if not (status & PP_ST_ANN_OVERFLOW).any():
                break
            cap *= 2
            LOG.info('annotation capacity overflow, retrying with %d per image', cap)
        if (status & PP_ST_NMS_OVERFLOW).any():
            raise PPError('NMS occupancy grid exceeds the workspace (keypoints far outside '
                          'the field); status={}'.format(status.tolist()))
        if (status & PP_ST_DEC_OVERFLOW).any():
            raise PPError('decoding/frontier order exceeded the record capacity')
        return b

    def decode(self, cif, caf, skeleton, cfg, cap=None, keep_cifhr=False, heads=None,
               compact=None, initial=None, ragged=None):
        """Full decode with overflow retry.  Returns (records, offsets, buffers).  With a
        HeadSet `heads`, cif / caf are ignored and the multi-scale decode runs.  `compact`
        flags (e.g. _abi.PACK_ALL) fetch compact records (pp_pack_compact) instead of full
        pp_ann records.  `initial` (InitialAnnotations): grown before the seed loop; the
        buffers then hold out_index (see pp_decode_initial).  `ragged` (RaggedFields, or a
        RaggedHeadSet for a multi-scale FieldConfig): the images decode at their own sizes
        (pp_decode_ragged / pp_decode_multi_ragged); cif / caf are ignored."""
        b = self.launch_checked(cif, caf, skeleton, cfg, cap=cap, keep_cifhr=keep_cifhr,
                                heads=heads, initial=initial, ragged=ragged)
        k = ragged.k if ragged is not None else cif.shape[1] if heads is None else heads.k
        recs, offsets = self.fetch(b, None if compact is None else
                                   (k, len(skeleton_array(skeleton)), compact))
        return recs, offsets, b

    def decode_async(self, cif, caf, skeleton, cfg, heads=None, compact=PACK_ALL,
                     device_out=False):
        """decode() up to the record pack: (buffers, PendingRecords of compact records, or
        full ones with compact=None).  `device_out` packs into device memory (what a
        multi-GPU rank sends, distributed.decode_sharded)."""
        b = self.launch_checked(cif, caf, skeleton, cfg, heads=heads)
        k = cif.shape[1] if heads is None else heads.k
        spec = None if compact is None else (k, len(skeleton_array(skeleton)), compact)
        return b, self.fetch_async(b, spec, device_out=device_out)

    @staticmethod
    def fetch(b, compact=None):
        """Packed records of all images and per-image offsets of the last decode into `b`
        (fetch_async(b).result())."""
        return DecodeEngine.fetch_async(b, compact).result()

    @staticmethod
    def fetch_async(b, compact=None, device_out=False, capacity=0, stream=None):
        """Enqueue the record fetch of the last decode into `b` on a side stream and return a
        PendingRecords; its result() waits for it.

        The records are packed image after image straight into a pinned host block
        (zero-copy through its mapped device address) together with the per-image counts,
        so one synchronisation hands over everything.  `compact` = (K, C, flags) selects
        pp_pack_compact's compact records (include/pifpaf_amd.h); None the full pp_ann
        records (pp_pack_records).  `device_out` packs the records into a device buffer
        instead (the multi-GPU gather sends them from there); the counts still land in
        pinned host memory.  The block is sized from the largest batch seen so far
        (`capacity` = records to reserve at least); result() re-packs a batch that outgrew
        it, and fetches full records when a compact record is flagged PP_PACK_REFETCH.  The
        slot stays valid until the second decode after this one, so a caller may launch the
        next decode before calling result().  `stream`: pack there instead of on the
        engine's pack stream."""
        est = max(getattr(b, 'pack_cap', 0), 16 * b.n, capacity)
        decoded = torch.cuda.Event()
        decoded.record()
        p = DecodeEngine._pack(b, b.anns, b.counts, b.status, compact, device_out, est, decoded,
                               stream)
        b._free[b._cur] = p.done_event
        return p

    @staticmethod
    def fetch_coco_async(b, metas, image_ids, *, hswap=None, small_threshold=0.0,
                         max_per_image=20, category_id=1, capacity=0, stream=None):
        """Enqueue the COCO prediction records (EvalCoco.from_predictions,
        eval_coco.py:108-158) of the last decode into `b` and return an
        eval_coco.PendingCoco; its result() waits and gives the batch's CocoRecords.

        As fetch_async: on the engine's pack stream (or `stream`) after the decode, the
        records written image after image straight into a pinned host block behind the
        counts, the decode's status and the per-image flags, and packed again into a larger
        block should the batch outgrow `capacity` records.  `metas` (device META_DTYPE
        bytes), `image_ids` (device int64) and `hswap` (device int32 or None) as
        eval_coco.metas_device builds them.  The decode's records are only read; result()
        raises PPError when the decode set an overflow bit."""
        from .eval_coco import coco_records_async  # pylint: disable=import-outside-toplevel
        decoded = torch.cuda.Event()
        decoded.record()
        side = DecodeEngine._pack_stream(b.anns.device) if stream is None else stream
        side.wait_event(decoded)
        recs = b.anns.view(b.n, b.cap, ANN_DTYPE.itemsize)
        p = coco_records_async(recs, b.counts, metas, image_ids, k=b.k, hswap=hswap,
                               small_threshold=small_threshold, max_per_image=max_per_image,
                               category_id=category_id, status=b.status, capacity=capacity,
                               stream=side)
        b._free[b._cur] = p.done_event
        return p

    @staticmethod
    def _pack(b, anns, counts, status, compact, device_out, est, after, stream=None):
        n = b.n
        dtype = ANN_DTYPE if compact is None else packed_dtype(*compact)
        width = dtype.itemsize
        # head: counts (n int32), the slot's status (n int32), per-image refetch flags
        # (n int32, pp_pack_compact's out_flags), then the records
        head = -(-12 * n // 256) * 256
        host = torch.empty(head + (0 if device_out else est * width), dtype=torch.uint8,
                           pin_memory=True)
        if compact is None:
            host[8 * n:12 * n].zero_()
        dev = (torch.empty(est * width, dtype=torch.uint8, device=anns.device)
               if device_out else None)
        out_ptr = dev.data_ptr() if device_out else host.data_ptr() + head
        # the pack runs on a side stream after the decode, so its PCIe writes overlap the
        # next decode; the slot is not rewritten before it is done (DecodeBuffers.next_slot)
        side = DecodeEngine._pack_stream(anns.device) if stream is None else stream
        side.wait_event(after)
        with torch.cuda.stream(side):
            if compact is None:
                call('pp_pack_records', _device.ptr(anns), _device.ptr(counts), n, b.cap,
                     ctypes.c_void_p(out_ptr), est, ctypes.c_void_p(host.data_ptr()),
                     _device.stream())
            else:
                k, c, flags = compact
                call('pp_pack_compact', _device.ptr(anns), _device.ptr(counts), n, b.cap,
                     k, c, ctypes.c_uint32(flags), ctypes.c_void_p(out_ptr), est,
                     ctypes.c_void_p(host.data_ptr()),
                     ctypes.c_void_p(host.data_ptr() + 8 * n), _device.stream())
            host[4 * n:8 * n].copy_(status.view(torch.uint8), non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            if dev is not None:
                dev.record_stream(side)
        return PendingRecords(b, (anns, counts, status), host, head, est, done, dtype, dev,
                              compact, device_out)

    _pack_streams = {}

    @staticmethod
    def _pack_stream(device):
        if device not in DecodeEngine._pack_streams:
            DecodeEngine._pack_streams[device] = torch.cuda.Stream(device=device)
        return DecodeEngine._pack_streams[device]

    @staticmethod
    def fetch_gather(b, anns=None, counts=None):
        """Packed records of all images (one gather + one D2H copy) and per-image offsets;
        `anns` / `counts` select an output slot (default: the last decode's)."""
        anns = b.anns if anns is None else anns
        counts = (b.counts if counts is None else counts).cpu().numpy().astype(np.int64)
        offsets = np.concatenate([[0], np.cumsum(counts)])
        total = int(offsets[-1])
        if total == 0:
            return np.zeros(0, ANN_DTYPE), offsets
        # row of record r of image i is i * cap + r: one vectorised gather index
        idx = np.arange(total, dtype=np.int64) + np.repeat(
            np.arange(len(counts), dtype=np.int64) * b.cap - offsets[:-1], counts)
        rows = anns.view(b.n * b.cap, ANN_DTYPE.itemsize)
        sel = rows.index_select(0, torch.from_numpy(idx).to(rows.device))
        # pinned destination from torch's caching host allocator: full-rate D2H, and the
        # returned array owns the block (released to the cache when the caller drops it)
        host = torch.empty(sel.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(sel, non_blocking=True)
        torch.cuda.current_stream(rows.device).synchronize()
        return host.numpy().reshape(-1).view(ANN_DTYPE), offsets


class PendingRecords:
    """A record fetch enqueued by DecodeEngine.fetch_async."""

    def __init__(self, b, slot, host, head, est, done, dtype, dev=None, compact=None,
                 device_out=False):
        self._b, self._slot = b, slot
        self._host, self._head, self._est, self._done = host, head, est, done
        self.dtype, self.device_records = dtype, dev
        self._compact, self._device_out = compact, device_out
        self._waited = False
        self.on_counts = None  # callback(counts) once the pack is waited for

    def __del__(self):
        # the pinned block goes back to torch's host cache when this object dies; the raw
        # pack kernel must have finished writing it by then
        if not self._waited and self._done is not None:
            try:
                self._done.synchronize()
            except Exception:  # pylint: disable=broad-except
                pass

    def wait(self):
        """Wait for the pack; per-image counts (int64).  Raises PPError when the decode set
        an overflow bit (its records are truncated)."""
        n = self._b.n
        self._done.synchronize()
        self._waited = True
        status = self._host[4 * n:8 * n].numpy().view(np.int32)
        if self.on_counts is not None:
            self.on_counts(self._host[:4 * n].numpy().view(np.int32))
        bad = status & (PP_ST_ANN_OVERFLOW | PP_ST_DEC_OVERFLOW | PP_ST_NMS_OVERFLOW)
        if bad.any():
            raise PPError('decode status flags set (records truncated; decode() retries with '
                          'more capacity): {}'.format(status[bad != 0][:8].tolist()))
        return self._host[:4 * n].numpy().view(np.int32).astype(np.int64)

    @property
    def done_event(self):
        return self._done

    @property
    def refetch(self):
        """True when a compact record of this fetch is flagged PP_PACK_REFETCH (valid after
        wait(); from pp_pack_compact's per-image flags, so device-resident records need not
        be read)."""
        n = self._b.n
        return bool(self._host[8 * n:12 * n].numpy().view(np.int32).any())

    def host_records(self):
        """The pinned block's record area (a CPU uint8 tensor; valid after wait())."""
        return self._host[self._head:]

    def fits(self, total):
        return total <= self._est

    def result(self):
        """(records, offsets) once the fetch has completed (waits for it).  Records are
        self.dtype, or full ANN_DTYPE records after a refetch."""
        width = self.dtype.itemsize
        counts = self.wait()
        offsets = np.concatenate([[0], np.cumsum(counts)])
        total = int(offsets[-1])
        if total > self._est:  # outgrew the block: pack again into one that fits
            self._b.pack_cap = 2 * total
            after = torch.cuda.Event()
            after.record(DecodeEngine._pack_stream(self._slot[0].device))
            return DecodeEngine._pack(self._b, *self._slot, self._compact, self._device_out,
                                      2 * total, after).result()
        if self.device_records is not None:
            host = torch.empty(total * width, dtype=torch.uint8, pin_memory=True)
            host.copy_(self.device_records[:total * width])
            recs = host.numpy().view(self.dtype)
        else:
            recs = self._host[self._head:self._head + total * width].numpy().view(self.dtype)
        if self.refetch:
            return DecodeEngine.fetch_gather(self._b, self._slot[0], self._slot[1])
        return recs, offsets

    def full_device_records(self):
        """The decode's full pp_ann records as one device uint8 tensor (image after image;
        what a multi-GPU rank sends instead of compact records after a refetch)."""
        b, anns = self._b, self._slot[0]
        counts = self.wait()
        offsets = np.concatenate([[0], np.cumsum(counts)])
        idx = np.arange(int(offsets[-1]), dtype=np.int64) + np.repeat(
            np.arange(len(counts), dtype=np.int64) * b.cap - offsets[:-1], counts)
        rows = anns.view(b.n * b.cap, ANN_DTYPE.itemsize)
        return rows.index_select(0, torch.from_numpy(idx).to(rows.device)).reshape(-1)


# The pipeline's scheduling choices are module constants, not environment switches (tests
# set them to check that every order gives the same records).
# _B_FIRST: the force-complete set order of DecodePipeline, True / False / 'lazy' (gated
# after the seed loop, on the tail stream); None: auto below
_B_FIRST = None
# auto: lazy sets (only the (field, direction) pairs force-complete needs, on the tail
# stream) until a batch averaged this many annotations per image, then sets first.  Round 4,
# with the tail split: planted cfg3 0.687-0.691 (lazy) vs 0.801-0.811 ms (first) per step,
# uniform 14.7k vs 15.1-15.2k images/s, cfg5 planted equal, cfg5 uniform 1180 vs 1200
_B_FIRST_DENSITY = 32.0
# workspaces in flight: batch i + depth's front half waits for batch i's tail
_PIPE_DEPTH = 2
# the tail as two calls (force-complete, then NMS): a workspace's next front half waits only
# for the force-complete, its next seed loop for the NMS (False: one call, the front half
# waits for both)
_SPLIT_TAIL = True
# Sparse batches: batch i's seed loop and tail share the back stream of its workspace
# (i % 2), so a seed loop starts beside the previous batch's slowest images (cfg5 planted
# 30.5k -> 41.7k images/s, cfg3 planted equal); dense ones: one stream for the seed loops
# and one for the tails (cfg3 uniform 15.5k vs 14.6k images/s); True / False forces either.
# The same two streams serve both (current + the library's side stream + two: four
# hardware queues).
_BACK2 = None


class DecodePipeline:
    """Decodes a sequence of batches with consecutive batches overlapped on the device.

    A decode has a bandwidth-bound front half (CifHr, seeds, CafScored: stages 1 | 2 | 4,
    here with the force-complete column sets too, STAGE_COMPLETE_EARLY) and a
    latency-bound back half: the seed loop, then force-complete and NMS (stage 8 in two
    calls).  Batch i's front half runs on the caller's current stream, its seed loop on a
    back stream that waits for it, and its force-complete, NMS and record pack on a tail
    stream that waits for the seed loop.  So batch i + 1's front half runs beside batch i's
    seed loop, and batch i + 1's seed loop beside batch i's tail.  Two engines (two
    workspaces) alternate; a workspace's front half waits until the tail that last used it
    is done, and its output slots are released by their record packs as in DecodeEngine.
    The tail is two calls (STAGE_COMPLETE_ONLY, then STAGE_NMS_ONLY): the workspace's next
    front half waits only for the force-complete (the last reader of the stage 1-4 buffers),
    its next seed loop for the NMS.
    (The front half stays on the current stream and the pack on the tail stream so that
    the streams in use -- current, back, tail, the library's CafScored side stream -- each
    get a hardware queue of their own: HIP shares 4 per process between streams.)
    For sparse batches the same two streams are used per workspace instead: batch i's seed
    loop and its tail both go on stream i % 2, so batch i + 1's seed loop can start on the
    CUs that batch i's finished images left (the loop ends with its slowest image); every
    order between batches is an event either way.

    The force-complete sets are lazy for sparse batches (built after the seed loop on the
    tail stream, only for the (field, direction) pairs an annotation left unset), and go
    first for dense ones, on the side stream before the CifHr map (they read only the CAF
    fields), then set A after them, beside the CifHr map and the seeds on the current
    stream (_B_FIRST = True / False / 'lazy' forces first / after set A / lazy).  Every order
    gives the same records.

    submit() returns (buffers, PendingRecords of the batch: DecodeEngine.fetch_async).
    The current stream does not wait for the back half; the fields must stay unchanged
    until the batch's records are fetched."""

    def __init__(self, device=None, depth=None):
        self.device = _device.require() if device is None else device
        if depth is None:
            depth = _PIPE_DEPTH
        self.depth = max(2, depth)  # workspaces in flight (3 or 4 measured slower)
        self.engines = tuple(DecodeEngine() for _ in range(self.depth))
        # dense batches: seed loops on `back`, tails on `tail`; sparse ones: each workspace's
        # loop and tail on one of the two (_BACK2 above, per submit)
        # (a high HIP priority for the back, tail or a separate front stream measured no
        # better: planted 385-389k / 373-382k / 365-389k vs 390-391k images/s, round 4)
        self.back = torch.cuda.Stream(device=self.device)
        self.tail = torch.cuda.Stream(device=self.device)
        self._back_done = [None] * self.depth
        self._sets_done = [None] * self.depth  # end of force-complete (last reader of 1-4)
        self._i = 0
        self.density = 0.0  # annotations per image of the last batch whose records were read

    def submit(self, cif, caf, skeleton, cfg, cap=None, heads=None, compact=None,
               device_out=False, events=None):
        """Enqueue one batch (cif / caf, or a multi-scale HeadSet `heads`).  `events`
        (five torch.cuda.Events, optional) are recorded around the CifHr stage, the other
        front stages (front stream), at the seed loop's start (back stream) and at the end
        of NMS (tail stream); a sixth one, if given, at the seed loop's end (back stream)."""
        par = self._i % self.depth
        self._i += 1
        eng = self.engines[par]
        front = torch.cuda.current_stream(self.device)

        def launch(stages):
            if heads is None:
                return eng.launch(cif, caf, skeleton, cfg, cap=cap, stages=stages)
            return eng.launch_multi(heads, skeleton, cfg, cap=cap, stages=stages)

        if self._sets_done[par] is not None:  # the workspace's previous force-complete
            front.wait_event(self._sets_done[par])
        with torch.cuda.stream(front):
            if events:
                events[0].record()
            dense = self.density >= _B_FIRST_DENSITY
            b_first = _B_FIRST if _B_FIRST is not None else (True if dense else 'lazy')
            # dense batches: the 8-wave NMS (uniform cfg3 15.1-15.3k vs 14.4-14.5k images/s);
            # sparse ones: the 4-wave NMS runs beside the next seed loop (planted 370-375k
            # vs 385-394k, A/B on one box)
            wide = STAGE_NMS_WIDE if dense else 0
            early = 0 if b_first == 'lazy' else STAGE_COMPLETE_EARLY
            if b_first == 'lazy':
                launch(STAGE_CIFHR)
            elif b_first:
                # the force-complete sets start on the library's side stream before the
                # CifHr map (they read only the CAF fields); the next call's join covers them
                launch(STAGE_CIFHR | STAGE_COMPLETE_EARLY)
            else:
                launch(STAGE_CIFHR)
            if events:
                events[1].record()
            launch(STAGE_SEEDS | STAGE_CAF | (0 if b_first else early))
            if events:
                events[2].record()
            front_done = torch.cuda.Event()
            front_done.record()
        per_ws = _BACK2 if _BACK2 is not None else not dense
        if per_ws:  # loop + tail on the workspace's stream (every cross-batch order is an event)
            back = tail = (self.back, self.tail)[par % 2]
        else:
            back, tail = self.back, self.tail
        back.wait_event(front_done)
        if self._back_done[par] is not None:  # the workspace's previous NMS (records)
            back.wait_event(self._back_done[par])
        with torch.cuda.stream(back):
            if events:
                events[3].record()
            launch(STAGE_GROW | early | STAGE_SEED_LOOP_ONLY)
            if events and len(events) > 5:
                events[5].record()
            loop_done = torch.cuda.Event()
            loop_done.record()
        if tail is not back:
            tail.wait_event(loop_done)
        with torch.cuda.stream(tail):
            if _SPLIT_TAIL:
                launch(STAGE_GROW | early | STAGE_AFTER_SEED_LOOP | STAGE_COMPLETE_ONLY | wide)
                sets_done = torch.cuda.Event()
                sets_done.record()
                b = launch(STAGE_GROW | early | STAGE_AFTER_SEED_LOOP | STAGE_NMS_ONLY | wide)
            else:
                b = launch(STAGE_GROW | early | STAGE_AFTER_SEED_LOOP | wide)
                sets_done = None
            if events:
                events[4].record()
            back_done = torch.cuda.Event()
            back_done.record()
            pending = DecodeEngine.fetch_async(b, compact, device_out=device_out,
                                               stream=tail)
        pending.on_counts = self._note_counts
        self._back_done[par] = back_done
        self._sets_done[par] = sets_done or back_done
        return b, pending

    def _note_counts(self, counts):
        self.density = float(counts.mean()) if len(counts) else 0.0


# ---- the detection decoder's engine (decoder/generator/cifdet.py) ---------------------------
class DetBuffers:
    """Workspace + two output slots (records, counts, status) of one CifDet decode shape:
    DecodeBuffers for the detection decoder.  `bound` is the capacity no image can exceed
    (K * cells), where the overflow retry stops."""

    def __init__(self, key, n, cap, size, bound, device):
        self.key, self.n, self.cap, self.bound = key, n, cap, bound
        self.ws = torch.empty(size, dtype=torch.uint8, device=device)
        self._slots = [(torch.empty((n, cap, DET_DTYPE.itemsize), dtype=torch.uint8,
                                    device=device),
                        torch.zeros(n, dtype=torch.int32, device=device),
                        torch.zeros(n, dtype=torch.int32, device=device)) for _ in range(2)]
        self._cur = 0
        self._free = [None, None]  # per slot: event after which its records were packed
        self.decodes = [0, 0]  # per slot: decodes written into it so far
        self.busy = None  # event behind the last decode / pack enqueued on these buffers
        self.inputs = None  # (cifdet, device batch, config) of the last launch, for its retry

    out = property(lambda self: self._slots[self._cur][0])
    counts = property(lambda self: self._slots[self._cur][1])
    status = property(lambda self: self._slots[self._cur][2])

    def next_slot(self):
        """DecodeBuffers.next_slot: the other slot, once its previous records have been
        packed.  Counts the slot's decodes, so that a pending fetch can tell whether the slot
        still holds its records."""
        self._cur ^= 1
        self.decodes[self._cur] += 1
        if self._free[self._cur] is not None:
            torch.cuda.current_stream().wait_event(self._free[self._cur])
            self._free[self._cur] = None

    def storage(self):
        """data_ptr of the workspace and of each slot's records, counts and status."""
        return (self.ws.data_ptr(),) + tuple(t.data_ptr() for s in self._slots for t in s)


class DetEngine:
    """The persistent state of one CifDet: per (entry point, batch shape, capacity) a
    workspace and two output slots (DetBuffers), kept between calls, and the record
    hand-over through pp_pack_det_records.  launch() enqueues one decode, fetch_async() its
    pack into a pinned host block (records, counts and status: one synchronisation hands
    over everything), PendingDetRecords.result() waits.  A call of a shape seen before
    allocates nothing on the device.

    A slot is not rewritten before the pack that reads it is done (DecodeBuffers.next_slot),
    and a decode waits for whatever last used its workspace, on any stream, so decodes of one
    engine may be enqueued on different streams (DetPipeline).  The detection decode uses no
    library side stream: everything runs on the stream current at the call."""

    KEYS = 4  # shapes kept; the least recently used goes first

    def __init__(self):
        self._bufs = collections.OrderedDict()
        self.pack_cap = 0  # records the pinned block reserves: the largest batch seen, doubled

    def buffers(self, key, n, cap, size, bound, device):
        b = self._bufs.get(key)
        if b is not None:
            self._bufs.move_to_end(key)
            return b
        while len(self._bufs) >= self.KEYS:
            _, old = self._bufs.popitem(last=False)
            if old.busy is not None:  # its memory goes back to the allocator: work done first
                old.busy.synchronize()
        b = self._bufs[key] = DetBuffers(key, n, cap, size, bound, device)
        return b

    def storage(self):
        """{buffer key: DetBuffers.storage()} of the shapes held."""
        return {key: b.storage() for key, b in self._bufs.items()}

    def launch(self, cifdet, batch, cap=None, config=None):
        """Enqueue one decode on the current stream, no read-back; returns the DetBuffers,
        whose current slot the decode writes.  `batch`: a (B, K, 7, H, W) tensor, the list of
        the head tensors of a multi-head or min-scale FieldConfig, or a RaggedDetFields;
        pp_cifdet_decode, pp_cifdet_decode_multi or pp_cifdet_decode_ragged as
        CifDet.decode_device / decode_ragged_device choose.  `config`: the (pp_config,
        pp_det_nms) of an earlier launch instead of the decoder classes' attributes as they
        are now (the overflow retry decodes with what the first attempt read)."""
        lib = load()
        cfg, z = config or (cifdet.config(), cifdet.nms_config())
        fc = cifdet.field_config
        arr = pairs = None
        if isinstance(batch, RaggedDetFields):
            n, k, h, w = batch.n, batch.k, batch.h, batch.w
            kind, shape, cells, dev = 'ragged', (h, w), h * w, batch.det.device
            cap = cap or max(64, h * w)
            size = lib.pp_cifdet_ragged_workspace_size(n, k, h, w, ctypes.byref(cfg), cap)
        else:
            heads = cifdet.device_heads(batch)
            n, k, _, h, w = heads[0].shape
            cells, dev = sum(t.shape[3] * t.shape[4] for t in heads), heads[0].device
            cap = cap or max(64, h * w)
            if cifdet.single_head():
                kind, shape, batch = 'single', (h, w), heads[0]
                size = lib.pp_cifdet_workspace_size(n, k, h, w, ctypes.byref(cfg), cap)
            else:
                arr = scale_list([(t.data_ptr(), t.shape[3], t.shape[4]) for t in heads], [],
                                 fc.cif_strides, [], fc.cif_min_scales)
                pairs = int(len(heads) == 10)  # CifHr.fill's 10-head layout (cif_hr.py:68-73)
                kind, batch = 'multi', heads
                shape = (pairs,) + tuple((s.H, s.W, s.stride, s.cif_min_scale) for s in arr)
                size = lib.pp_cifdet_multi_workspace_size(arr, len(arr), pairs, n, k, cap)
        b = self.buffers((kind, n, k, shape, cap, int(size), dev), n, cap, int(size), k * cells,
                         dev)
        if b.busy is not None:
            torch.cuda.current_stream(dev).wait_event(b.busy)
        b.next_slot()
        out = (ctypes.byref(cfg), ctypes.byref(z), _device.ptr(None), _device.ptr(b.out), cap,
               _device.ptr(b.counts), _device.ptr(b.status), _device.ptr(b.ws),
               ctypes.c_size_t(b.ws.numel()), _device.stream())
        if kind == 'ragged':
            call('pp_cifdet_decode_ragged', _device.ptr(batch.det), n, k, h, w,
                 _device.ptr(batch.extents),
                 batch.extents_host.ctypes.data_as(ctypes.c_void_p), *out)
        elif kind == 'multi':
            call('pp_cifdet_decode_multi', arr, len(arr), pairs, n, k, *out)
        else:
            call('pp_cifdet_decode', _device.ptr(batch), n, k, h, w, *out)
        b.busy = torch.cuda.Event()
        b.busy.record()
        b.inputs = (cifdet, batch, (cfg, z))
        return b

    def fetch_async(self, b, capacity=0, stream=None):
        """Enqueue the record pack of the last decode into `b` and return a
        PendingDetRecords: pp_pack_det_records writes the counts, the decode's status and the
        records, image after image, straight into a pinned host block (zero-copy through its
        mapped address).  The block is sized from the largest batch seen (`capacity` = records
        to reserve at least); result() packs a batch that outgrew it again, or decodes it again
        should the slot have been rewritten meanwhile (the second decode into `b` after this
        one takes it).  On the current stream, behind the decode, or on `stream` after it."""
        est = max(self.pack_cap, 16 * b.n, capacity)
        p = self._pack(b, b._cur, b.inputs, est, stream)
        b._free[b._cur] = b.busy = p.done_event
        return p

    def _pack(self, b, slot_i, inputs, est, stream=None):
        n, slot = b.n, b._slots[slot_i]
        head = -(-8 * n // 256) * 256  # counts (n int32), status (n int32), then the records
        host = torch.empty(head + est * DET_DTYPE.itemsize, dtype=torch.uint8, pin_memory=True)
        cur = torch.cuda.current_stream(slot[0].device)
        side = cur if stream is None else stream
        if side != cur:
            side.wait_stream(cur)
        with torch.cuda.stream(side):
            base = host.data_ptr()
            call('pp_pack_det_records', _device.ptr(slot[0]), _device.ptr(slot[1]),
                 _device.ptr(slot[2]), n, b.cap, ctypes.c_void_p(base + head), est,
                 ctypes.c_void_p(base), ctypes.c_void_p(base + 4 * n), _device.stream())
            done = torch.cuda.Event()
            done.record()
        return PendingDetRecords(self, b, slot_i, inputs, host, head, est, done)

    def decode_async(self, cifdet, batch, cap=None, config=None):
        """launch + fetch_async: one decode and one pack on the current stream."""
        return self.fetch_async(self.launch(cifdet, batch, cap, config))


class PendingDetRecords:
    """A detection record fetch enqueued by DetEngine.fetch_async.  It keeps the decode's
    inputs alive, because result() decodes again when an image overflowed the capacity: the
    caller leaves them unchanged until result() returns."""

    def __init__(self, eng, b, slot_i, inputs, host, head, est, done):
        self._eng, self._b, self._slot_i, self._inputs = eng, b, slot_i, inputs
        self._cifdet, self._decode = inputs[0], b.decodes[slot_i]
        self._host, self._head, self._est, self._done = host, head, est, done
        self._waited, self._result = False, None

    def __del__(self):
        # the pinned block goes back to torch's host cache when this object dies; the raw
        # pack kernel must have finished writing it by then
        if not self._waited and self._done is not None:
            try:
                self._done.synchronize()
            except Exception:  # pylint: disable=broad-except
                pass

    @property
    def done_event(self):
        return self._done

    def wait(self):
        """Wait for the pack: (per-image counts int64, the decode's status words int32)."""
        n = self._b.n
        self._done.synchronize()
        self._waited = True
        words = self._host[:8 * n].numpy().view(np.int32)
        return words[:n].astype(np.int64), words[n:]

    def result(self):
        """(DET_DTYPE records of all images, per-image offsets) of a complete decode: waits
        for the pack; where an image overflowed, decodes again at doubled capacity (PPError
        once the capacity is K * cells and still overflows, as CifDet.decode_device); packs
        again into a larger block when the batch outgrew this one."""
        if self._result is not None:
            return self._result
        counts, status = self.wait()
        b, eng = self._b, self._eng
        if (status & PP_ST_ANN_OVERFLOW).any():
            if b.cap >= b.bound:
                raise PPError('CifDet: detection capacity overflow')
            cap = min(b.bound, 2 * b.cap)
            LOG.info('detection capacity overflow, retrying with %d per image', cap)
            cifdet, batch, config = self._inputs
            again = eng.decode_async(cifdet, batch, cap, config)
        else:
            offsets = np.concatenate([[0], np.cumsum(counts)])
            total = int(offsets[-1])
            if total <= self._est:
                size = total * DET_DTYPE.itemsize
                recs = self._host[self._head:self._head + size].numpy().view(DET_DTYPE)
                self._result = (recs, offsets)
                self._inputs = None
                return self._result
            eng.pack_cap = max(eng.pack_cap, 2 * total)  # outgrew the block
            if b.decodes[self._slot_i] == self._decode:  # the slot still holds the records
                # pylint: disable=protected-access
                again = eng._pack(b, self._slot_i, self._inputs, eng.pack_cap)
                b._free[self._slot_i] = again.done_event  # its next decode waits for this too
            else:  # rewritten by a later decode: once more from the inputs
                cifdet, batch, config = self._inputs
                again = eng.decode_async(cifdet, batch, b.cap, config)
        self._result = again.result()
        self._inputs = None
        return self._result

    def annotations(self):
        """One list of AnnotationDet per image (CifDet.decode_batch's lists)."""
        return self._cifdet.annotations_from_records(*self.result())


class DetPipeline:
    """Detection decodes of a sequence of batches, consecutive ones overlapped on the device:
    batch i's decode and its pack run on stream i % 2 of the pipeline's own two streams, after
    what the caller's current stream held at submit, so one batch's latency-bound select loop
    (one wave per field) runs beside the next batch's bandwidth-bound CifHr map.  `depth`
    engines (workspaces in flight, at least two) alternate; a decode waits for the pack that
    last used its workspace and for the pack that last read its slot (DetEngine.launch).
    The detection decode uses no library side stream, so a process has the current stream and
    these two in use (HIP shares 4 hardware queues per process between streams).

    submit() returns the batch's PendingDetRecords.  The current stream does not wait for the
    decode; the inputs stay unchanged until the batch's result() has returned."""

    def __init__(self, device=None, depth=2):
        self.device = _device.require() if device is None else device
        self.depth = max(2, depth)
        self.engines = tuple(DetEngine() for _ in range(self.depth))
        self.streams = tuple(torch.cuda.Stream(device=self.device) for _ in range(2))
        self._i = 0

    def submit(self, cifdet, batch, cap=None):
        """Enqueue one batch (DetEngine.launch's `batch`) for `cifdet`."""
        i = self._i
        self._i += 1
        stream = self.streams[i % 2]
        stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(stream):
            return self.engines[i % self.depth].decode_async(cifdet, batch, cap)


_ENGINE = None


def engine():
    global _ENGINE  # pylint: disable=global-statement
    if _ENGINE is None:
        _ENGINE = DecodeEngine()
    return _ENGINE
