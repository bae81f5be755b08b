"""Network-output ingestion on the device (network/heads.py).

`fields_from_conv` turns the raw conv output of a CompositeFieldFused head into the
decoder's fields in one HIP pass (pp_fields_from_conv): the eval-mode tail of
CompositeFieldFused.forward (heads.py:406-455) and CifCafCollector / CifdetCollector
(heads.py:65-88, 127-144) fused.  `CifCafCollector` keeps the reference collector's role
for a model whose heads stop at their conv: forward(conv outputs) -> (cif, caf).

The same pass reads float16 / bfloat16 conv outputs directly and undoes the horizontal
flip of a mirrored pass (heads.PifHFlip / PafHFlip, heads.py:145-214; pp_fields_from_conv_ex).
Channels-last tensors and channel, batch or spatial slices of a larger tensor are read where
they lie, by their strides (pp_fields_from_conv_strided).
`MultiScaleCollector` does that for the head list of a ShellMultiScale-style model
(network/nets.py:95-143), whose second five scales come from the mirrored image.
`fields_from_conv_ragged` / `RaggedCollector` ingest the conv outputs of images of different
sizes straight into the containers of a ragged batch (pp_fields_from_conv_ragged, and
pp_fields_from_conv_ragged_interleaved for channels-last conv outputs, read in place too);
`RaggedDetCollector` does it for a detection head (engine.RaggedDetFields).
`RaggedHeadsIngest` / `RaggedMultiScaleCollector` ingest every head of a multi-scale model, all
images, in one launch (pp_fields_from_conv_ragged_heads, engine.RaggedHeadSet.from_conv).
"""
import ctypes

import numpy as np
import torch

from . import _device, constants
from ._lib import call, load

LAYOUTS = {'cif': (0, 5), 'caf': (1, 9), 'cifdet': (2, 7)}
_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}  # PP_DTYPE_*


def fields_dim(n, quad):
    """Field size after `quad` PixelShuffle(2) dequads with the last row / column dropped."""
    return int(load().pp_fields_dim(int(n), int(quad)))


class HFlip:
    """What un-flipping a head of a horizontally mirrored pass takes besides mirroring the
    columns and negating the x offsets: `src_field[f]` = the conv field that output field f
    reads (the left / right permutation) and, for a CAF head, `swap_ends[f]` = 1 where the
    edge's direction reverses, so that its two end points trade places.  HFlip() alone is
    the mirror without tables (a CifDet head)."""

    def __init__(self, src_field=None, swap_ends=None):
        self.src_field = None if src_field is None else tuple(int(v) for v in src_field)
        self.swap_ends = None if swap_ends is None else tuple(int(bool(v)) for v in swap_ends)
        self._src = self._swap = None
        if self.src_field is not None:
            self._src = (ctypes.c_int32 * len(self.src_field))(*self.src_field)
        if self.swap_ends is not None:
            self._swap = (ctypes.c_uint8 * len(self.swap_ends))(*self.swap_ends)

    def tables(self, n_fields):
        for t in (self.src_field, self.swap_ends):
            if t is not None and len(t) != n_fields:
                raise ValueError('hflip table has {} entries for {} fields'.format(
                    len(t), n_fields))
        return self._src, self._swap


def cif_hflip(keypoints, hflip=constants.HFLIP):
    """The table of heads.PifHFlip (heads.py:149-152): field kp reads its mirror partner."""
    return HFlip([keypoints.index(hflip[name]) if name in hflip else i
                  for i, name in enumerate(keypoints)])


def caf_hflip(keypoints, skeleton, hflip=constants.HFLIP):
    """The tables of heads.PafHFlip (heads.py:173-191), built in its order: an edge whose
    mirror image is in the skeleton reads that edge, and one whose mirror image is there
    reversed reads that one and has its end points exchanged (the later match wins)."""
    names = [(keypoints[j1 - 1], keypoints[j2 - 1]) for j1, j2 in skeleton]
    flipped = [(hflip.get(n1, n1), hflip.get(n2, n2)) for n1, n2 in names]
    src_field = list(range(len(names)))
    swap_ends = [0] * len(names)
    for i, (n1, n2) in enumerate(names):
        if (n1, n2) in flipped:
            src_field[i] = flipped.index((n1, n2))
        if (n2, n1) in flipped:
            src_field[i] = flipped.index((n2, n1))
            swap_ends[i] = 1
    return HFlip(src_field, swap_ends)


def _in_place(conv):
    """Whether pp_fields_from_conv_strided reads this (B, C, h, w) tensor as it lies: its
    columns or its channels are adjacent (the stride of an extent-1 dimension says nothing)."""
    stride = [s if n > 1 else 0 for s, n in zip(conv.stride(), conv.shape)]
    return min(stride) >= 0 and (stride[1] == 1 or stride[3] == 1 or conv.shape[3] == 1)


def fields_from_conv(conv, n_fields, kind, quad=1, hflip=None, out=None, out_field0=0):
    """conv (B, n_fields * per_field * 4^quad, h, w) -> decoder fields (B, n_fields,
    5 | 9 | 7, H, W) float32 for kind 'cif' | 'caf' | 'cifdet'.

    A float32, float16 or bfloat16 device tensor is read as it is (no float32 copy of a
    half tensor); anything else becomes a float32 device tensor first.  It is also read where
    it is (pp_fields_from_conv_strided): a tensor or view whose columns are adjacent in memory
    (NCHW and its channel, batch and spatial slices) or whose channels are (channels-last
    and its slices) is not copied.  Only a view that is neither, such as one with a step
    along both the channels and the columns, is copied once with .contiguous().

    `hflip` (an HFlip: cif_hflip / caf_hflip, or HFlip() for a CifDet head) undoes the
    horizontal flip of a head computed from a mirrored image in the same pass.  With `out` (a contiguous float32
    device tensor (B, out_fields, n_out, H, W)) the fields go to out[:, out_field0:
    out_field0 + n_fields], the rest of it is left alone and `out` is returned."""
    layout, n_out = LAYOUTS[kind]
    if not (_device.is_device(conv) and conv.dtype in _DTYPES):
        conv = _device.to_device(conv)
    b, ch, h, w = conv.shape
    if not _in_place(conv):
        conv = conv.contiguous()
    if ch != n_fields * n_out * 4 ** quad:
        raise ValueError('{} conv expects {} channels, got {}'.format(
            kind, n_fields * n_out * 4 ** quad, ch))
    shape = (b, n_out, fields_dim(h, quad), fields_dim(w, quad))
    if out is None:
        if out_field0:
            raise ValueError('out_field0 needs out')
        out = torch.empty((b, n_fields) + shape[1:], dtype=torch.float32, device=conv.device)
    elif (not _device.is_device(out) or out.dtype != torch.float32 or not out.is_contiguous()
          or out.dim() != 5 or (out.shape[0],) + tuple(out.shape[2:]) != shape
          or out.device != conv.device):
        raise ValueError('out must be a contiguous float32 device tensor (B, out_fields, '
                         '{}, H, W) for this conv'.format(n_out))
    src_field, swap_ends = hflip.tables(n_fields) if hflip is not None else (None, None)
    call('pp_fields_from_conv_strided', _device.ptr(conv), _DTYPES[conv.dtype],
         (ctypes.c_int64 * 4)(*conv.stride()), b, n_fields, layout, h, w, quad,
         int(hflip is not None), src_field, swap_ends, _device.ptr(out), out.shape[1],
         int(out_field0), _device.stream())
    return out


class RaggedIngest:
    """One head's conv outputs of n images of different sizes and the container of a ragged
    batch they are ingested into (pp_fields_from_conv_ragged, or for channels-last inputs
    pp_fields_from_conv_ragged_interleaved: `interleaved`): the pinned host tables, the
    device tables and the output, built once; launch() enqueues the pass on the current
    stream, again after the conv tensors were rewritten in place.  The arguments are
    fields_from_conv_ragged's; `out_fields` widens a container allocated here.

    out           the container (n, out_fields, 5 | 9 | 7, H, W)
    extents       device (n, 2) int32 field sizes (H_i, W_i), written by the launch
    extents_host  the same table, NumPy"""

    def __init__(self, convs, n_fields, kind, quad=1, hflip=None, conv_extents=None,
                 shape=None, out=None, out_field0=0, out_fields=None):
        layout, n_out = LAYOUTS[kind]
        channels = n_fields * n_out * 4 ** quad
        if isinstance(convs, torch.Tensor):
            ptrs, strides, ext, keep, interleaved = self._batched(convs, conv_extents)
        else:
            if conv_extents is not None:
                raise ValueError('conv_extents goes with one batched tensor; the tensors of a '
                                 'list have their own sizes')
            ptrs, strides, ext, keep, interleaved = self._listed(list(convs))
        first = keep[0]
        if first.shape[-3] != channels:
            raise ValueError('{} conv expects {} channels, got {}'.format(
                kind, channels, first.shape[-3]))
        self._convs = keep  # the tables point into them
        self.interleaved = interleaved
        self.n = n = len(ext)
        self.extents_host = ext.astype(np.int32)
        for _ in range(quad):  # pp_fields_dim
            self.extents_host = 2 * self.extents_host - 1
        largest = tuple(int(v) for v in self.extents_host.max(axis=0))
        if out is not None and shape is None:
            shape = tuple(out.shape[3:])
        self.h, self.w = (int(v) for v in shape) if shape is not None else largest
        if self.h < largest[0] or self.w < largest[1]:
            raise ValueError('a container of {} x {} does not hold fields of {} x {}'.format(
                self.h, self.w, *largest))
        if out is None:
            if out_field0 and out_fields is None:
                raise ValueError('out_field0 needs out')
            out = torch.empty((n, out_fields or n_fields, n_out, self.h, self.w),
                              dtype=torch.float32, device=first.device)
        elif (not _device.is_device(out) or out.dtype != torch.float32 or not out.is_contiguous()
              or out.dim() != 5 or out.device != first.device
              or (out.shape[0],) + tuple(out.shape[2:]) != (n, n_out, self.h, self.w)):
            raise ValueError('out must be a contiguous float32 device tensor (n, out_fields, '
                             '{}, H, W) for these convs'.format(n_out))
        if out_field0 < 0 or out_field0 + n_fields > out.shape[1]:
            raise ValueError('fields {}..{} do not fit in the {} of out'.format(
                out_field0, out_field0 + n_fields - 1, out.shape[1]))
        self.out, self.out_field0 = out, int(out_field0)
        self._src_field, self._swap_ends = (hflip.tables(n_fields) if hflip is not None
                                            else (None, None))
        self._args = (_DTYPES[first.dtype], n_fields, layout, quad, int(hflip is not None))
        # one pinned host block: pointers, strides, conv extents (8-byte entries first)
        lib = load()
        self._host = torch.empty(32 * n, dtype=torch.uint8, pin_memory=True)
        host = self._host.numpy()
        host[:8 * n].view(np.uint64)[:] = ptrs
        host[8 * n:24 * n].view(np.int64)[:] = strides.reshape(-1)
        host[24 * n:].view(np.int32)[:] = ext.reshape(-1)
        size, ext_off = lib.pp_ragged_conv_tables_size(n), lib.pp_ragged_conv_extents_offset(n)
        self._tables = torch.empty(size, dtype=torch.uint8, device=first.device)
        self.extents = self._tables[ext_off:].view(torch.int32).view(n, 2)

    @staticmethod
    def _check(t):
        if not (_device.is_device(t) and t.dtype in _DTYPES):
            raise ValueError('ragged conv outputs must be float32, float16 or bfloat16 device '
                             'tensors')

    @staticmethod
    def _readable(shape, stride):
        """(planar, interleaved): whether a (ch, h, w) view is read where it lies by its column
        stride 1 (pp_fields_from_conv_ragged) and by its channel stride 1
        (pp_fields_from_conv_ragged_interleaved).  The stride of an extent of 1 says nothing."""
        return shape[2] == 1 or stride[2] == 1, shape[0] == 1 or stride[0] == 1

    @classmethod
    def _listed(cls, convs):
        """Per-image tensors (ch, h_i, w_i) or (1, ch, h_i, w_i), classified once.  The call
        is interleaved when some image is read by its channel stride alone (channels-last and
        its slices) and none by its column stride alone; any other list is planar, as it was
        before the interleaved symbol.  A view the call's class does not read is copied into
        it, that image only."""
        if not convs:
            raise ValueError('a ragged batch needs at least one image')
        keep = []
        for t in convs:
            cls._check(t)
            if t.dim() == 4 and t.shape[0] == 1:
                t = t[0]
            if t.dim() != 3:
                raise ValueError('expected per-image conv outputs (ch, h, w) or (1, ch, h, w), '
                                 'got {}'.format(tuple(t.shape)))
            keep.append(t)
        if any(t.dtype != keep[0].dtype or t.device != keep[0].device or
               t.shape[0] != keep[0].shape[0] for t in keep):
            raise ValueError('the conv outputs of a ragged batch differ in type, device or '
                             'channels')
        kinds = [cls._readable(t.shape, t.stride()) for t in keep]
        interleaved = (any(i and not p for p, i in kinds) and
                       not any(p and not i for p, i in kinds))
        if interleaved:
            keep = [t if i else t.permute(1, 2, 0).contiguous().permute(2, 0, 1)
                    for t, (_, i) in zip(keep, kinds)]
            strides = np.array([t.stride()[1:] for t in keep], np.int64)
        else:
            keep = [t if p else t.contiguous() for t, (p, _) in zip(keep, kinds)]
            strides = np.array([t.stride()[:2] for t in keep], np.int64)
        ptrs = np.array([t.data_ptr() for t in keep], np.uint64)
        ext = np.array([t.shape[1:] for t in keep], np.int64)
        return ptrs, strides, ext, keep, interleaved

    @classmethod
    def _batched(cls, conv, conv_extents):
        """One (n, ch, hmax, wmax) tensor whose image i is valid in [0, h_i) x [0, w_i):
        pointers are base + i * image stride (no per-image data_ptr()).  A channels-last
        tensor, or a channel slice of one, is the interleaved call; a view that is neither
        planar nor interleaved is copied once."""
        cls._check(conv)
        if conv.dim() != 4 or conv.shape[0] == 0:
            raise ValueError('expected a batched conv output (n, ch, hmax, wmax), n > 0')
        n = conv.shape[0]
        if conv_extents is None:
            ext = np.tile(np.array(conv.shape[2:], np.int64), (n, 1))
        else:
            ext = np.asarray(conv_extents, dtype=np.int64)
        if ext.shape != (n, 2) or (ext <= 0).any() or (ext > np.array(conv.shape[2:])).any():
            raise ValueError('conv_extents must be (n, 2) rows (h_i, w_i) inside the batched '
                             'tensor, 0 < h_i <= {}, 0 < w_i <= {}'.format(*conv.shape[2:]))
        planar, interleaved = cls._readable(conv.shape[1:], conv.stride()[1:])
        interleaved = interleaved and not planar
        if not (planar or interleaved):
            conv = conv.contiguous()
        ptrs = (np.uint64(conv.data_ptr()) + np.arange(n, dtype=np.uint64) *
                np.uint64(conv.stride(0) * conv.element_size()))
        strides = np.tile(np.array(conv.stride()[2:] if interleaved else conv.stride()[1:3],
                                   np.int64), (n, 1))
        return ptrs, strides, ext, [conv], interleaved

    def launch(self):
        self.enqueue()
        _hold(self)
        return self

    def enqueue(self):
        """The library call alone; the caller keeps this object until the stream is past it."""
        n, size = self.n, self._tables.numel()
        dtype, n_fields, layout, quad, mirror = self._args
        host = self._host.data_ptr()
        call('pp_fields_from_conv_ragged_interleaved' if self.interleaved else
             'pp_fields_from_conv_ragged', ctypes.c_void_p(host), dtype,
             ctypes.c_void_p(host + 24 * n), ctypes.c_void_p(host + 8 * n), n, n_fields, layout,
             quad, mirror, self._src_field, self._swap_ends, self.h, self.w,
             _device.ptr(self.out), self.out.shape[1], self.out_field0,
             _device.ptr(self._tables), ctypes.c_size_t(size), _device.stream())


# launches whose pinned host tables and conv tensors the stream may not have read yet: they
# stay referenced until an event recorded behind the launch has passed, whatever the caller
# keeps of the results
_PENDING = []


def _hold(ingest):
    _PENDING[:] = [(e, i) for e, i in _PENDING if not e.query()]
    event = torch.cuda.Event()
    event.record()
    _PENDING.append((event, ingest))


def fields_from_conv_ragged(convs, n_fields, kind, quad=1, hflip=None, conv_extents=None,
                            shape=None, out=None, out_field0=0):
    """Conv outputs of n images of different sizes -> the container of a ragged batch
    (engine.RaggedFields, CifCaf.decode_ragged) in one HIP pass per head
    (pp_fields_from_conv_ragged): no per-image fields and no pack.

    `convs` is a list of per-image device tensors (ch, h_i, w_i) or (1, ch, h_i, w_i), or one
    (n, ch, hmax, wmax) tensor with `conv_extents` (n, 2), the valid (h_i, w_i) of each image
    (a padded batch, or a channel slice of a fused one).  float32, float16 and bfloat16 are
    read as they lie: views whose columns are adjacent (NCHW and its slices) by their channel
    and row strides, views whose channels are adjacent (channels-last and its channel and
    spatial slices, e.g. contiguous(memory_format=channels_last)[0] or a permuted NHWC tensor)
    by their row and column strides (pp_fields_from_conv_ragged_interleaved).  One call reads
    one class: a list with images that only the first reads and images that only the second
    reads is planar, and its channels-last images are copied, each once; a view that is
    neither (a step along both channels and columns) is copied once into the call's class.
    `hflip` as in fields_from_conv; the mirror is about each image's own width.  `shape`
    (H, W) sets a container larger than the largest field size, which is the default.  With
    `out` (n, out_fields, 5 | 9 | 7, H, W) the fields go to out[:, out_field0:out_field0 +
    n_fields], written in full (zero outside each image's extent), the rest is left alone.

    Returns (container, device (n, 2) int32 table of the field sizes (H_i, W_i), the same
    table on the host)."""
    ing = RaggedIngest(convs, n_fields, kind, quad, hflip, conv_extents, shape, out,
                       out_field0).launch()
    return ing.out, ing.extents, ing.extents_host


def _planar_views(convs, conv_extents):
    """The conv outputs of one head as pp_fields_from_conv_ragged_heads reads them: pointers
    (n) uint64, channel and row strides (n, 2) int64, conv extents (n, 2) int64, the channel
    counts (n), the type, the device and the tensors the pointers lead into.  `convs` and
    `conv_extents` are fields_from_conv_ragged's.  Everything is collected in one pass over
    the tensors and checked afterwards as arrays.  A view whose columns are not adjacent
    (channels-last, or a step along the columns) is copied once into NCHW, that tensor only."""
    if isinstance(convs, torch.Tensor):
        RaggedIngest._check(convs)
        if convs.dim() != 4 or convs.shape[0] == 0:
            raise ValueError('expected a batched conv output (n, ch, hmax, wmax), n > 0')
        if convs.shape[3] > 1 and convs.stride(3) != 1:
            convs = convs.contiguous()
        n = convs.shape[0]
        ext = (np.tile(np.array(convs.shape[2:], np.int64), (n, 1)) if conv_extents is None
               else np.asarray(conv_extents, dtype=np.int64))
        if ext.shape != (n, 2) or (ext <= 0).any() or (ext > np.array(convs.shape[2:])).any():
            raise ValueError('conv_extents must be (n, 2) rows (h_i, w_i) inside the batched '
                             'tensor, 0 < h_i <= {}, 0 < w_i <= {}'.format(*convs.shape[2:]))
        ptrs = (np.uint64(convs.data_ptr()) + np.arange(n, dtype=np.uint64) *
                np.uint64(convs.stride(0) * convs.element_size()))
        strides = np.tile(np.array(convs.stride()[1:3], np.int64), (n, 1))
        channels = np.full(n, convs.shape[1], np.int64)
        return ptrs, strides, ext, channels, convs.dtype, convs.device, [convs]
    if conv_extents is not None:
        raise ValueError('conv_extents goes with one batched tensor; the tensors of a list have '
                         'their own sizes')
    convs = list(convs)
    if not convs:
        raise ValueError('a ragged batch needs at least one image')
    shapes, strides, ptrs, keep, kinds = [], [], [], [], set()
    tensor = torch.Tensor
    for t in convs:
        if not (isinstance(t, tensor) and t.is_cuda):
            raise ValueError('ragged conv outputs must be float32, float16 or bfloat16 device '
                             'tensors')
        sh, st = t.shape, t.stride()
        if len(sh) == 4 and sh[0] == 1:
            sh, st = sh[1:], st[1:]
        if len(sh) != 3:
            raise ValueError('expected per-image conv outputs (ch, h, w) or (1, ch, h, w), '
                             'got {}'.format(tuple(t.shape)))
        if sh[2] > 1 and st[2] != 1:
            t = t.contiguous()
            st = t.stride()[-3:]
        shapes.append(sh)
        strides.append(st[:2])
        ptrs.append(t.data_ptr())
        kinds.add((t.dtype, t.device))
        keep.append(t)
    if len(kinds) != 1 or keep[0].dtype not in _DTYPES:
        raise ValueError('the conv outputs of a ragged batch must be of one type (float32, '
                         'float16 or bfloat16) and on one device')
    shapes = np.array(shapes, np.int64)
    return (np.array(ptrs, np.uint64), np.array(strides, np.int64), shapes[:, 1:], shapes[:, 0],
            keep[0].dtype, keep[0].device, keep)


class RaggedHeadsIngest:
    """The conv outputs of several heads of n images of different sizes and the containers of
    a ragged head set they are ingested into in one launch (pp_fields_from_conv_ragged_heads):
    one pinned host block, the device tables and the containers, built once; launch()
    enqueues the pass on the current stream, again after the conv tensors were rewritten in
    place.

    `parts` is a list of (convs, n_fields, kind, hflip, group): `convs` and `conv_extents` as
    fields_from_conv_ragged takes them, `n_fields` (None: what the channels say), `kind` 'cif'
    or 'caf', `hflip` an HFlip or None, `group` the container the part writes.  The groups are
    numbered from 0 in the order of their first part; the parts of one group are of one kind,
    have the same conv sizes and lie side by side in its container, in their order.
    `outs` maps a group to a container of the caller's, a contiguous float32 device tensor
    (n, out_fields, 5 | 9, H, W) that holds every field size of the group, and `field0` a
    group to the first field its parts write (0): the fields of the container outside the
    group's range are left alone.

    outs          per group the container (n, fields of the group, 5 | 9, H_g, W_g), (H_g, W_g)
                  the group's largest field size
    extents       device (n_groups, n, 2) int32 field sizes, written by the launch
    extents_host  the same table, NumPy"""

    def __init__(self, parts, quad=1, conv_extents=None, outs=None, field0=None):
        from ._abi import CONV_HEAD_DTYPE  # pylint: disable=import-outside-toplevel
        lib = load()
        parts = list(parts)
        views = [_planar_views(p[0], conv_extents) for p in parts]
        counts = sorted({len(v[0]) for v in views})
        if len(counts) != 1:
            raise ValueError('the heads of a ragged batch have different numbers of images: ' +
                             ', '.join(str(c) for c in counts))
        self.n = n = counts[0]
        n_entries = len(parts)
        if len({(v[4], v[5]) for v in views}) != 1:
            raise ValueError('the conv outputs of a ragged batch differ in type or device')
        dtype, dev = views[0][4], views[0][5]
        self._convs = [v[6] for v in views]  # the tables point into them
        ext = np.stack([v[2] for v in views])  # (n_entries, n, 2) conv sizes
        field_ext = ext.astype(np.int32)
        for _ in range(quad):  # pp_fields_dim
            field_ext = 2 * field_ext - 1
        rows, groups = [], {}
        for m, ((_, n_fields, kind, hflip, group), v) in enumerate(zip(parts, views)):
            layout, n_out = LAYOUTS[kind]
            per_field = n_out * 4 ** quad
            channels = v[3]
            if n_fields is None:
                n_fields = int(channels[0]) // per_field
            if n_fields <= 0 or (channels != n_fields * per_field).any():
                raise ValueError('{} conv of {} fields expects {} channels, got {}: the images '
                                 'of a ragged batch may not differ in K or C'.format(
                                     kind, n_fields, n_fields * per_field,
                                     sorted(set(channels.tolist()))))
            g = groups.setdefault(group, dict(kind=kind, first=m, members=[],
                                              fields=int((field0 or {}).get(group, 0))))
            if g['kind'] != kind:
                raise ValueError('the parts of one container are of one kind')
            if not np.array_equal(ext[g['first']], ext[m]):
                raise ValueError('the parts of one container differ in conv size')
            rows.append((m, layout, n_fields, g['fields'], hflip, g))
            g['fields'] += n_fields
            g['members'].append(m)
        self.extents_host = np.ascontiguousarray(
            np.stack([field_ext[g['first']] for g in groups.values()]))
        n_rows = len(groups)
        self.outs = []
        for r, g in enumerate(groups.values()):
            h, w = (int(v) for v in self.extents_host[r].max(axis=0))
            n_out = LAYOUTS[g['kind']][1]
            out = (outs or {}).get(list(groups)[r])
            if out is None:
                out = torch.empty((n, g['fields'], n_out, h, w), dtype=torch.float32, device=dev)
            elif (not _device.is_device(out) or out.dtype != torch.float32 or out.dim() != 5
                  or not out.is_contiguous() or out.device != dev
                  or tuple(out.shape[::2]) != (n, n_out, out.shape[4]) or g['fields'] < 0
                  or out.shape[1] < g['fields'] or out.shape[3] < h or out.shape[4] < w):
                raise ValueError('out must be a contiguous float32 device tensor (n, out_fields, '
                                 '{}, H, W) that holds fields ..{} of {} x {}'.format(
                                     n_out, g['fields'] - 1, h, w))
            g['row'], g['hw'] = r, tuple(out.shape[3:])
            self.outs.append(out)
        # one pinned host block in the order of the device tables: pointers, strides, entries,
        # conv extents; the field extents the kernel writes follow on the device
        size = lib.pp_ragged_conv_heads_tables_size(n, n_entries)
        ext_off = lib.pp_ragged_conv_heads_extents_offset(n, n_entries)
        cells = n_entries * n
        off = (0, 8 * cells, 24 * cells, 24 * cells + CONV_HEAD_DTYPE.itemsize * n_entries)
        if size == 0 or off[3] + 8 * cells != ext_off:
            raise ValueError('{} conv heads of {} images: outside what '
                             'pp_fields_from_conv_ragged_heads takes'.format(n_entries, n))
        self._host = torch.empty(ext_off, dtype=torch.uint8, pin_memory=True)
        host = self._host.numpy()
        host[:off[1]].view(np.uint64)[:] = np.concatenate([v[0] for v in views])
        host[off[1]:off[2]].view(np.int64)[:] = np.concatenate([v[1] for v in views]).reshape(-1)
        host[off[3]:].view(np.int32)[:] = ext.reshape(-1)
        heads = host[off[2]:off[3]].view(CONV_HEAD_DTYPE)
        heads[:] = np.zeros((), CONV_HEAD_DTYPE)
        base = self._host.data_ptr()
        for m, layout, n_fields, field0, hflip, g in rows:
            out = self.outs[g['row']]
            heads[m]['d_container'] = out.data_ptr()
            heads[m]['layout'], heads[m]['n_fields'] = layout, n_fields
            heads[m]['H'], heads[m]['W'] = g['hw']
            heads[m]['out_fields'], heads[m]['out_field0'] = out.shape[1], field0
            heads[m]['ext_row'] = g['row'] if m == g['first'] else -1
            if hflip is not None:
                src_field, swap_ends = hflip.tables(n_fields)
                call('pp_conv_head_set_flip',
                     ctypes.c_void_p(base + off[2] + CONV_HEAD_DTYPE.itemsize * m), 1, src_field,
                     swap_ends)
        self._off = off
        self._args = (n_entries, n_rows, _DTYPES[dtype], quad)
        self._tables = torch.empty(size, dtype=torch.uint8, device=dev)
        self.extents = self._tables[ext_off:ext_off + 8 * n_rows * n].view(torch.int32).view(
            n_rows, n, 2)

    def launch(self):
        self.enqueue()
        _hold(self)
        return self

    def enqueue(self):
        """The library call alone; the caller keeps this object until the stream is past it."""
        n_entries, n_rows, dtype, quad = self._args
        base, off = self._host.data_ptr(), self._off
        call('pp_fields_from_conv_ragged_heads', ctypes.c_void_p(base + off[2]), n_entries,
             n_rows, ctypes.c_void_p(base), ctypes.c_void_p(base + off[3]),
             ctypes.c_void_p(base + off[1]), self.n, dtype, quad, _device.ptr(self._tables),
             ctypes.c_size_t(self._tables.numel()), _device.stream())


class RaggedMultiScaleCollector(torch.nn.Module):
    """MultiScaleCollector for images of different sizes: forward(convs, conv_extents=None) ->
    engine.RaggedHeadSet, every head of every image ingested in one launch
    (engine.RaggedHeadSet.from_conv).  The constructor takes MultiScaleCollector's arguments
    and the `field_config` that names the heads.  `convs` holds per scale `cif, caf[, dense
    caf]`, the unflipped scales first, then the mirrored ones, which are un-flipped in the same
    pass; each is a list of per-image tensors or one batched tensor with `conv_extents`
    (fields_from_conv_ragged).  With a `dense_skeleton` the dense CAF is written behind the CAF
    into one container (the `concat_dense` layout, the only one a FieldConfig with one CAF
    index per scale names), so the head list has `cif, caf` per scale."""

    def __init__(self, keypoints, skeleton, field_config, dense_skeleton=None, quad=1,
                 n_scales=5, include_hflip=True, concat_dense=False):
        super().__init__()
        if concat_dense and dense_skeleton is None:
            raise ValueError('concat_dense needs a dense_skeleton')
        self.field_config = field_config
        self.n_cif, self.n_caf = len(keypoints), len(skeleton)
        self.n_dense = 0 if dense_skeleton is None else len(dense_skeleton)
        self.quad, self.n_scales, self.include_hflip = quad, n_scales, include_hflip
        self.cif_flip = cif_hflip(keypoints)
        self.caf_flip = caf_hflip(keypoints, skeleton)
        self.dense_flip = caf_hflip(keypoints, dense_skeleton) if self.n_dense else None

    def forward(self, *args, conv_extents=None):  # pylint: disable=arguments-differ
        from .engine import RaggedHeadSet  # pylint: disable=import-outside-toplevel
        convs = args[0]
        per = 3 if self.n_dense else 2
        n = self.n_scales * (2 if self.include_hflip else 1)
        if len(convs) != per * n:
            raise ValueError('expected {} conv outputs ({} per scale), got {}'.format(
                per * n, per, len(convs)))
        entries = []
        for s in range(n):
            flipped = s >= self.n_scales
            entries.append((convs[per * s], self.cif_flip if flipped else None))
            caf = [(convs[per * s + 1], self.n_caf, self.caf_flip if flipped else None)]
            if self.n_dense:
                caf.append((convs[per * s + 2], self.n_dense,
                            self.dense_flip if flipped else None))
            entries.append(caf)
        return RaggedHeadSet.from_conv(entries, self.field_config, self.quad,
                                       conv_extents=conv_extents)


class RaggedCollector(torch.nn.Module):
    """CifCafCollector for images of different sizes: forward((cif_convs, caf_convs),
    conv_extents=None) -> engine.RaggedFields, each head ingested straight into its
    container (the arguments are RaggedFields.from_conv's)."""

    def __init__(self, n_cif, n_caf, quad=1):
        super().__init__()
        self.n_cif, self.n_caf, self.quad = n_cif, n_caf, quad

    def forward(self, *args, conv_extents=None):  # pylint: disable=arguments-differ
        from .engine import RaggedFields  # pylint: disable=import-outside-toplevel
        cif_convs, caf_convs = args[0]
        return RaggedFields.from_conv(cif_convs, caf_convs, self.n_cif, self.n_caf, self.quad,
                                      conv_extents=conv_extents)


class RaggedDetCollector(torch.nn.Module):
    """CifdetCollector for images of different sizes: forward((det_convs,),
    conv_extents=None) -> engine.RaggedDetFields, the head ingested straight into its
    container (the arguments are RaggedDetFields.from_conv's)."""

    def __init__(self, n_categories, quad=1):
        super().__init__()
        self.n_categories, self.quad = n_categories, quad

    def forward(self, *args, conv_extents=None):  # pylint: disable=arguments-differ
        from .engine import RaggedDetFields  # pylint: disable=import-outside-toplevel
        return RaggedDetFields.from_conv(args[0][0], self.n_categories, self.quad,
                                         conv_extents=conv_extents)


class CifCafCollector(torch.nn.Module):
    """heads.CifCafCollector for heads that stop at their conv: forward((cif_conv,
    caf_conv)) -> (cif, caf) in the decoder layout, on the device."""

    def __init__(self, n_cif, n_caf, quad=1):
        super().__init__()
        self.n_cif, self.n_caf, self.quad = n_cif, n_caf, quad

    def forward(self, *args):  # pylint: disable=arguments-differ
        cif_conv, caf_conv = args[0]
        return (fields_from_conv(cif_conv, self.n_cif, 'cif', self.quad),
                fields_from_conv(caf_conv, self.n_caf, 'caf', self.quad))


class CifdetCollector(torch.nn.Module):
    """heads.CifdetCollector for a detection head that stops at its conv."""

    def __init__(self, n_categories, quad=1):
        super().__init__()
        self.n_categories, self.quad = n_categories, quad

    def forward(self, *args):  # pylint: disable=arguments-differ
        return (fields_from_conv(args[0][0], self.n_categories, 'cifdet', self.quad),)


class MultiScaleCollector(torch.nn.Module):
    """The head list of a ShellMultiScale-style model (nets.py:111-143) whose heads stop at
    their conv: forward(conv outputs) -> decoder fields, in the same order.

    Input: per scale `cif, caf` (and the dense caf with `dense_skeleton`), the `n_scales`
    unflipped scales first, then, with `include_hflip`, the scales of the mirrored image,
    whose fields are un-flipped in the ingest pass.  Output: per scale `cif, caf[, dense
    caf]` (the v*3 indices of factory_decode(multi_scale=True)); with `concat_dense`, caf
    and dense caf share one (B, C + Cd, 9, H, W) tensor and the list has `cif, caf` per scale
    (the v*2 indices of dense_connections=True).  CifCaf.decode_heads takes the list."""

    def __init__(self, keypoints, skeleton, dense_skeleton=None, quad=1, n_scales=5,
                 include_hflip=True, concat_dense=False):
        super().__init__()
        if concat_dense and dense_skeleton is None:
            raise ValueError('concat_dense needs a dense_skeleton')
        self.n_cif, self.n_caf = len(keypoints), len(skeleton)
        self.n_dense = 0 if dense_skeleton is None else len(dense_skeleton)
        self.quad, self.n_scales = quad, n_scales
        self.include_hflip, self.concat_dense = include_hflip, concat_dense
        self.cif_flip = cif_hflip(keypoints)
        self.caf_flip = caf_hflip(keypoints, skeleton)
        self.dense_flip = caf_hflip(keypoints, dense_skeleton) if self.n_dense else None

    def forward(self, *args):  # pylint: disable=arguments-differ
        convs = args[0]
        per = 3 if self.n_dense else 2
        n = self.n_scales * (2 if self.include_hflip else 1)
        if len(convs) != per * n:
            raise ValueError('expected {} conv outputs ({} per scale), got {}'.format(
                per * n, per, len(convs)))
        out = []
        for s in range(n):
            flipped = s >= self.n_scales
            cif, caf = convs[per * s], convs[per * s + 1]
            out.append(fields_from_conv(cif, self.n_cif, 'cif', self.quad,
                                        hflip=self.cif_flip if flipped else None))
            caf_flip = self.caf_flip if flipped else None
            if not self.n_dense:
                out.append(fields_from_conv(caf, self.n_caf, 'caf', self.quad, hflip=caf_flip))
                continue
            dense = convs[per * s + 2]
            dense_flip = self.dense_flip if flipped else None
            if not self.concat_dense:
                out.append(fields_from_conv(caf, self.n_caf, 'caf', self.quad, hflip=caf_flip))
                out.append(fields_from_conv(dense, self.n_dense, 'caf', self.quad,
                                            hflip=dense_flip))
                continue
            both = torch.empty(
                (caf.shape[0], self.n_caf + self.n_dense, 9,
                 fields_dim(caf.shape[2], self.quad), fields_dim(caf.shape[3], self.quad)),
                dtype=torch.float32, device=_device.require())
            fields_from_conv(caf, self.n_caf, 'caf', self.quad, hflip=caf_flip, out=both)
            fields_from_conv(dense, self.n_dense, 'caf', self.quad, hflip=dense_flip, out=both,
                             out_field0=self.n_caf)
            out.append(both)
        return out
