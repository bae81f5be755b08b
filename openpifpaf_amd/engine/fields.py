"""The decoders' inputs on the device: initial annotations, the heads of a multi-scale
FieldConfig, and the containers of ragged batches (images of different field sizes)."""
import ctypes

import numpy as np
import torch

from .. import _device
from .._abi import ANN_DTYPE, scale_list
from .._lib import call, load


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
        self.n, self.k, self.c = (*self.cifs[0].shape[:2], self.cafs[0].shape[1])
        if any(t.shape[0] != self.n for t in self.cifs + self.cafs):
            raise ValueError('heads have different batch sizes')
        if any(t.shape[1] != self.k for t in self.cifs) or any(t.shape[1] != self.c for t in self.cafs):
            raise ValueError('heads have different field counts')
        self.h, self.w = self.cifs[0].shape[3], self.cifs[0].shape[4]
        self.arr, self.pairs, self.stride0, self.shape_key = head_scales(
            self.cifs, self.cafs, fc, ragged=False)


def head_scales(cifs, cafs, fc, ragged):
    """(pp_scale array, pairs, stride of the first CIF head, shape key) of the batched CIF and
    CAF head tensors (or containers) of FieldConfig `fc`.  The shape key names the shapes for
    the engine's buffer cache; a ragged batch's starts with 'ragged'."""
    arr = scale_list([(t.data_ptr(), t.shape[3], t.shape[4]) for t in cifs],
                     [(t.data_ptr(), t.shape[3], t.shape[4]) for t in cafs],
                     fc.cif_strides, fc.caf_strides, fc.cif_min_scales,
                     fc.caf_min_distances, fc.caf_max_distances)
    pairs = int(len(fc.cif_indices) == 10)  # cif_hr.py:63
    key = (('ragged', pairs) if ragged else (pairs,)) + tuple(
        (s.H, s.W, s.stride, s.role) for s in arr)
    return arr, pairs, int(fc.cif_strides[0]), key


class _RaggedContainers:
    """What RaggedFields and RaggedDetFields share: per field kind of KINDS, (attribute of the
    container, attribute of its plane count, channels), a container, pinned host tables
    (pointers, then extents) and their device copy, and the pack launches over them."""

    KINDS = ()
    _ingests = ()  # from_conv: the heads.RaggedIngest of each head (or part), CIF first

    def _build(self, images, pointers):
        """From the images' tensors of the first kind: n, the extents, the containers at
        (n, planes, channels, H, W) and the tables, pointers[kind] the images' data_ptr of
        that kind; then the pack."""
        lib, dev = load(), images[0].device
        self.n = n = len(images)
        self.extents_host = np.array([f.shape[2:] for f in images], np.int32).reshape(n, 2)
        self.h, self.w = (int(v) for v in self.extents_host.max(axis=0))
        for attr, planes, ch in self.KINDS:
            setattr(self, attr, torch.empty((n, getattr(self, planes), ch, self.h, self.w),
                                            dtype=torch.float32, device=dev))
        # pinned host tables (pointers, then extents, per field kind): the copies are
        # asynchronous, so the tables live as long as this object
        size, ext_off = lib.pp_ragged_tables_size(n), lib.pp_ragged_extents_offset(n)
        self._host = torch.empty((len(self.KINDS), size), dtype=torch.uint8, pin_memory=True)
        self._tables = torch.empty((len(self.KINDS), size), dtype=torch.uint8, device=dev)
        for kind, ptrs in enumerate(pointers):
            host = self._host[kind].numpy()
            host[:ext_off].view(np.uint64)[:] = ptrs
            host[ext_off:].view(np.int32)[:] = self.extents_host.reshape(-1)
        self.extents = self._tables[0][ext_off:].view(torch.int32).view(n, 2)
        self.pack()

    def pack(self):
        """The pack launches (one per field kind, CIF first) on the current stream, from the
        tables built at construction: again after the images' tensors were rewritten in
        place.  After from_conv: the ingest launches."""
        for ingest in self._ingests:
            ingest.launch()
        if self._ingests:
            return
        size, ext_off = self._host.shape[1], load().pp_ragged_extents_offset(self.n)
        for kind, (attr, planes, ch) in enumerate(self.KINDS):
            call('pp_fields_pack_ragged', ctypes.c_void_p(self._host[kind].data_ptr()),
                 ctypes.c_void_p(self._host[kind].data_ptr() + ext_off), self.n,
                 getattr(self, planes), ch, self.h, self.w, _device.ptr(getattr(self, attr)),
                 _device.ptr(self._tables[kind]), ctypes.c_size_t(size), _device.stream())


class RaggedFields(_RaggedContainers):
    """A batch of images of different field sizes (pp_fields_pack_ragged): `fields` is a list
    of per-image (cif, caf) device tensors, float32 and contiguous, (K, 5, h_i, w_i) and
    (C, 9, h_i, w_i) with K and C the same for every image.  Packs them on the current stream
    into the containers `cif` (n, K, 5, H, W) and `caf` (n, C, 9, H, W), (H, W) the largest
    size, zero outside each image's extent, and owns them with the extent table (`extents`,
    device (n, 2) int32; `extents_host` the same on the host).  The images' tensors may be
    freed once the pack has run.  A list of equal shapes takes the same route.
    RaggedFields.from_conv builds the same object from the heads' conv outputs, without
    per-image fields and without the pack."""

    KINDS = (('cif', 'k', 5), ('caf', 'c', 9))

    def __init__(self, fields):
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
        self.k, self.c = fields[0][0].shape[0], fields[0][1].shape[0]
        if any(f[0].shape[0] != self.k or f[1].shape[0] != self.c for f in fields):
            raise ValueError('the images of a ragged batch differ in K or C: ' + ', '.join(
                sorted({'K={} C={}'.format(f[0].shape[0], f[1].shape[0]) for f in fields})))
        self._build([f[0] for f in fields],
                    [[f[kind].data_ptr() for f in fields] for kind in range(2)])

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
        from ..heads import RaggedIngest  # pylint: disable=import-outside-toplevel
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


class RaggedDetFields(_RaggedContainers):
    """RaggedFields for the detection decoder (pp_cifdet_decode_ragged): `fields` is a list of
    per-image CifDet device tensors, float32 and contiguous, (K, 7, h_i, w_i) with K the same
    for every image.  Packs them on the current stream into the container `det`
    (n, K, 7, H, W), (H, W) the largest size, zero outside each image's extent, and owns it
    with the extent table (`extents`, device (n, 2) int32; `extents_host` the same on the
    host).  The images' tensors may be freed once the pack has run.  A list of equal shapes
    takes the same route.  RaggedDetFields.from_conv builds the same object from the head's
    conv outputs, without per-image fields and without the pack."""

    KINDS = (('det', 'k', 7),)

    def __init__(self, fields):
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
        self.k = fields[0].shape[0]
        if any(f.shape[0] != self.k for f in fields):
            raise ValueError('the images of a ragged batch differ in K: ' + ', '.join(
                sorted({'K={}'.format(f.shape[0]) for f in fields})))
        self._build(fields, [[f.data_ptr() for f in fields]])

    @classmethod
    def from_conv(cls, convs, n_categories, quad=1, conv_extents=None, hflip=None):
        """The same object from the detection head's conv outputs, one HIP pass straight into
        the container (heads.fields_from_conv_ragged has the forms `convs` and `conv_extents`
        take; `hflip`: heads.HFlip() for a mirrored pass): no per-image fields and no pack.
        pack() runs the ingest launch again."""
        from ..heads import RaggedIngest  # pylint: disable=import-outside-toplevel
        ingest = RaggedIngest(convs, n_categories, 'cifdet', quad, hflip, conv_extents)
        self = cls.__new__(cls)
        self.n, self.k, self.h, self.w = ingest.n, n_categories, ingest.h, ingest.w
        self.det = ingest.out
        self.extents, self.extents_host = ingest.extents, ingest.extents_host
        self._ingests = [ingest]
        self.pack()
        return self


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
        self.arr, self.pairs, self.stride0, self.shape_key = head_scales(
            self.cifs, self.cafs, fc, ragged=True)
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
        from ..heads import HFlip  # pylint: disable=import-outside-toplevel
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
        from ..heads import RaggedHeadsIngest, RaggedIngest  # pylint: disable=import-outside-toplevel
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
        self.arr, self.pairs, self.stride0, self.shape_key = head_scales(
            self.cifs, self.cafs, fc, ragged=True)
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
