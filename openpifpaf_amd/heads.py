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
"""
import ctypes

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
