"""CifDet (decoder/generator/cifdet.py:17-52) on gfx950.

Same constructor and call signature as the reference.  One call runs CifDetHr, CifDetSeeds,
the occupancy loop and nms.Detection on the device for one image (`__call__`) or a whole
batch (`decode_batch`), or for images of different field sizes as one batch
(`decode_ragged`, `coco_ragged`; engine.RaggedDetFields), configured from the CifHr /
CifSeeds / nms.Detection class attributes as the reference's decoder.configure() sets them.
"""
import numpy as np
import torch

from ... import _device
from ..._abi import DET_DTYPE, PP_ST_ANN_OVERFLOW, DetNms, check_seed_mask, make_config
from ..._lib import PPError, call
from ...annotation import AnnotationDet
from ...engine import DetEngine, RaggedDetFields, det_call, det_tail
from .. import nms
from ..cif_hr import CifHr
from ..cif_seeds import CifSeeds
from ..field_config import FieldConfig
from .generator import Generator

def det_nms_config(cls=None):
    cls = cls or nms.Detection
    return DetNms(cls.suppression, cls.suppression_soft, cls.instance_threshold,
                  cls.iou_threshold, cls.iou_threshold_soft, 1)


class CifDet(Generator):
    occupancy_visualizer = None
    supports_sharding = True

    def __init__(self, field_config: FieldConfig, categories, *, worker_pool=None):
        super().__init__(worker_pool)
        self.field_config = field_config
        self.categories = categories
        self._ws = None
        # the persistent buffers and the record hand-over of decode_records and everything above
        self.engine = DetEngine()

    def single_head(self):
        """One detection head without a min scale: pp_cifdet_decode; anything else (several
        heads, min-scale masks) runs pp_cifdet_decode_multi."""
        fc = self.field_config
        return len(fc.cif_indices) == 1 and not fc.cif_min_scales[0]

    def head_fields(self, fields):
        """The FieldConfig's detection heads of a field list, in cif_indices order."""
        return [fields[i] for i in self.field_config.cif_indices]

    def config(self):
        if CifSeeds.threshold is None:
            raise TypeError("'>' not supported between instances of 'float' and 'NoneType' "
                            "(CifSeeds.threshold is not configured)")
        stride = int(self.field_config.cif_strides[0])
        check_seed_mask(self.field_config.seed_mask, len(self.categories))
        return make_config(cif_threshold=CifHr.v_threshold, seed_threshold=CifSeeds.threshold,
                           seed_score_scale=CifSeeds.score_scale, stride=int(stride),
                           cif_neighbors=CifHr.neighbors, seed_mask=self.field_config.seed_mask)

    def nms_config(self):
        return det_nms_config()

    def decode_async(self, det_batch, cap=None):
        """decode_records enqueued on the current stream (one decode, one record pack into
        pinned host memory, no read-back): an engine.PendingDetRecords, whose result() waits
        and gives decode_records' (records, offsets) and whose annotations() gives
        decode_batch's lists.  det_batch stays unchanged until then."""
        return self.engine.decode_async(self, det_batch, cap)

    def decode_records(self, det_batch, cap=None):
        """det_batch (B, K, 7, H, W), or with several heads / min scales the list of the
        FieldConfig's heads (each (B, K, 7, H_m, W_m), cif_indices order) -> (pp_det
        records, per-image offsets).  One decode, one pack and one synchronisation in the
        engine's buffers (engine.DetEngine); the records lie in pinned host memory."""
        return self.decode_async(det_batch, cap).result()

    def coco_batch(self, det_batch, metas, **params):
        """decode_device's input and one meta dict per image (with 'image_id') -> the batch's
        eval_coco.CocoRecords of detections: EvalCoco.from_predictions
        (eval_coco.py:108-158) on the device behind the decode.  `params`: max_per_image."""
        from ...eval_coco import coco_records, metas_device  # pylint: disable=import-outside-toplevel
        out, counts = self.decode_device(det_batch)
        if len(metas) != len(counts):
            raise ValueError('{} metas for {} images'.format(len(metas), len(counts)))
        d_metas, d_ids, _ = metas_device(metas, 0)
        return coco_records(out, counts, d_metas, d_ids, det=True,
                            k=params.pop('n_keypoints', 17), **params)

    def coco_heads(self, heads, metas, **params):
        """coco_batch from the model's head list (each (B, ...))."""
        heads = self.head_fields(heads)
        return self.coco_batch(heads[0] if self.single_head() else heads, metas, **params)

    def device_heads(self, det_batch):
        """decode_records' input as the checked list of the heads' device tensors."""
        heads = [_device.to_device(t) for t in
                 (det_batch if isinstance(det_batch, (list, tuple)) else [det_batch])]
        for det in heads:
            if det.dim() != 5 or det.shape[2] != 7:
                raise ValueError('expected CifDet fields (B, K, 7, H, W)')
        if len(heads) != len(self.field_config.cif_indices):
            raise ValueError('expected {} CifDet heads, got {}'.format(
                len(self.field_config.cif_indices), len(heads)))
        if any(t.shape[:3] != heads[0].shape[:3] for t in heads):
            raise ValueError('CifDet heads differ in batch or field count')
        return heads

    def decode_device(self, det_batch, cap=None):
        """decode_records up to the device records: ((B, cap, record bytes) uint8, (B) int32
        counts), complete (the capacity doubles until no image overflows) and the caller's
        own, not an engine slot.  A RaggedDetFields as `det_batch`: decode_ragged_device."""
        d = det_call(self, det_batch)
        cfg, z = self.config(), det_nms_config()
        cap, bound = cap or d.cap, d.k * d.cells
        while True:
            size = d.size(cfg, cap)
            if self._ws is None or self._ws.numel() < size or self._ws.device != d.device:
                self._ws = torch.empty(size, dtype=torch.uint8, device=d.device)
            out = torch.empty((d.n, cap, DET_DTYPE.itemsize), dtype=torch.uint8, device=d.device)
            counts = torch.empty(d.n, dtype=torch.int32, device=d.device)
            status = torch.empty(d.n, dtype=torch.int32, device=d.device)
            call(d.name, *d.lead, *det_tail(cfg, z, out, cap, counts, status, self._ws))
            st = status.cpu().numpy()
            if not (st & PP_ST_ANN_OVERFLOW).any():
                break
            if cap >= bound:
                raise PPError('CifDet: detection capacity overflow')
            cap = min(bound, 2 * cap)
        return out, counts

    # -- ragged batches: images of different field sizes -----------------------------------
    def _ragged(self, fields_list, kw):
        """RaggedDetFields of a list of per-image head lists (each read through the
        FieldConfig's one detection head), packed on the device."""
        if kw.pop('group', None) is not None:
            raise NotImplementedError('a ragged batch does not take group: its decode is '
                                      'single-GPU (sharded ragged decode is not built)')
        if kw:
            raise TypeError('unexpected arguments: ' + ', '.join(sorted(kw)))
        fc = self.field_config
        if len(fc.cif_indices) != 1:
            raise NotImplementedError('a ragged batch needs a FieldConfig with one detection '
                                      'head, got {}; several heads are not built'.format(
                                          len(fc.cif_indices)))
        if fc.cif_min_scales[0]:
            raise NotImplementedError('a ragged batch needs a FieldConfig without min scales; '
                                      'min-scale masks over ragged extents are not built')
        if isinstance(fields_list, RaggedDetFields):  # packed or ingested already
            return fields_list
        return RaggedDetFields([_device.to_device(f[fc.cif_indices[0]]) for f in fields_list])

    def decode_ragged_device(self, ragged, cap=None):
        """decode_device over a RaggedDetFields (pp_cifdet_decode_ragged), the workspace at the
        container's shape: ((n, cap, record bytes) uint8, (n) int32 counts), complete."""
        return self.decode_device(ragged, cap)

    def decode_ragged_records(self, fields_list, cap=None, **kw):
        """decode_ragged up to the records: (pp_det records of all images, per-image
        offsets); pp_det.image is the image's position in the batch."""
        return self.decode_ragged_async(fields_list, cap, **kw).result()

    def decode_ragged_async(self, fields_list, cap=None, **kw):
        """decode_ragged_records enqueued on the current stream, as decode_async: an
        engine.PendingDetRecords (result(): the records and offsets; annotations():
        decode_ragged's lists)."""
        return self.engine.decode_async(self, self._ragged(fields_list, kw), cap)

    def decode_ragged(self, fields_list, **kw):
        """One entry per image, each image's head outputs [det (K, 7, h_i, w_i), ...] at its
        OWN size -> one list of AnnotationDet per image, each as __call__ gives it for that
        image alone, decoded as one device batch (pp_cifdet_decode_ragged).  An
        engine.RaggedDetFields (e.g. RaggedDetFields.from_conv, heads.RaggedDetCollector) in place of the list is decoded as it is."""
        return self.annotations_from_records(*self.decode_ragged_records(fields_list, **kw))

    def coco_ragged(self, fields_list, metas, **params):
        """coco_batch for images of different field sizes (decode_ragged's `fields_list`)."""
        ragged = self._ragged(fields_list, {k: params.pop(k) for k in ('group',) if k in params})
        if len(metas) != ragged.n:
            raise ValueError('{} metas for {} images'.format(len(metas), ragged.n))
        return self.coco_batch(ragged, metas, **params)

    def annotations_from_records(self, recs, offsets):
        return [[AnnotationDet.from_record(r, self.categories)
                 for r in recs[offsets[i]:offsets[i + 1]]] for i in range(len(offsets) - 1)]

    def decode_batch(self, det_batch, *, group=None, dst=0, local=False):
        """(B, K, 7, H, W) -> one list of AnnotationDet per image.

        With a torch.distributed process `group`, the batch is image-sharded as in
        CifCaf.decode_batch: each rank decodes its contiguous `distributed.shard` of the
        images (`local=True`: det_batch is already this rank's share, possibly None), and
        rank `dst` returns the detections of all images in rank order, gathered as pp_det
        records whose digests it checks (distributed.gather_records; GatherMismatch on a
        mismatch).  Other ranks return None.  Replaces the reference's
        worker_pool.starmap over the batch (generator.py:96-97)."""
        if group is None:
            return self.annotations_from_records(*self.decode_records(det_batch))
        import torch.distributed as dist  # pylint: disable=import-outside-toplevel
        from ...distributed import GatherMismatch, gather_records, shard
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        several = isinstance(det_batch, (list, tuple))
        n = 0 if det_batch is None else len(det_batch[0] if several else det_batch)
        a, b = (0, n) if local else shard(n, rank, world)
        if b > a:
            recs, offsets = self.decode_records([t[a:b] for t in det_batch] if several
                                                else det_batch[a:b])
        else:
            recs, offsets = np.zeros(0, DET_DTYPE), np.zeros(1, np.int64)
        nccl = dist.get_backend(group) == 'nccl'
        device = (torch.device('cuda', torch.cuda.current_device()) if nccl
                  else torch.device('cpu'))
        self.last_gather = {}
        recs, offsets = gather_records(recs, offsets, dist, device, dst=dst,
                                       report=self.last_gather, group=group)
        if recs is None:
            return None
        if self.last_gather['ranks_verified'] != world:
            raise GatherMismatch('gathered detections of {} of {} ranks do not match their '
                                 'digests'.format(world - self.last_gather['ranks_verified'],
                                                  world))
        return self.annotations_from_records(recs, offsets)

    def decode_heads(self, heads, *, group=None, dst=0, local=False):
        """Generator.batch: the model's head list (each (B, ...)); reads the CifDet head
        (`group` / `dst` / `local`: image-sharded, as decode_batch)."""
        kw = {} if group is None else {'group': group, 'dst': dst, 'local': local}
        if heads is None:  # this rank's shard of a sharded batch is empty
            return self.decode_batch(None, **kw)
        heads = self.head_fields(heads)
        return self.decode_batch(heads[0] if self.single_head() else heads, **kw)

    def __call__(self, fields):
        """generator/cifdet.py:27-52 for one image's field list."""
        heads = [_device.to_device(t)[None] for t in self.head_fields(fields)]
        return self.decode_batch(heads[0] if self.single_head() else heads)[0]
