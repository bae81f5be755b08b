"""CifCaf greedy pose decoder (decoder/generator/cifcaf.py:24-351) on gfx950.

Same constructor, class attributes and call signature as the reference.  One call runs the
whole per-image pipeline on the device (engine.DecodeEngine -> pp_decode_stages):
CifHr -> CifSeeds -> CafScored (both thresholds) -> seed loop with occupancy and the
frontier grow -> complete_annotations / flood fill -> nms.Keypoints, and returns
Annotation objects.  `decode_batch` decodes a whole (B, ...) batch of device fields in
one launch sequence, which is how `batch()` (generator.py:84-101) is served.
"""
from collections import defaultdict
import ctypes
import logging
import time

import numpy as np

from ... import _device, _edges, functional
from ..._abi import PACK_ALL, check_seed_mask, make_config, skeleton_array
from ...annotation import Annotation
from ...distributed import decode_sharded, shard
from ...engine import (HeadSet, InitialAnnotations, RaggedFields, RaggedHeadSet,
                       check_head_lists, engine)
from ...functional import _edge_call, grow_connection_blend
from .. import nms as nms_module
from ..caf_scored import CafScored
from ..cif_hr import CifHr
from ..cif_seeds import CifSeeds
from ..field_config import FieldConfig
from .generator import Generator

LOG = logging.getLogger(__name__)


class CifCaf(Generator):
    """Generate CifCaf poses from fields.

    :param: nms: set to None to switch off non-maximum suppression.
    """
    connection_method = 'blend'
    supports_sharding = True
    force_complete = False
    greedy = False
    keypoint_threshold = 0.0

    def __init__(self, field_config: FieldConfig, *, keypoints, skeleton, out_skeleton=None,
                 confidence_scales=None, worker_pool=None, nms=True):
        super().__init__(worker_pool)
        if nms is True:
            nms = nms_module.Keypoints()
        # nms.Keypoints (its own annotations()) runs inside the device decode; any other
        # object with an annotations(list) method (cifcaf.py:117-118) runs on the host over
        # each image's decoded list, which the device then leaves unsuppressed
        if nms is not None and not callable(getattr(nms, 'annotations', None)):
            raise TypeError('nms must provide annotations(annotations)')
        # confidence_scales (cifcaf.py:39,52): per-CAF weights on the frontier priorities
        # of _grow (cifcaf.py:259-260, 282-284), applied on the device (pp_config).  The
        # reference indexes it per CAF while growing; a list shorter than the skeleton
        # raises its IndexError here, before any decode -- deliberately stricter than the
        # reference (see config(), which checks again for lists replaced after __init__).
        if confidence_scales is not None and len(confidence_scales) < len(skeleton):
            raise IndexError('list index out of range (confidence_scales has {} entries for '
                             '{} CAF fields)'.format(len(confidence_scales), len(skeleton)))
        self.field_config = field_config
        self.keypoints = keypoints
        self.skeleton = skeleton
        self.skeleton_m1 = np.asarray(skeleton) - 1
        self.out_skeleton = out_skeleton or skeleton
        self.confidence_scales = confidence_scales
        self.nms = nms
        self.timers = defaultdict(float)
        # cifcaf.py:57-65 (kept for API parity; the kernel builds the same tables)
        self.by_target = defaultdict(dict)
        for caf_i, (j1, j2) in enumerate(self.skeleton_m1):
            self.by_target[j2][j1] = (caf_i, True)
            self.by_target[j1][j2] = (caf_i, False)
        self.by_source = defaultdict(dict)
        for caf_i, (j1, j2) in enumerate(self.skeleton_m1):
            self.by_source[j1][j2] = (caf_i, True)
            self.by_source[j2][j1] = (caf_i, False)

    # -- configuration -------------------------------------------------------------------
    def config(self):
        """pp_config from the class attributes decoder.configure() writes (factory.py:64-98)."""
        stride = int(self.field_config.cif_strides[0])  # multi-scale heads carry their own
        if CifSeeds.threshold is None:
            raise TypeError('CifSeeds.threshold is not configured (decoder.configure sets it)')
        nms = self.nms if self._device_nms() else None
        check_seed_mask(self.field_config.seed_mask, len(self.keypoints))
        # Deliberately stricter than the reference: it indexes confidence_scales per CAF
        # inside _grow and raises IndexError only when a grow reaches an edge past the end
        # of the list (cifcaf.py:259-260, 282-284), so a decode that never grows such an
        # edge succeeds there.  The device table needs every edge's weight up front, so a
        # short list raises the same IndexError here, at the start of every decode.
        cs = self.confidence_scales
        if cs is not None and len(cs) < len(self.skeleton):
            raise IndexError('list index out of range (confidence_scales has {} entries for '
                             '{} CAF fields)'.format(len(cs), len(self.skeleton)))
        return make_config(
            cif_threshold=CifHr.v_threshold,
            seed_threshold=CifSeeds.threshold,
            seed_score_scale=CifSeeds.score_scale,
            caf_threshold=CafScored.default_score_th,
            complete_caf_threshold=0.0001,
            keypoint_threshold=self.keypoint_threshold,
            nms_keypoint_threshold=nms.keypoint_threshold if nms else 0.0,
            nms_instance_threshold=nms.instance_threshold if nms else 0.0,
            nms_suppression=nms.suppression if nms else 0.0,
            stride=stride,
            cif_neighbors=CifHr.neighbors,
            force_complete=self.force_complete,
            greedy=self.greedy,
            connection_method=self.connection_method,
            apply_nms=nms is not None,
            seed_mask=self.field_config.seed_mask,
            confidence_scales=self.confidence_scales,
        )

    def _device_nms(self):
        """nms.Keypoints (not a subclass overriding annotations()) runs on the device."""
        return (isinstance(self.nms, nms_module.Keypoints) and
                type(self.nms).annotations is nms_module.Keypoints.annotations)

    def _host_nms(self, anns):
        """cifcaf.py:117-118 for an NMS object other than nms.Keypoints."""
        if self.nms is None or self._device_nms():
            return anns
        return self.nms.annotations(anns)

    # -- decoding ------------------------------------------------------------------------
    def __call__(self, fields, initial_annotations=None):
        """One image: fields = the head outputs [cif (K, 5, H, W), caf (C, 9, H, W), ...]
        (numpy or device), read through the FieldConfig (single- or multi-scale)."""
        start = time.perf_counter()
        if initial_annotations:
            anns = self._call_initial(fields, list(initial_annotations))
            LOG.debug('%d annotations, %.3fs', len(anns), time.perf_counter() - start)
            return anns
        if self.field_config.is_single_scale():
            cif_i, caf_i, _ = self.field_config.single_scale()
            anns = self.decode_batch(_device.to_device(fields[cif_i])[None],
                                     _device.to_device(fields[caf_i])[None])[0]
        else:
            used = set(self.field_config.cif_indices) | set(self.field_config.caf_indices)
            batched = [_device.to_device(f)[None] if i in used else None
                       for i, f in enumerate(fields)]
            anns = self.decode_fields_batch(batched)[0]
        LOG.debug('%d annotations, %.3fs', len(anns), time.perf_counter() - start)
        return anns

    def _call_initial(self, fields, initial):
        """cifcaf.py:67-71, 95-98: the initial annotations are grown first, marked occupied
        and kept in the annotation list (pp_decode_initial).  As in the reference, the
        returned list holds the same initial Annotation objects, mutated (grown, completed,
        NMS-suppressed); one that NMS drops is mutated too (the reference edits the objects
        in place before filtering, nms.py:20-53), from the decode's working records
        (pp_decode_multi_work_offset)."""
        init = InitialAnnotations([np.stack([a.to_record() for a in initial])],
                                  _device.require())
        skel = skeleton_array(self.skeleton)
        if self.field_config.is_single_scale():
            cif_i, caf_i, _ = self.field_config.single_scale()
            recs, offsets, b = engine().decode(_device.to_device(fields[cif_i])[None],
                                               _device.to_device(fields[caf_i])[None], skel,
                                               self.config(), initial=init)
        else:
            used = set(self.field_config.cif_indices) | set(self.field_config.caf_indices)
            heads = HeadSet([_device.to_device(f)[None] if i in used else None
                             for i, f in enumerate(fields)], self.field_config)
            recs, offsets, b = engine().decode(None, None, skel, self.config(), heads=heads,
                                               initial=init)
        n = int(offsets[1])
        index = b.out_index[:n].cpu().numpy()
        out = []
        for rec, idx in zip(recs[:n], index):
            if 0 <= idx < len(initial):
                out.append(initial[idx].update_from_record(rec))
            else:
                out.append(Annotation.from_record(rec, self.keypoints, self.out_skeleton))
        dropped = sorted(set(range(len(initial))) - set(int(i) for i in index))
        if dropped:
            for i, rec in zip(dropped, b.work_records(0, dropped)):
                initial[i].update_from_record(rec)
        return self._host_nms(out)

    def decode_records(self, cif_batch, caf_batch, keep_cifhr=False, compact=None):
        """Device decode of a batch -> (packed records, per-image offsets, buffers): full
        pp_ann records, or compact ones (pp_pack_compact) with `compact` flags."""
        cif = _device.to_device(cif_batch)
        caf = _device.to_device(caf_batch)
        return engine().decode(cif, caf, skeleton_array(self.skeleton), self.config(),
                               keep_cifhr=keep_cifhr, compact=compact)

    def decode_fields_records(self, fields_batch, keep_cifhr=False, compact=None):
        """Multi-scale device decode (pp_decode_multi): fields_batch is the head output list
        with a batch dimension, indexed by the FieldConfig (factory.py:153-180)."""
        heads = HeadSet([None if f is None else _device.to_device(f) for f in fields_batch],
                        self.field_config)
        return engine().decode(None, None, skeleton_array(self.skeleton), self.config(),
                               keep_cifhr=keep_cifhr, heads=heads, compact=compact)

    def annotations_from_records(self, recs, offsets):
        """Full or compact records + per-image offsets -> one list of Annotation per image."""
        out = []
        for i in range(len(offsets) - 1):
            out.append(self._host_nms([Annotation.from_any(r, self.keypoints, self.out_skeleton)
                                       for r in recs[offsets[i]:offsets[i + 1]]]))
        return out

    def decode_heads(self, heads, *, group=None, dst=0, local=False):
        """Generator.batch: the model's head list (each (B, ...)) through the FieldConfig.
        `group` / `dst` / `local`: image-sharded over a process group (decode_batch)."""
        kw = {} if group is None else {'group': group, 'dst': dst, 'local': local}
        if heads is None:  # this rank's shard of a sharded batch is empty
            return self.decode_batch(None, None, **kw)
        if self.field_config.is_single_scale():
            cif_i, caf_i, _ = self.field_config.single_scale()
            return self.decode_batch(heads[cif_i], heads[caf_i], **kw)
        used = set(self.field_config.cif_indices) | set(self.field_config.caf_indices)
        return self.decode_fields_batch([h if i in used else None for i, h in enumerate(heads)],
                                        **kw)

    def decode_batch(self, cif_batch, caf_batch, *, group=None, dst=0, local=False):
        """(B, K, 5, H, W) + (B, C, 9, H, W) -> one list of Annotation per image.

        With a torch.distributed process `group` (e.g. `dist.group.WORLD`: one rank per
        GPU, nccl = RCCL over xGMI, or gloo; the nccl leg has not yet run on hardware with
        more than one GPU), the batch is image-sharded: each rank decodes
        its contiguous `distributed.shard` of the B images (every rank passes the whole
        batch; `local=True`: the arguments are already this rank's images, possibly None
        for none), and rank `dst` returns the annotation lists of all images in rank order,
        gathered as compact records whose digests it checks (distributed.decode_sharded;
        GatherMismatch on a mismatch).  Other ranks return None.  This replaces the
        reference's worker_pool.starmap over the batch (generator.py:96-97)."""
        if group is None:
            recs, offsets, _ = self.decode_records(cif_batch, caf_batch, compact=PACK_ALL)
            return self.annotations_from_records(recs, offsets)
        n = 0 if cif_batch is None else len(cif_batch)
        return self._decode_sharded(
            n, lambda a, b: (_device.to_device(cif_batch[a:b]).contiguous(),
                             _device.to_device(caf_batch[a:b]).contiguous(), None),
            group, dst, local)

    def decode_fields_batch(self, fields_batch, *, group=None, dst=0, local=False):
        """Batched head outputs of any FieldConfig -> one list of Annotation per image
        (`group` / `dst` / `local`: image-sharded, as decode_batch)."""
        if group is None:
            recs, offsets, _ = self.decode_fields_records(fields_batch, compact=PACK_ALL)
            return self.annotations_from_records(recs, offsets)
        n = 0 if fields_batch is None else len(
            fields_batch[self.field_config.cif_indices[0]])

        def take(a, b):
            fields = [None if f is None else _device.to_device(f[a:b]).contiguous()
                      for f in fields_batch]
            return None, None, HeadSet(fields, self.field_config)
        return self._decode_sharded(n, take, group, dst, local)

    def coco_batch(self, cif_batch, caf_batch, metas, **params):
        """(B, K, 5, H, W) + (B, C, 9, H, W) and one meta dict per image (with 'image_id')
        -> the batch's eval_coco.CocoRecords: EvalCoco.from_predictions
        (eval_coco.py:108-158) on the device behind the decode, without Annotation objects.
        `params`: small_threshold, max_per_image, category_id."""
        return self._coco(_device.to_device(cif_batch), _device.to_device(caf_batch), None, metas,
                          params)

    def coco_heads(self, heads, metas, **params):
        """coco_batch from the model's head list (each (B, ...)) through the FieldConfig."""
        if self.field_config.is_single_scale():
            cif_i, caf_i, _ = self.field_config.single_scale()
            return self.coco_batch(heads[cif_i], heads[caf_i], metas, **params)
        used = set(self.field_config.cif_indices) | set(self.field_config.caf_indices)
        head_set = HeadSet([_device.to_device(h) if i in used else None
                            for i, h in enumerate(heads)], self.field_config)
        return self._coco(None, None, head_set, metas, params)

    # -- ragged batches: images of different field sizes -----------------------------------
    def _ragged(self, fields_list, kw):
        """RaggedFields (single-scale FieldConfig) or RaggedHeadSet (any other) of a list of
        per-image head lists (Generator.fields_batch entries, each read through the
        FieldConfig), packed on the device."""
        for name in ('group', 'initial_annotations', 'keep_cifhr'):
            if kw.pop(name, None):
                raise NotImplementedError(
                    'a ragged batch does not take {}: its decode is single-GPU, starts from '
                    'the seeds and keeps no dense CifHr map'.format(name))
        if kw:
            raise TypeError('unexpected arguments: ' + ', '.join(sorted(kw)))
        if isinstance(fields_list, (RaggedFields, RaggedHeadSet)):  # packed or ingested already
            if isinstance(fields_list, RaggedFields) != self.field_config.is_single_scale():
                raise TypeError('a single-scale FieldConfig decodes a RaggedFields, a '
                                'multi-scale one a RaggedHeadSet')
            return fields_list
        if not self.field_config.is_single_scale():
            check_head_lists(self.field_config)  # before anything goes to the device
            used = set(self.field_config.cif_indices) | set(self.field_config.caf_indices)
            return RaggedHeadSet([[_device.to_device(h) if i in used else None
                                   for i, h in enumerate(f)] for f in fields_list],
                                 self.field_config)
        cif_i, caf_i, _ = self.field_config.single_scale()
        return RaggedFields([(_device.to_device(f[cif_i]), _device.to_device(f[caf_i]))
                             for f in fields_list])

    def decode_ragged(self, fields_list, **kw):
        """One entry per image, each image's head outputs [cif (K, 5, h_i, w_i), caf (C, 9,
        h_i, w_i), ...] at its OWN size (what Generator.fields_batch returns, from any
        number of forward passes) -> one list of Annotation per image, each as __call__
        gives it for that image alone, decoded as one device batch (pp_decode_ragged).  With a
        multi-scale FieldConfig every head of an image has its own size and the batch takes
        pp_decode_multi_ragged.  An engine.RaggedFields (e.g. RaggedFields.from_conv,
        heads.RaggedCollector) or, multi-scale, an engine.RaggedHeadSet in place of the list
        is decoded as it is."""
        ragged = self._ragged(fields_list, kw)
        recs, offsets, _ = engine().decode(None, None, skeleton_array(self.skeleton),
                                           self.config(), compact=PACK_ALL, ragged=ragged)
        return self.annotations_from_records(recs, offsets)

    def coco_ragged(self, fields_list, metas, **params):
        """coco_batch for images of different field sizes (decode_ragged's `fields_list`)."""
        ragged = self._ragged(fields_list, {k: params.pop(k) for k in
                                            ('group', 'initial_annotations', 'keep_cifhr')
                                            if k in params})
        return self._coco(None, None, None, metas, params, ragged=ragged)

    def _coco(self, cif, caf, heads, metas, params, ragged=None):
        from ...eval_coco import metas_device  # pylint: disable=import-outside-toplevel
        if self.nms is not None and not self._device_nms():
            raise TypeError('coco_batch needs the device NMS (nms.Keypoints or None): a host '
                            'NMS object leaves no device records')
        n = ragged.n if ragged is not None else len(cif) if heads is None else heads.n
        if len(metas) != n:
            raise ValueError('{} metas for {} images'.format(len(metas), n))
        b = engine().launch_checked(cif, caf, skeleton_array(self.skeleton), self.config(),
                                    heads=heads, ragged=ragged)
        d_metas, d_ids, d_swap = metas_device(metas, len(self.keypoints))
        return engine().fetch_coco_async(b, d_metas, d_ids, hswap=d_swap, **params).result()

    def _decode_sharded(self, n, take, group, dst, local):
        import torch.distributed as dist  # pylint: disable=import-outside-toplevel
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        a, b = (0, n) if local else shard(n, rank, world)
        cfg, skel = self.config(), skeleton_array(self.skeleton)

        def decode_local(device_out):
            cif, caf, heads = take(a, b)
            _, pending = engine().decode_async(cif, caf, skel, cfg, heads=heads,
                                               compact=PACK_ALL, device_out=device_out)
            return pending
        self.last_gather = {}
        recs, offsets = decode_sharded(decode_local, b - a, dist, group=group, dst=dst,
                                       report=self.last_gather)
        if recs is None:
            return None
        return self.annotations_from_records(recs, offsets)

    # -- reference building blocks, on the device ------------------------------------------
    def _grow_connection(self, xy, xy_scale, caf_field):
        assert len(xy) == 2
        assert caf_field.shape[0] == 9
        return grow_connection_blend(caf_field, xy[0], xy[1], xy_scale,
                                     connection_method=self.connection_method)

    def connection_value(self, ann, caf_scored, start_i, end_i, *, reverse_match=True):
        """cifcaf.py:194-217 on the device (one launch of pp_connection_values): the joint
        that the CAF from start_i to end_i connects ann's start joint to, as (x, y, scale,
        score) of four np.float32, or (0.0, 0.0, 0.0, 0.0).  caf_scored: anything with the
        reference's directed(caf_i, forward), host- or device-backed.  Inputs are converted
        to float32 first: for Python-float inputs the reference computes (and returns) in
        float64, which this does not follow."""
        caf_i, forward = self.by_source[start_i][end_i]
        caf_f, caf_b = caf_scored.directed(caf_i, forward)
        xyv = ann.data[start_i]
        r = functional.connection_values(
            [caf_b, caf_f], [[xyv[0], xyv[1], xyv[2], ann.joint_scales[start_i]]], [1],
            connection_method=self.connection_method,
            keypoint_threshold=self.keypoint_threshold, reverse_match=reverse_match)[0]
        if not r.any():
            return 0.0, 0.0, 0.0, 0.0
        return tuple(np.float32(v) for v in r)

    @staticmethod
    def p2p_value(source_xyv, caf_scored, source_s, target_xysv, caf_i, forward):
        """cifcaf.py:219-245 on the device (one launch of pp_p2p_values): how well the CAF
        caf_i connects the source joint to the target joint, an np.float32, or 0.0 when no
        column lies in the source's box.  The reference's max() over the kept columns is
        restated: NaN exactly when the first kept column's score is NaN, a NaN of a later
        column is ignored.  Inputs are converted to float32 first (the reference computes
        Python-float inputs in float64; this does not)."""
        caf_f, _ = caf_scored.directed(caf_i, forward)
        r = functional.p2p_values(
            [caf_f], [[source_xyv[0], source_xyv[1], source_xyv[2], source_s]],
            [[target_xysv[0], target_xysv[1], target_xysv[2]]], [0])[0]
        return 0.0 if r.view(np.uint32) == 0 else np.float32(r)

    def connection_values(self, anns, caf_scored, *, reverse_match=True, device=False):
        """connection_value for every directed skeleton edge of every annotation in ONE
        launch: (n_ann, 2C, 4) float32, [a, 2 * caf_i] the forward edge (start j1, end j2)
        and [a, 2 * caf_i + 1] the backward one (start j2, end j1) of self.skeleton's CAF
        caf_i.  Each element is what connection_value returns for that argument tuple,
        unset start joints (v == 0) included.  device=True: a device tensor, no sync."""
        q = _edges.connection_queries(_edges.annotation_table(anns, len(self.keypoints)),
                                      self.skeleton_m1)
        sets = _edges.caf_scored_sets(caf_scored, len(self.skeleton_m1), _device.require())
        r = _edge_call('pp_connection_values', sets, q,
                       _edges.method_bits(self.connection_method, 'numpy_simd'),
                       (ctypes.c_float(self.keypoint_threshold),
                        ctypes.c_int32(bool(reverse_match))), (4,), device)
        return r.reshape(len(anns), 2 * len(self.skeleton_m1), 4)

    @staticmethod
    def p2p_values(sources, targets, caf_scored, skeleton, *, device=False):
        """p2p_value of every source annotation's joint at an edge's start against every
        target annotation's joint at its end, in ONE launch: (n_src, n_tgt, C, 2) float32,
        [s, t, caf_i, 0] forward (source joint j1, target joint j2), [s, t, caf_i, 1]
        backward (source j2, target j1).  skeleton: 1-based joint pairs, as CifCaf's.  Each
        element is what p2p_value returns for that argument tuple, unset joints included.
        device=True: a device tensor, no sync."""
        skel = np.asarray(skeleton, dtype=np.int64).reshape(-1, 2) - 1
        k = int(skel.max()) + 1 if len(skel) else 0
        q = _edges.p2p_queries(_edges.annotation_table(sources, k),
                               _edges.annotation_table(targets, k), skel)
        sets = _edges.caf_scored_sets(caf_scored, len(skel), _device.require())
        r = _edge_call('pp_p2p_values', sets, q, _edges.method_bits('blend', 'numpy_simd'), (),
                       (), device)
        return r.reshape(len(sources), len(targets), len(skel), 2)
