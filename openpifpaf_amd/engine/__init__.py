"""Re-exports only: fields.py has the decoders' inputs, handover.py what both engines hand
records over with, pose.py the CifCaf engine and its pipeline, det.py the CifDet ones."""
from .det import DetBuffers, DetCall, DetEngine, DetPipeline, PendingDetRecords, det_call, det_tail
from .fields import (HeadSet, InitialAnnotations, RaggedDetFields, RaggedFields, RaggedHeadSet,
                     check_head_lists, head_scales)
from .handover import OutputSlots, PinnedBlock, gather_index, head_size, offsets_of
from .pose import (STAGE_AFTER_SEED_LOOP, STAGE_ALL, STAGE_CAF, STAGE_CIFHR, STAGE_COMPLETE_EARLY,
                   STAGE_COMPLETE_ONLY, STAGE_GROW, STAGE_NMS_BITMAP, STAGE_NMS_ONLY,
                   STAGE_NMS_WIDE, STAGE_SEED_LOOP_ONLY, STAGE_SEEDS, DecodeBuffers, DecodeEngine,
                   DecodePipeline, PendingRecords, default_ann_capacity, engine)
