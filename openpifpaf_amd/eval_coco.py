"""COCO prediction records (eval_coco.py:108-158, EvalCoco.from_predictions).

`coco_predictions(predictions, meta)` maps decoded annotations to image coordinates on
the device (transforms.Preprocess.annotations_inverse), applies EvalCoco's small-object
filter and per-image cap, and returns the json records pycocotools reads.  The COCO
evaluation itself (pycocotools) is not part of this package.

`coco_records(...)` does the same for a whole batch of device records in two launches
(pp_coco_keypoints / pp_coco_dets): one meta per image, the finished records packed image
after image into pinned host memory, the decode's records left as they are.
`CocoRecords.predictions()` is the list `coco_predictions` gives image by image, and
`Predictions` collects batches and writes the files of EvalCoco.write_predictions
(eval_coco.py:160-171).
"""
import ctypes
import json
import zipfile

import numpy as np
import torch

from . import _device, transforms
from ._abi import (COCO_DET_DTYPE, PP_COCO_EMPTY, PP_COCO_NAN, PP_ST_ANN_OVERFLOW,
                   PP_ST_DEC_OVERFLOW, PP_ST_NMS_OVERFLOW, CocoParams, coco_dtype)
from ._lib import PPError, call, load
from .engine.handover import PinnedBlock, offsets_of

KEYS = ('category_id', 'score', 'keypoints', 'bbox', 'image_id')


def coco_predictions(predictions, meta, *, small_threshold=0.0, max_per_image=20,
                     n_keypoints=17):
    image_id = int(meta['image_id'])
    predictions = transforms.Preprocess.annotations_inverse(predictions, meta)
    if small_threshold:
        predictions = [pred for pred in predictions
                       if pred.scale(v_th=0.01) >= small_threshold]
    if len(predictions) > max_per_image:
        predictions = predictions[:max_per_image]
    image_annotations = []
    for pred in predictions:
        pred_data = pred.json_data()
        pred_data['image_id'] = image_id
        image_annotations.append({k: v for k, v in pred_data.items() if k in KEYS})
    if not image_annotations:  # at least one record per image (for pycocotools)
        image_annotations.append({
            'image_id': image_id,
            'category_id': 1,
            'keypoints': np.zeros((n_keypoints * 3,)).tolist(),
            'bbox': [0, 0, 1, 1],
            'score': 0.001,
        })
    return image_annotations


def metas_device(metas, k=17, device=None):
    """(META_DTYPE block, image ids, swap table or None) as device tensors from a list of the
    reference's meta dicts (transforms/annotations.py:39-44, with 'image_id').  One swap
    table serves a batch: every flipped image that has a `horizontal_swap` must give the
    same table."""
    device = device or _device.require()
    block = np.concatenate([transforms.meta_record(m) for m in metas]) if metas else \
        np.zeros(0, transforms.META_DTYPE)
    ids = np.asarray([int(m['image_id']) for m in metas], np.int64)
    table = None
    for m in metas:
        if m['hflip'] and m.get('horizontal_swap'):
            t = transforms.swap_table(m['horizontal_swap'], k)
            if table is not None and not np.array_equal(table, t):
                raise ValueError('the flipped images of one batch need one horizontal_swap')
            table = t
    if table is not None and any(m['hflip'] and not m.get('horizontal_swap') for m in metas):
        raise ValueError('a flipped image without horizontal_swap beside one with it')
    d_metas = torch.from_numpy(block.view(np.uint8).reshape(-1)).to(device)
    d_ids = torch.from_numpy(ids).to(device)
    d_swap = None if table is None else torch.from_numpy(table).to(device)
    return d_metas, d_ids, d_swap


class CocoRecords:
    """The COCO prediction records of a batch: `records` (a structured array,
    _abi.coco_dtype(k) or COCO_DET_DTYPE, image after image), `offsets` (n + 1) and per-image
    `flags` (PP_COCO_NAN, PP_COCO_EMPTY)."""

    def __init__(self, records, offsets, flags, k, det=False):
        self.records, self.offsets, self.flags = records, offsets, flags
        self.k, self.det = k, det

    def check(self):
        """The reference asserts inside annotations_inverse (preprocess.py:67)."""
        if (self.flags & PP_COCO_NAN).any():
            raise AssertionError('NaN in annotation data (preprocess.py:67)')
        return self

    def image(self, i):
        """from_predictions' records of image i, in its key order."""
        recs = self.records[self.offsets[i]:self.offsets[i + 1]]
        if self.flags[i] & PP_COCO_EMPTY:
            return [{'image_id': int(recs[0]['image_id']), 'category_id': 1,
                     'keypoints': np.zeros((self.k * 3,)).tolist(), 'bbox': [0, 0, 1, 1],
                     'score': 0.001}]
        ids, cats = recs['image_id'].tolist(), recs['category_id'].tolist()
        scores, boxes = recs['score'].tolist(), recs['bbox'].tolist()
        if self.det:
            return [{'category_id': c, 'score': s, 'bbox': b, 'image_id': i_}
                    for c, s, b, i_ in zip(cats, scores, boxes, ids)]
        kps = recs['keypoints'].reshape(len(recs), -1).tolist()
        return [{'keypoints': kp, 'bbox': b, 'score': s, 'category_id': c, 'image_id': i_}
                for kp, b, s, c, i_ in zip(kps, boxes, scores, cats, ids)]

    def predictions(self):
        """What `coco_predictions` returns image by image, concatenated."""
        self.check()
        out = []
        for i in range(len(self.offsets) - 1):
            out += self.image(i)
        return out


class PendingCoco:
    """COCO records enqueued by `coco_records` / DecodeEngine.fetch_coco_async: a pinned
    block (counts, decode status, flags, then the records) the device writes zero-copy."""

    def __init__(self, launch, block, k, det, stream):
        self._launch, self._block, self._k, self._det, self._stream = launch, block, k, det, stream
        self.dtype = COCO_DET_DTYPE if det else coco_dtype(k)

    @property
    def done_event(self):
        return self._block.done

    def result(self):
        """The batch's CocoRecords (waits; packs again when the batch outgrew the block)."""
        block = self._block
        block.wait()
        status = block.status()
        bad = status & (PP_ST_ANN_OVERFLOW | PP_ST_DEC_OVERFLOW | PP_ST_NMS_OVERFLOW)
        if bad.any():
            raise PPError('decode status flags set (records truncated): {}'.format(
                status[bad != 0][:8].tolist()))
        offsets = offsets_of(block.counts())
        total = int(offsets[-1])
        if total > block.est:
            return self._launch(2 * total, self._stream).result()
        return CocoRecords(block.records(total, self.dtype), offsets, block.flags(), self._k,
                           self._det)


def coco_records_async(recs, counts, metas, image_ids, *, k=17, hswap=None, small_threshold=0.0,
                       max_per_image=20, category_id=1, det=False, status=None, capacity=0,
                       stream=None):
    """Enqueue pp_coco_keypoints / pp_coco_dets over device record batches `recs`
    (n_img, cap, record bytes) with per-image `counts` (device int32), `metas` (device
    META_DTYPE bytes), `image_ids` (device int64) and the optional swap table `hswap` (device
    int32) on `stream` (default: the current stream); returns a PendingCoco.  `status`: the
    decode's per-image status words, copied beside the counts.  The records go straight
    into a pinned host block sized for `capacity` records (default: max_per_image per
    image, which always fits)."""
    n, cap = recs.shape[0], recs.shape[1]
    params = CocoParams(float(small_threshold), int(max_per_image), int(category_id))
    width = (COCO_DET_DTYPE if det else coco_dtype(k)).itemsize
    ws_size = max(256, int(load().pp_coco_workspace_size(n)))

    def launch(est, side):
        block = PinnedBlock(n, 3, est, width)  # counts, the decode's status, flags, records
        block.word_bytes(1).zero_()
        with torch.cuda.stream(side):
            # the per-image counts between the two launches; one per call, so calls on
            # different streams do not share it
            ws = torch.empty(ws_size, dtype=torch.uint8, device=recs.device)
            tail = (ctypes.byref(params), block.records_ptr(), est, block.ptr(0), block.ptr(2),
                    _device.ptr(ws), _device.stream())
            if det:
                call('pp_coco_dets', _device.ptr(recs), _device.ptr(counts), n, cap,
                     _device.ptr(metas), _device.ptr(image_ids), *tail)
            else:
                call('pp_coco_keypoints', _device.ptr(recs), _device.ptr(counts), n, cap, k,
                     _device.ptr(metas), _device.ptr(image_ids), _device.ptr(hswap), *tail)
            if status is not None:
                block.word_bytes(1).copy_(status.view(torch.uint8), non_blocking=True)
            block.done = torch.cuda.Event()
            block.done.record()
            for t in (recs, counts, metas, image_ids, hswap, status):
                if t is not None:
                    t.record_stream(side)
        return PendingCoco(launch, block, k, det, side)

    est = max(int(capacity), 1) if capacity else max(1, n * min(int(max_per_image), cap))
    return launch(est, stream or torch.cuda.current_stream(recs.device))


def coco_records(recs, counts, metas, image_ids, *, k=17, hswap=None, small_threshold=0.0,
                 max_per_image=20, category_id=1, det=False):
    """EvalCoco.from_predictions (eval_coco.py:108-158) over a batch of device records, as
    transforms.inverse_records takes them; the records are not modified.  Returns the
    batch's CocoRecords."""
    return coco_records_async(recs, counts, metas, image_ids, k=k, hswap=hswap,
                              small_threshold=small_threshold, max_per_image=max_per_image,
                              category_id=category_id, det=det).result()


def coco_records_cpu(recs, counts, metas, image_ids, *, k=17, hswap=None, small_threshold=0.0,
                     max_per_image=20, category_id=1, det=False, out_capacity=None):
    """The host twins pp_coco_keypoints_cpu / pp_coco_dets_cpu on NumPy arrays: `recs`
    (n_img, cap) ANN_DTYPE or DET_DTYPE, `counts` int32, `metas` META_DTYPE, `image_ids`
    int64, `hswap` int32 or None.  Byte for byte what the device writes."""
    recs = np.ascontiguousarray(recs)
    n, cap = recs.shape
    counts = np.ascontiguousarray(counts, np.int32)
    metas = np.ascontiguousarray(metas, transforms.META_DTYPE)
    image_ids = np.ascontiguousarray(image_ids, np.int64)
    hswap = None if hswap is None else np.ascontiguousarray(hswap, np.int32)
    params = CocoParams(float(small_threshold), int(max_per_image), int(category_id))
    dtype = COCO_DET_DTYPE if det else coco_dtype(k)
    est = n * max(1, min(int(max_per_image), cap)) if out_capacity is None else out_capacity
    out = np.full(max(est, 1) * dtype.itemsize, 0xFF, np.uint8)
    out_counts, flags = np.zeros(n, np.int32), np.zeros(n, np.int32)
    vp = lambda a: ctypes.c_void_p(None if a is None else a.ctypes.data)  # noqa: E731
    tail = (ctypes.byref(params), vp(out), est, vp(out_counts), vp(flags))
    if det:
        call('pp_coco_dets_cpu', vp(recs), vp(counts), n, cap, vp(metas), vp(image_ids), *tail)
    else:
        call('pp_coco_keypoints_cpu', vp(recs), vp(counts), n, cap, k, vp(metas), vp(image_ids),
             vp(hswap), *tail)
    offsets = offsets_of(out_counts)
    total = min(int(offsets[-1]), est)
    return CocoRecords(out[:total * dtype.itemsize].view(dtype), offsets, flags, k, det)


class Predictions:
    """EvalCoco's prediction list (eval_coco.py:54, 158) filled batch by batch."""

    def __init__(self):
        self.predictions = []
        self.image_ids = []

    def from_batch(self, records):
        """Append a CocoRecords' predictions (from_predictions for each of its images)."""
        preds = records.predictions()
        self.image_ids += [int(records.records[records.offsets[i]]['image_id'])
                           for i in range(len(records.offsets) - 1)]
        self.predictions += preds
        return self

    def write_predictions(self, filename):
        """eval_coco.py:160-171: `filename`.pred.json and `filename`.zip."""
        predictions = [{k: v for k, v in annotation.items()
                        if k in ('image_id', 'category_id', 'keypoints', 'score')}
                       for annotation in self.predictions]
        with open(filename + '.pred.json', 'w') as f:
            json.dump(predictions, f)
        with zipfile.ZipFile(filename + '.zip', 'w') as myzip:
            myzip.write(filename + '.pred.json', arcname='predictions.json')
