"""The detection decoder's engine (decoder/generator/cifdet.py): persistent buffers, the
record hand-over through pinned host memory and overlapped batches, as pose.py for CifCaf."""
import collections
import ctypes
import logging

import numpy as np
import torch

from .. import _device
from .._abi import DET_DTYPE, PP_ST_ANN_OVERFLOW, scale_list
from .._lib import PPError, call, load
from .fields import RaggedDetFields
from .handover import OutputSlots, PinnedBlock, offsets_of

LOG = logging.getLogger(__name__)

DetCall = collections.namedtuple(
    'DetCall', 'name lead batch n k kind shape cells device cap size')


def det_call(cifdet, batch):
    """The CifDet entry point of `batch` for decoder `cifdet`: its `name` and `lead`ing
    arguments (det_tail has the rest), the checked device `batch`, `n` images of `k`
    categories, the buffer-key parts `kind` and `shape`, `cells` per category (k * cells
    bounds the capacity), the `device`, the default capacity `cap` and the workspace size as
    `size(cfg, cap)`.  `batch`: a (B, K, 7, H, W) tensor (pp_cifdet_decode), the list of the
    heads of a multi-head or min-scale FieldConfig (pp_cifdet_decode_multi), or a
    RaggedDetFields (pp_cifdet_decode_ragged)."""
    lib = load()
    if isinstance(batch, RaggedDetFields):
        n, k, h, w = batch.n, batch.k, batch.h, batch.w
        lead = (_device.ptr(batch.det), n, k, h, w, _device.ptr(batch.extents),
                batch.extents_host.ctypes.data_as(ctypes.c_void_p))
        return DetCall('pp_cifdet_decode_ragged', lead, batch, n, k, 'ragged', (h, w), h * w,
                       batch.det.device, max(64, h * w), lambda cfg, cap: int(
                           lib.pp_cifdet_ragged_workspace_size(n, k, h, w, ctypes.byref(cfg), cap)))
    heads = cifdet.device_heads(batch)
    n, k, _, h, w = heads[0].shape
    cells, dev = sum(t.shape[3] * t.shape[4] for t in heads), heads[0].device
    if cifdet.single_head():
        return DetCall('pp_cifdet_decode', (_device.ptr(heads[0]), n, k, h, w), heads[0], n, k,
                       'single', (h, w), cells, dev, max(64, h * w), lambda cfg, cap: int(
                           lib.pp_cifdet_workspace_size(n, k, h, w, ctypes.byref(cfg), cap)))
    fc = cifdet.field_config
    arr = scale_list([(t.data_ptr(), t.shape[3], t.shape[4]) for t in heads], [],
                     fc.cif_strides, [], fc.cif_min_scales)
    pairs = int(len(heads) == 10)  # CifHr.fill's 10-head layout (cif_hr.py:68-73)
    shape = (pairs,) + tuple((s.H, s.W, s.stride, s.cif_min_scale) for s in arr)
    return DetCall('pp_cifdet_decode_multi', (arr, len(arr), pairs, n, k), heads, n, k, 'multi',
                   shape, cells, dev, max(64, h * w), lambda cfg, cap: int(
                       lib.pp_cifdet_multi_workspace_size(arr, len(arr), pairs, n, k, cap)))


def det_tail(cfg, z, out, cap, counts, status, ws):
    """What every CifDet entry point ends in: the configs, no CifHr map, the outputs, the
    workspace and the stream."""
    return (ctypes.byref(cfg), ctypes.byref(z), _device.ptr(None), _device.ptr(out), cap,
            _device.ptr(counts), _device.ptr(status), _device.ptr(ws),
            ctypes.c_size_t(ws.numel()), _device.stream())


class DetBuffers(OutputSlots):
    """Workspace + two output slots (records, counts, status) of one CifDet decode shape:
    DecodeBuffers for the detection decoder.  `bound` is the capacity no image can exceed
    (K * cells), where the overflow retry stops."""

    def __init__(self, key, n, cap, size, bound, device):
        self.key, self.n, self.cap, self.bound = key, n, cap, bound
        self.ws = torch.empty(size, dtype=torch.uint8, device=device)
        super().__init__(lambda: (
            torch.empty((n, cap, DET_DTYPE.itemsize), dtype=torch.uint8, device=device),
            torch.zeros(n, dtype=torch.int32, device=device),
            torch.zeros(n, dtype=torch.int32, device=device)))
        self.busy = None  # event behind the last decode / pack enqueued on these buffers
        self.inputs = None  # (cifdet, device batch, config) of the last launch, for its retry

    out = OutputSlots.records

    def storage(self):
        """data_ptr of the workspace and of each slot's records, counts and status."""
        return (self.ws.data_ptr(),) + tuple(t.data_ptr() for t in self.slot(0) + self.slot(1))


class DetEngine:
    """The persistent state of one CifDet: per (entry point, batch shape, capacity) a
    workspace and two output slots (DetBuffers), kept between calls, and the record
    hand-over through pp_pack_det_records.  launch() enqueues one decode, fetch_async() its
    pack into a pinned host block (records, counts and status: one synchronisation hands
    over everything), PendingDetRecords.result() waits.  A call of a shape seen before
    allocates nothing on the device.

    A slot is not rewritten before the pack that reads it is done (OutputSlots.next_slot),
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
        cfg, z = config or (cifdet.config(), cifdet.nms_config())
        d = det_call(cifdet, batch)
        cap = cap or d.cap
        size = d.size(cfg, cap)
        b = self.buffers((d.kind, d.n, d.k, d.shape, cap, size, d.device), d.n, cap, size,
                         d.k * d.cells, d.device)
        if b.busy is not None:
            torch.cuda.current_stream(d.device).wait_event(b.busy)
        b.next_slot()
        call(d.name, *d.lead, *det_tail(cfg, z, b.out, cap, b.counts, b.status, b.ws))
        b.busy = torch.cuda.Event()
        b.busy.record()
        b.inputs = (cifdet, d.batch, (cfg, z))
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
        p = self._pack(b, b.current, b.inputs, est, stream)
        b.busy = p.done_event
        return p

    def _pack(self, b, slot_i, inputs, est, stream=None):
        """The pack of slot `slot_i`, which it releases: the slot's next decode waits for it."""
        records, counts, status = b.slot(slot_i)
        block = PinnedBlock(b.n, 2, est, DET_DTYPE.itemsize)  # counts, status, the records
        cur = torch.cuda.current_stream(records.device)
        side = cur if stream is None else stream
        if side != cur:
            side.wait_stream(cur)
        with torch.cuda.stream(side):
            call('pp_pack_det_records', _device.ptr(records), _device.ptr(counts),
                 _device.ptr(status), b.n, b.cap, block.records_ptr(), est, block.ptr(0),
                 block.ptr(1), _device.stream())
            block.done = torch.cuda.Event()
            block.done.record()
        b.released_by(slot_i, block.done)
        return PendingDetRecords(self, b, slot_i, inputs, block)

    def decode_async(self, cifdet, batch, cap=None, config=None):
        """launch + fetch_async: one decode and one pack on the current stream."""
        return self.fetch_async(self.launch(cifdet, batch, cap, config))


class PendingDetRecords:
    """A detection record fetch enqueued by DetEngine.fetch_async.  It keeps the decode's
    inputs alive, because result() decodes again when an image overflowed the capacity: the
    caller leaves them unchanged until result() returns."""

    def __init__(self, eng, b, slot_i, inputs, block):
        self._eng, self._b, self._slot_i, self._inputs = eng, b, slot_i, inputs
        self._cifdet, self._decode = inputs[0], b.decodes[slot_i]
        self._block, self._result = block, None

    @property
    def done_event(self):
        return self._block.done

    def wait(self):
        """Wait for the pack: (per-image counts int64, the decode's status words int32)."""
        self._block.wait()
        return self._block.counts().astype(np.int64), self._block.status()

    def result(self):
        """(DET_DTYPE records of all images, per-image offsets) of a complete decode: waits
        for the pack; where an image overflowed, decodes again at doubled capacity (PPError
        once the capacity is K * cells and still overflows, as CifDet.decode_device); packs
        again into a larger block when the batch outgrew this one."""
        if self._result is not None:
            return self._result
        counts, status = self.wait()
        b, eng = self._b, self._eng
        cifdet, batch, config = self._inputs
        if (status & PP_ST_ANN_OVERFLOW).any():
            if b.cap >= b.bound:
                raise PPError('CifDet: detection capacity overflow')
            cap = min(b.bound, 2 * b.cap)
            LOG.info('detection capacity overflow, retrying with %d per image', cap)
            again = eng.decode_async(cifdet, batch, cap, config)
        else:
            offsets = offsets_of(counts)
            total = int(offsets[-1])
            if total <= self._block.est:
                self._result = (self._block.records(total, DET_DTYPE), offsets)
                self._inputs = None
                return self._result
            eng.pack_cap = max(eng.pack_cap, 2 * total)  # outgrew the block
            if b.decodes[self._slot_i] == self._decode:  # the slot still holds the records
                # pylint: disable=protected-access
                again = eng._pack(b, self._slot_i, self._inputs, eng.pack_cap)
            else:  # rewritten by a later decode: once more from the inputs
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
