"""engine/handover.py without a device: the pinned block's head arithmetic and views, the
offset and gather-index helpers, and the two output slots with the streams stubbed out."""
import numpy as np
import pytest

from openpifpaf_amd.engine import handover


@pytest.mark.parametrize('n, words, want', [(1, 3, 256), (21, 3, 256), (22, 3, 512),
                                            (32, 2, 256), (33, 2, 512)])
def test_head_size(n, words, want):
    # 12 * 21 = 252 -> 256, 12 * 22 = 264 -> 512, 8 * 32 = 256 -> 256, 8 * 33 = 264 -> 512
    assert handover.head_size(n, words) == want


def test_block_views_land_on_their_bytes():
    n, est, dtype = 5, 3, np.dtype([('a', np.int32), ('b', np.float32)])
    raw = np.zeros(handover.head_size(n, 3) + est * dtype.itemsize, np.uint8)
    block = handover.PinnedBlock(n, 3, est, dtype.itemsize, host=raw)
    assert block.head == 256 and block.est == est
    block.counts()[:] = 0x01010101
    assert raw[:4 * n].tolist() == [1] * (4 * n) and not raw[4 * n:].any()
    block.status()[:] = 0x02020202
    assert raw[4 * n:8 * n].tolist() == [2] * (4 * n) and not raw[8 * n:].any()
    block.flags()[:] = 0x03030303
    assert raw[8 * n:12 * n].tolist() == [3] * (4 * n) and not raw[12 * n:].any()
    for view in (block.counts(), block.status(), block.flags()):
        assert view.dtype == np.int32 and view.shape == (n,)
    recs = block.records(2, dtype)
    assert recs.dtype == dtype and recs.shape == (2,)
    recs['a'] = -1
    assert raw[256:260].tolist() == [255] * 4 and raw[264:268].tolist() == [255] * 4
    assert not raw[12 * n:256].any() and not raw[256 + 2 * dtype.itemsize:].any()
    base = block.ptr(0).value
    assert base == raw.ctypes.data
    assert [block.ptr(i).value - base for i in (1, 2)] == [4 * n, 8 * n]
    assert block.records_ptr().value - base == 256
    # a two-word head (detection): the records start behind counts and status
    assert handover.PinnedBlock(33, 2, 1, 32, host=np.zeros(512 + 32, np.uint8)).head == 512


def test_offsets_of():
    for counts, want in (([], [0]), ([0, 3, 0, 2], [0, 0, 3, 3, 5])):
        for arg in (counts, np.array(counts, np.int32), np.array(counts, np.int64)):
            got = handover.offsets_of(arg)
            assert got.dtype == np.int64 and got.tolist() == want


def test_gather_index():
    got = handover.gather_index([0, 3, 0, 2], cap=4)
    assert got.dtype == np.int64 and got.tolist() == [4, 5, 6, 12, 13]
    got = handover.gather_index(np.array([0, 3, 0, 2], np.int32), cap=4)
    assert got.dtype == np.int64 and got.tolist() == [4, 5, 6, 12, 13]
    for counts in ([0, 0, 0], []):
        got = handover.gather_index(counts, cap=4)
        assert got.dtype == np.int64 and got.shape == (0,)


class _Stream:
    def __init__(self):
        self.waited = []

    def wait_event(self, event):
        self.waited.append(event)


def test_output_slots(monkeypatch):
    stream = _Stream()
    monkeypatch.setattr(handover.torch.cuda, 'current_stream', lambda: stream)
    made = []

    def make():
        made.append(tuple('{}{}'.format(name, len(made)) for name in ('records', 'counts', 'status')))
        return made[-1]

    slots = handover.OutputSlots(make)
    assert len(made) == 2 and slots.slot(0) == made[0] and slots.slot(1) == made[1]
    assert slots.current == 0 and slots.decodes == [0, 0]
    assert (slots.records, slots.counts, slots.status) == made[0]
    slots.next_slot()
    assert slots.current == 1 and slots.decodes == [0, 1] and stream.waited == []
    assert (slots.records, slots.counts, slots.status) == made[1]
    slots.released_by(1, 'packed-1')
    slots.released_by(0, 'packed-0')
    slots.next_slot()  # slot 0: waits for its pack, and only for it
    assert slots.current == 0 and slots.decodes == [1, 1] and stream.waited == ['packed-0']
    slots.next_slot()
    assert slots.current == 1 and slots.decodes == [1, 2]
    assert stream.waited == ['packed-0', 'packed-1']
    slots.next_slot()  # the release events were cleared: nothing more to wait for
    slots.next_slot()
    assert slots.decodes == [2, 3] and stream.waited == ['packed-0', 'packed-1']
