"""What both decoders' engines hand their records over with: the two output slots a decode
writes in turn, the pinned host block a pack kernel writes, and the offset arithmetic of
packed records."""
import ctypes

import numpy as np
import torch


def offsets_of(counts):
    """Per-image offsets (n + 1, int64) of records packed image after image."""
    return np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])


def gather_index(counts, cap):
    """Rows (int64) of the images' first counts[i] records in an (n * cap)-row table, image
    after image: record r of image i is row i * cap + r."""
    counts = np.asarray(counts, np.int64)
    offsets = offsets_of(counts)
    return np.arange(int(offsets[-1]), dtype=np.int64) + np.repeat(
        np.arange(len(counts), dtype=np.int64) * cap - offsets[:-1], counts)


def head_size(n, words):
    """Bytes of a block's head: `words` int32 per image, rounded up to 256."""
    return -(-4 * words * n // 256) * 256


class OutputSlots:
    """Two slots of (records, counts, status) device tensors, `make()` allocates one: a decode
    writes the slot after the previous one, so decode i's records can still be packed while
    decode i + 1 runs.  Keeps the current slot and, per slot, the event after which its records
    were packed and the decodes written into it so far (by which a pending fetch tells whether
    the slot still holds its records)."""

    def __init__(self, make):
        self._slots = (make(), make())
        self._cur = 0
        self._free = [None, None]
        self.decodes = [0, 0]

    records = property(lambda self: self._slots[self._cur][0])
    counts = property(lambda self: self._slots[self._cur][1])
    status = property(lambda self: self._slots[self._cur][2])
    current = property(lambda self: self._cur)

    def slot(self, i):
        """The (records, counts, status) of slot i."""
        return self._slots[i]

    def next_slot(self):
        """Switch to the other slot; the current stream waits until that slot's previous
        records have been packed (the packs run on other streams)."""
        self._cur ^= 1
        self.decodes[self._cur] += 1
        if self._free[self._cur] is not None:
            torch.cuda.current_stream().wait_event(self._free[self._cur])
            self._free[self._cur] = None

    def released_by(self, slot, event):
        """`event` ends the pack that reads slot `slot`: its next decode waits for it."""
        self._free[slot] = event


class PinnedBlock:
    """A pinned uint8 block the device writes zero-copy: a head of `words` int32 per image
    (counts, status[, flags]; head_size bytes), then `est` records of `width` bytes.
    `records=False` leaves the record area out (they go to device memory); `host` takes an
    existing uint8 array or tensor instead of allocating.  `done`, set after the launch, is the
    event behind the last write: the block waits for it before it goes back to the host cache."""

    def __init__(self, n, words, est, width, records=True, host=None):
        self.done, self.waited = None, False
        self.n, self.est, self.head = n, est, head_size(n, words)
        self.host = torch.as_tensor(host) if host is not None else torch.empty(
            self.head + (est * width if records else 0), dtype=torch.uint8, pin_memory=True)

    def __del__(self):
        # the raw pack kernel must have finished writing the block by the time it is reused
        if not self.waited and self.done is not None:
            try:
                self.done.synchronize()
            except Exception:  # pylint: disable=broad-except
                pass

    def wait(self):
        self.done.synchronize()
        self.waited = True

    def word_bytes(self, i):
        """Head words i of every image as a uint8 tensor (for copy_ / zero_)."""
        return self.host[4 * self.n * i:4 * self.n * (i + 1)]

    def counts(self):
        return self.word_bytes(0).numpy().view(np.int32)

    def status(self):
        return self.word_bytes(1).numpy().view(np.int32)

    def flags(self):
        return self.word_bytes(2).numpy().view(np.int32)

    def records(self, total, dtype):
        return self.host[self.head:self.head + total * dtype.itemsize].numpy().view(dtype)

    def ptr(self, word=0):
        """The address of head words `word` (0 counts, 1 status, 2 flags) for a C call."""
        return ctypes.c_void_p(self.host.data_ptr() + 4 * self.n * word)

    def records_ptr(self):
        return ctypes.c_void_p(self.host.data_ptr() + self.head)
