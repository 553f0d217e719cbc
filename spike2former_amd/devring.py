"""The record a captured step keeps ON THE DEVICE and the host reads once per log line: one allocation of 8-byte words,
    head (int64 [4]) | the log's state words (streaks) | ring ([window, ...] rows)
head[0] counts the rows appended so far (row r lives in ring[r % window]); head[1] and head[3] latch the FIRST event of a kind as
`row << 32 | index` (-1: none yet); head[2] is the ticket word of the appending kernel (csrc/s2f_ring.h; 0 between launches).  An
append is the log's own launch, capturable; a read is ONE device-to-host copy of the whole allocation into a pinned mirror on the
current stream and ONE wait for it.  Neither the ring nor the state words are in a checkpoint: a resumed run starts them afresh, and
`base` names the rows that ran before row 0.  runner.TrainLog, firing.FiringLog and gradlog.GradLog are rings of this kind."""
import torch


def unwrap(ring, count, window, last=0):
    """-> the last min(count - last, window) of the `count` rows appended to `ring` (numpy [window, ...]), oldest first, as a copy"""
    k = max(0, min(count - last, window, count))
    return ring[[(count - k + i) % window for i in range(k)]]


def latch(word, names):
    """a latch word of the head -> None (-1: nothing latched) or (row, name)"""
    word = int(word)
    return None if word < 0 else (word >> 32, names[word & 0xffffffff])


class DeviceRing:
    def _allocate(self, state_words, ring_words, device):
        """-> (state, ring): the int64 views behind `head`, for the subclass to shape"""
        self.device = torch.device(device)
        self._buf = torch.zeros(4 + state_words + ring_words, dtype=torch.int64, device=self.device)
        self.head = self._buf[:4]
        self._host = torch.zeros_like(self._buf, device="cpu")
        self._event = None
        if self.device.type == "cuda":
            self._host = self._host.pin_memory()
            self._event = torch.cuda.Event()
        self.base = 0          # the rows that ran before row 0 (a resumed run)
        return self._buf[4:4 + state_words], self._buf[4 + state_words:]

    def fetch(self):
        """-> the allocation's words as numpy int64 (the host mirror: valid until the next fetch).  The one copy and the one wait."""
        if self._event is not None:
            self._host.copy_(self._buf, non_blocking=True)
            self._event.record()
            self._event.synchronize()
        else:
            self._host.copy_(self._buf)
        return self._host.numpy()

    def clear(self):
        """ring as new, the head's first words <- the subclass's `HEAD` (their initial values).  Not under capture."""
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{type(self).__name__}.clear under capture")
        self.ring.zero_()
        self.head[:len(self.HEAD)].copy_(torch.tensor(self.HEAD, dtype=torch.int64))

    def rebase(self, start, unit=1):
        """row 0 of a fresh ring belongs to iteration start + 1; `unit`: the iterations per row.  Consumes no row."""
        self.base = start // unit - int(self.fetch()[0])
