"""numpy restatement of s2f_firing_log_append (include/s2f.h "firing log"): the ring, the head, the silent streaks, the latch of the
first dead neuron and the clearing of the counters -- written from the header's words, one neuron at a time, for the tests of the
kernel and of the op's CPU route."""
import numpy as np

U64 = (1 << 64) - 1


def new_state(n, window, silent=None):
    """-> (ring int64 [window, n, 2], silent int32 [n], head int64 [4] = {0, -1, 0, 0})"""
    s = np.zeros(n, np.int32) if silent is None else np.asarray(silent, np.int32).copy()
    return np.zeros((window, n, 2), np.int64), s, np.array([0, -1, 0, 0], np.int64)


def append(counters, ring, silent, head, patience):
    """One launch, in place.  counters: uint64 or int64 [n, slots, 2] (the sums wrap modulo 2^64, as 64-bit adds do)."""
    n, window = counters.shape[0], ring.shape[0]
    assert ring.shape == (window, n, 2) and silent.shape == (n,) and head.shape == (4,) and patience >= 1
    row = int(head[0])
    latch = int(head[1]) & U64          # -1: the largest unsigned value, "none"
    for i in range(n):
        total = [int(counters[i, :, k].astype(np.uint64).sum(dtype=np.uint64)) for k in (0, 1)]          # (wraps modulo 2^64)
        ring[row % window, i] = [t - (1 << 64) if t >> 63 else t for t in total]
        counters[i] = 0
        if silent[i] == -1:
            continue
        silent[i] = silent[i] + 1 if total[0] == 0 else 0
        if silent[i] == patience:
            latch = min(latch, (row << 32) + i)
    head[1] = latch - (1 << 64) if latch >> 63 else latch
    head[0] = row + 1
    assert head[2] == 0
    return ring


def first_dead(head):
    """head -> (row, neuron index) or None"""
    return None if int(head[1]) < 0 else (int(head[1]) >> 32, int(head[1]) & 0xffffffff)
