"""CPU: the device ring's host side (spike2former_amd/devring.py) -- the unwrap against a ring written by hand, the latch decoder,
`rebase`, TrainLog on the ring's 8-byte-word layout, and graph.step_tail's table together with the two classes that derive from it
(runner.TrainLoop and graph._Captured, on fakes at a patched world size)."""
import types

import numpy as np
import pytest
import torch


def ring_cls():
    from spike2former_amd.devring import DeviceRing, unwrap

    class Ring(DeviceRing):
        """two state words and rows of `n` words; rows and head are written by hand (what an appending kernel does)"""
        HEAD = (0, -1, 0, -1)

        def __init__(self, window, n):
            self.window, self.n, self._last = window, n, 0
            self.state, ring = self._allocate(2, window * n, "cpu")
            self.ring = ring.view(window, n)
            self.clear()

        def append(self, row):
            count = int(self.head[0])
            self.ring[count % self.window] = torch.tensor(row, dtype=torch.int64)
            self.head[0] = count + 1

        def read(self, consume=True):          # (GradLog's rule: the rows since the last read)
            words = self.fetch()
            rows = unwrap(words[4 + 2:].reshape(self.window, self.n), int(words[0]), self.window, self._last)
            if consume:
                self._last = int(words[0])
            return rows
    return Ring


@pytest.mark.parametrize("window", [1, 3])
def test_unwrap_against_a_ring_written_by_hand(window):
    from spike2former_amd.devring import unwrap
    Ring = ring_cls()
    for count in (0, 1, window - 1, window, window + 1, 3 * window + 2):
        log = Ring(window, 2)
        assert log.head.data_ptr() == log._buf.data_ptr() and log.ring.data_ptr() == log._buf.data_ptr() + 8 * (4 + 2)
        assert log.head.tolist() == [0, -1, 0, -1] and log.head.dtype == torch.int64 and log.base == 0
        hand = np.zeros((window, 2), np.int64)
        for r in range(count):          # row r lands in ring[r % window]
            log.append([r, -10 * r])
            hand[r % window] = [r, -10 * r]
        words = log.fetch()
        assert words.dtype == np.int64 and words.shape == (4 + 2 + window * 2,) and words[:4].tolist() == [count, -1, 0, -1]
        assert np.array_equal(words[6:].reshape(window, 2), hand)
        for last in (0, count - 1, count, count - window - 1):
            want = [r for r in range(count) if r >= last and r >= count - window]          # oldest first
            for got in (unwrap(hand, count, window, last), unwrap(words[6:].reshape(window, 2), count, window, last)):
                assert got.dtype == np.int64 and got.shape == (len(want), 2)
                assert got[:, 0].tolist() == want and got[:, 1].tolist() == [-10 * r for r in want]
            got[...] = 77          # a copy: the ring is not written through it
            assert np.array_equal(words[6:].reshape(window, 2), hand)
        assert unwrap(hand, count, window).shape == (min(count, window), 2)          # last = 0: the whole window
        log.state.fill_(5)
        log.clear()
        assert log.head.tolist() == [0, -1, 0, -1] and int(log.ring.abs().sum()) == 0 and log.state.tolist() == [5, 5]


def test_latch_decoder():
    from spike2former_amd.devring import latch
    names = ["a", "b", "c"]
    assert latch(-1, names) is None and latch(np.int64(-1), names) is None
    assert latch(0, names) == (0, "a") and latch(np.int64(0), names) == (0, "a")
    assert latch((5 << 32) | 2, names) == (5, "c") and latch(np.int64((5 << 32) | 2), names) == (5, "c")
    big = 2 ** 31 + 7          # a row past 2^31: the row is the word's upper half, not a 32-bit quantity
    assert latch((big << 32) | 1, names) == (big, "b")
    top = 2 ** 31 - 1          # the last row whose word is not negative as an int64
    assert latch(np.int64((top << 32) | 2), names) == (top, "c")
    row, name = latch(np.array([(7 << 32) | 1], np.int64)[0], names)
    assert type(row) is int and (row, name) == (7, "b")


def test_rebase_consumes_nothing():
    log = ring_cls()(4, 1)
    for r in range(3):
        log.append([r])
    log.rebase(10)          # three rows were appended before the run: row 0 is iteration 8, the next row iteration 11
    assert log.base == 7 and log._last == 0
    assert log.read()[:, 0].tolist() == [0, 1, 2] and log.read().shape == (0, 1)
    log.rebase(10)
    assert log.base == 7
    log.append([3])
    log.rebase(12, unit=3)          # rows that count updates of 3 iterations: 12 iterations are 4 updates, 4 rows are in
    assert log.base == 0 and log.read()[:, 0].tolist() == [3]
    log.rebase(14, unit=3)
    assert log.base == 0


def test_rebase_of_a_grad_log_leaves_its_rows_to_the_next_read():
    import spike2former_amd as s2f
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.train import FlatAdamW
    model = torch.nn.Linear(2, 2)
    opt = FlatAdamW(model, FlatGradAllReduce(model.parameters(), 1), lr=0.01)
    gl = s2f.GradLog(opt, window=3, patience=2)
    assert gl.head.tolist() == [0, -1, 0, -1] and gl.streak.shape == (2, 2) and gl.ring.shape == (3, 2, 8)
    assert gl.ring.data_ptr() == gl._buf.data_ptr() + 8 * (4 + 2)
    for r in range(2):          # two rows, by hand (the append is two HIP launches)
        gl.ring[r, :, 7] = r + 1
    gl.head[0] = 2
    gl.rebase(9, unit=3)
    assert gl.base == 1
    read = gl.read()
    assert read.count == 2 and read.numel.tolist() == [[1, 1], [2, 2]] and gl.read().cols.shape == (0, 2, 8)
    gl.clear()
    assert gl.head.tolist() == [0, -1, 0, -1] and int(gl.ring.abs().sum()) == 0 and gl.read().count == 0


def test_train_log_on_the_ring_layout():
    import spike2former_amd as s2f
    log = s2f.TrainLog(window=3, device="cpu", capacity=3)          # nine fp32 cells: five 8-byte words, the last half used
    assert log.head.dtype == torch.int64 and tuple(log.head.shape) == (4,) and log.head.tolist() == [0, -1, 0, 0]
    assert log._buf.dtype == torch.int64 and log._buf.numel() == 4 + 5
    assert log.ring.dtype == torch.float32 and tuple(log.ring.shape) == (3, 3) and log.ring.data_ptr() == log._buf.data_ptr() + 32
    empty = log.read()
    assert empty.names == [] and empty.rows.shape == (0, 0) and empty.count == 0 and empty.first_nonfinite is None
    vals = {"loss": torch.zeros(()), "grad_norm": torch.zeros(())}
    log.bind(vals)
    assert log.read().rows.shape == (0, 2) and log.read().rows.dtype == np.float32
    for it in range(5):
        vals["loss"].fill_(float("nan") if it == 1 else 0.5 + it)
        vals["grad_norm"].fill_(0.25 * it)
        log.append()
    read = log.read()
    assert read.names == ["loss", "grad_norm"] and read.count == 5 and read.first_nonfinite == 1
    assert read.rows.dtype == np.float32 and read.rows.flags["C_CONTIGUOUS"]
    assert read.rows.tolist() == [[2.5, 0.5], [3.5, 0.75], [4.5, 1.0]]          # iterations 3, 4, 5, oldest first
    assert log.head.tolist() == [5, 1, 0, 0]
    log.rebase(5)
    assert log.base == 0 and log.read().rows.tolist() == read.rows.tolist()


# update, row by (optimizer handed to the step, accumulating, world)
TABLE = {(True, False, 1): ("graph", "graph"), (True, False, 2): ("graph", "caller"),
         (False, False, 1): ("caller", "graph"), (False, False, 2): ("caller", "caller"),
         (True, True, 1): ("call", "call"), (True, True, 2): ("caller", "caller")}


def test_step_tail_is_the_table():
    from spike2former_amd.graph import step_tail
    for (in_step, accumulating, world), want in TABLE.items():
        assert step_tail(in_step, accumulating, world) == want
        if world > 1:
            assert step_tail(in_step, accumulating, 8) == want


class FakeLog:
    window = 4

    def __init__(self):
        self.calls = []

    def declare(self, names):
        self.calls.append("declare")

    def append(self):
        self.calls.append("append")

    def bind(self, terms):
        self.calls.append("bind")


class FakeStep:
    """what runner.TrainLoop sees of a step before it runs"""

    def __init__(self, model, optimizer, log):
        self.model, self.log = model, log
        self.log_terms = {"loss": torch.zeros(1)}
        self.static_in, self.static_seg = torch.zeros(2, 1), torch.zeros(1, dtype=torch.uint8)
        if optimizer is not None:
            self.optimizer = optimizer
        else:
            self.red = object()          # (a step without the optimizer leaves reduce and update to the loop)


@pytest.mark.parametrize("case", list(TABLE))
def test_loop_and_step_derive_from_the_table(case, monkeypatch):
    import spike2former_amd as s2f
    from spike2former_amd import graph, runner
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.train import FlatAdamW, LinearThenPoly
    (in_step, accumulating, world), (update, row) = case, TABLE[case]
    monkeypatch.setattr(runner, "_rank_world", lambda: (0, world))
    monkeypatch.setattr(graph, "_world_size", lambda: world)
    model = torch.nn.Sequential(torch.nn.Linear(3, 5))
    opt = FlatAdamW(model, FlatGradAllReduce(model.parameters(), 1), lr=0.01, accumulative_counts=3 if accumulating else 1)
    assert (opt.accum is not None) == accumulating
    # the loop
    log = FakeLog()
    step = FakeStep(model, opt if in_step else None, log)
    aug = types.SimpleNamespace(rng=np.random.default_rng(0))
    loop = s2f.TrainLoop(step, opt, LinearThenPoly(opt, warmup=2, total=50, start_factor=0.1), aug, [(None, None)], max_iters=6)
    assert loop.world == world
    assert loop.eager_update == (update == "caller") and loop.eager_append == (row == "caller")
    assert log.calls == (["bind"] if row == "caller" else [])          # the loop binds the row it appends
    step.log_captured = row == "graph"          # what a captured step says of itself agrees
    again = s2f.TrainLoop(step, opt, loop.scheduler, aug, [(None, None)], max_iters=6)
    assert (again.eager_update, again.eager_append) == (loop.eager_update, loop.eager_append)
    # the step
    cap = graph._Captured()
    cap.optimizer, cap.log = (opt if in_step else None), FakeLog()
    assert cap._update_in_graph() == (update == "graph")
    cap._record_log({"loss": torch.zeros(1)})
    assert cap.log_captured == (row == "graph") and cap.log.calls == (["declare", "append"] if row == "graph" else [])
    assert set(cap.log_terms) == {"loss"} | ({"grad_norm", "clip_coef"} if in_step else set()) \
        | ({"grad_sq_micro", "grad_sq_accum"} if accumulating else set())
    cap._after_capture()
    assert cap.log.calls[-1:] == ([] if row == "caller" else ["bind"])
