"""CPU: the gradient log without a GPU -- the span table, the two ABI rows and their argument errors, GradRead's arithmetic and ring
unwrapping from a hand-written host buffer, the restatement's latches (tests/gradlog_ref.py), and LoggerHook's grad/ keys, grad.jsonl,
its one warning and its window check, driven by a fake step and a fake log (runner.py)."""
import json
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gradlog_ref as R  # noqa: E402

P = 1 << 20          # a 16-byte aligned dummy address: never dereferenced on the host
SPAN = 16384


# ---------------------------------------------------------------------------------------------------- the span table
def slots_of(sizes):
    off, rows = 0, []
    for n in sizes:
        rows.append((P, off, n))
        off += (n + 3) // 4 * 4
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 3)


@pytest.mark.parametrize("sizes,want", [
    ((1,), [(0, 0)]),
    ((SPAN,), [(0, 0)]),
    ((SPAN + 1,), [(0, 0), (0, SPAN)]),
    ((5, 2 * SPAN + 7, 0, SPAN, 1), [(0, 0), (1, 0), (1, SPAN), (1, 2 * SPAN), (3, 0), (4, 0)]),
])
def test_span_table(sizes, want):
    from spike2former_amd import _lib, ops
    assert _lib.lib.s2f_grad_log_span_elems() == SPAN
    spans = ops.grad_log_table(slots_of(sizes))
    assert spans.dtype == torch.int32 and spans.is_contiguous() and spans.tolist() == [list(w) for w in want]


def test_span_table_refuses_what_is_no_slot_table():
    from spike2former_amd import ops
    with pytest.raises(ValueError):
        ops.grad_log_table(torch.zeros(3, 2, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.grad_log_table(slots_of((4,)).to(torch.int32))
    with pytest.raises(ValueError, match="no parameter"):
        ops.grad_log_table(slots_of((0, 0)))


# ---------------------------------------------------------------------------------------------------- ABI
def test_abi_rows_and_argument_errors():
    from spike2former_amd import _lib
    lib = _lib.lib
    assert lib.s2f_version() >= 50
    assert len(_lib.SIGNATURES["s2f_grad_log_partials"][1]) == 11 and len(_lib.SIGNATURES["s2f_grad_log_rows"][1]) == 10
    part = lib.s2f_grad_log_partials
    good = [P, P, P, 3, P, P, P, P, 1e-8, P, None]
    for k in (0, 1, 2, 4, 5, 6, 7, 9):
        args = list(good)
        args[k] = None
        assert part(*args) == -1 and b"s2f_grad_log_partials: null" in lib.s2f_last_error()
    for n in (0, -2):
        args = list(good)
        args[3] = n
        assert part(*args) == -1 and b"n " in lib.s2f_last_error()
    for k, d in ((4, 4), (5, 8), (6, 4), (9, 4), (0, 4)):          # g, m, v 16-byte; partials, slots 8-byte
        args = list(good)
        args[k] = P + d
        assert part(*args) == -2 and b"aligned" in lib.s2f_last_error()
    rows = lib.s2f_grad_log_rows
    good = [P, 3, P, 2, P, 4, P, 1, P, None]
    for k in (0, 2, 4, 6, 8):
        args = list(good)
        args[k] = None
        assert rows(*args) == -1 and b"s2f_grad_log_rows: null" in lib.s2f_last_error()
    for k, word in ((1, b"n "), (3, b"n "), (5, b"window"), (7, b"patience")):
        for bad in (0, -3):
            args = list(good)
            args[k] = bad
            assert rows(*args) == -1 and word in lib.s2f_last_error()
    for k, d in ((2, 4), (4, 4), (8, 4), (6, 2)):          # partials, ring, head 8-byte; streak 4-byte
        args = list(good)
        args[k] = P + d
        assert rows(*args) == -2 and b"aligned" in lib.s2f_last_error()


def test_op_checks_its_tensors_and_has_no_cpu_route():
    from spike2former_amd import ops
    n, window = 2, 3
    slots = slots_of((5, 9))
    spans = ops.grad_log_table(slots)
    flat = torch.zeros(20)
    good = dict(slots=slots, spans=spans, hyper=torch.zeros(n, 2), state=torch.zeros(8), flat=flat, exp_avg=flat.clone(),
                exp_avg_sq=flat.clone(), partials=torch.zeros(2, 8, dtype=torch.int64),
                ring=torch.zeros(window, n, 8, dtype=torch.int64), streak=torch.zeros(n, 2, dtype=torch.int32),
                head=torch.zeros(4, dtype=torch.int64), eps=1e-8, patience=2)
    with pytest.raises(RuntimeError, match="no CPU route"):
        ops.grad_log_append(**good)
    for key, bad in (("slots", slots.to(torch.int32)), ("spans", spans.to(torch.int64)), ("hyper", torch.zeros(n + 1, 2)),
                     ("state", torch.zeros(4)), ("exp_avg", torch.zeros(19)), ("exp_avg_sq", flat.double()),
                     ("partials", torch.zeros(3, 8, dtype=torch.int64)), ("ring", torch.zeros(window, n, 2, dtype=torch.int64)),
                     ("ring", torch.zeros(window, 8, n, dtype=torch.int64).transpose(1, 2)),
                     ("streak", torch.zeros(n, dtype=torch.int32)), ("head", torch.zeros(2, dtype=torch.int64)), ("patience", 0)):
        with pytest.raises(ValueError):
            ops.grad_log_append(**{**good, key: bad})


# ---------------------------------------------------------------------------------------------------- GradRead
def hand_buffer(n, window, rows, streak=None, head1=-1, head3=-1):
    """the log's allocation after `rows` ([(floats [n, 4], ints [n, 4])], in order) were appended"""
    buf = np.zeros(4 + n + window * n * 8, np.int64)
    ring = buf[4 + n:].reshape(window, n, 8)
    for r, (floats, ints) in enumerate(rows):
        ring[r % window, :, :4] = np.asarray(floats, np.float64).view(np.int64)
        ring[r % window, :, 4:] = ints
    buf[0], buf[1], buf[3] = len(rows), head1, head3
    if streak is not None:
        buf[4:4 + n] = np.asarray(streak, np.int32).reshape(n, 2).view(np.int64).reshape(n)
    return buf


def test_grad_read_arithmetic_and_unwrapping():
    from spike2former_amd import GradRead
    names = ["a.weight", "a.bias", "b.weight"]
    rows = [([[9.0 * (r + 1), 16.0, 4.0, 2.5], [0.0, 0.0, 1.0, 0.0], [16.0, 100.0, 1e-4, 3.0]],
             [[1, 0, 0, 10], [4, 0, 2, 4], [0, r, 0, 7]]) for r in range(5)]
    buf = hand_buffer(3, 3, rows, streak=[[0, 0], [5, 0], [0, 4]], head1=(1 << 32) | 1, head3=(1 << 32) | 2)
    read = GradRead.from_buffer(buf, names, window=3)
    assert read.names == names and read.count == 5 and read.cols.shape == (3, 3, 8) and read.cols.dtype == np.int64
    assert read.grad_norm[:, 0].tolist() == [np.sqrt(9.0 * 3), np.sqrt(9.0 * 4), np.sqrt(9.0 * 5)]          # rows 2, 3, 4, oldest first
    assert read.weight_norm[0].tolist() == [4.0, 0.0, 10.0] and read.grad_max[0].tolist() == [2.5, 0.0, 3.0]
    assert read.update_ratio[0].tolist() == [0.5, 0.0, np.sqrt(1e-4 / 100.0)]          # 0 where the weight's norm is 0
    assert read.zero_share[0].tolist() == [0.1, 1.0, 0.0] and read.numel[0].tolist() == [10, 4, 7]
    assert read.nonfinite[:, 2].tolist() == [[2, 0], [3, 0], [4, 0]] and read.nonfinite[0, 1].tolist() == [0, 2]
    assert read.total_grad_norm.tolist() == [np.sqrt(9.0 * (r + 1) + 0.0 + 16.0) for r in (2, 3, 4)]
    assert read.streak.tolist() == [[0, 0], [5, 0], [0, 4]]
    assert read.first_stalled == (1, "a.bias") and read.first_nonfinite == (1, "b.weight")
    # only the rows since the last read; never more than the window
    assert GradRead.from_buffer(buf, names, 3, last=4).cols.shape == (1, 3, 8)
    assert GradRead.from_buffer(buf, names, 3, last=4).grad_norm[0, 0] == np.sqrt(45.0)
    assert GradRead.from_buffer(buf, names, 3, last=5).cols.shape == (0, 3, 8)
    assert GradRead.from_buffer(buf, names, 3, last=1).cols.shape == (3, 3, 8)
    empty = GradRead.from_buffer(hand_buffer(3, 3, []), names, 3)
    assert empty.count == 0 and empty.grad_norm.shape == (0, 3) and empty.total_grad_norm.shape == (0,)
    assert empty.first_stalled is None and empty.first_nonfinite is None
    # before the ring wraps
    two = GradRead.from_buffer(hand_buffer(3, 3, rows[:2]), names, 3)
    assert two.cols.shape == (2, 3, 8) and two.grad_norm[:, 0].tolist() == [3.0, np.sqrt(18.0)]


def test_restatement_rows_streaks_and_latches():
    g = np.array([0.0, -3.0, np.nan, 2.0, np.inf], np.float32)
    p = np.array([1.0, np.inf, 2.0, 0.0, 0.0], np.float32)
    m = np.array([1.0, 1.0, 1.0, 0.0, -2.0], np.float32)
    v = np.array([4.0, 0.0, 1.0, 1.0, 1.0], np.float32)
    floats, ints = R.row(g, p, m, v, lr=0.5, bc1=0.5, bc2s=1.0, eps=1.0)
    third = float(np.float32(1.0) / np.float32(3.0))          # step_size 1, denom = sqrt(v) + 1 = [3, 1, 2, 2, 2]
    assert R.update(m, v, 0.5, 0.5, 1.0, 1.0).tolist() == [third, 1.0, 0.5, 0.0, -1.0]
    assert floats.tolist() == [13.0, 5.0, third * third + 2.25, 3.0]
    assert ints.tolist() == [1, 2, 1, 5]
    assert R.row(g, p, m, v, lr=-1.0, bc1=0.5, bc2s=1.0, eps=1.0)[0][2] == 0.0
    ring, streak, head = R.new_state(3, 2)
    zero, live, bad = (np.zeros(4), np.array([4, 0, 0, 4])), (np.ones(4), np.array([0, 0, 0, 4])), (np.ones(4), np.array([0, 1, 0, 4]))
    R.append([live, zero, zero], ring, streak, head, 2)
    assert R.event(head[1]) is None and R.event(head[3]) is None and streak[:, 0].tolist() == [0, 1, 1]
    R.append([live, zero, zero], ring, streak, head, 2)
    assert R.event(head[1]) == (1, 1)          # two parameters in one row: the lower one
    R.append([bad, live, bad], ring, streak, head, 2)
    assert R.event(head[3]) == (2, 0) and streak.tolist() == [[0, 1], [0, 0], [0, 1]]
    R.append([zero, zero, bad], ring, streak, head, 2)
    R.append([zero, zero, live], ring, streak, head, 2)
    assert R.event(head[1]) == (1, 1) and R.event(head[3]) == (2, 0) and head[0] == 5 and streak.tolist() == [[2, 0], [2, 0], [0, 0]]


# ---------------------------------------------------------------------------------------------------- LoggerHook
class FakeAugment:
    rng = np.random.default_rng(0)

    def __call__(self, images, segs, out=None):
        pass


class FakeGradLog:
    """what the loop sees of a GradLog: scripted rows, one per iteration, read since the last read"""
    prefix = "grad"

    def __init__(self, names, script, window, patience, stalled=None):
        self.names, self.script, self.window, self.patience, self.base = names, script, window, patience, 0
        self.count = self._last = self.reads = 0
        self.stalled = stalled          # (row, index): latched once `count` has passed the row

    def append(self):
        self.count += 1

    def read(self, consume=True):
        from spike2former_amd import GradRead
        n = len(self.names)
        streak = np.zeros((n, 2), np.int32)
        for r in range(self.count):
            ints = np.asarray(self.script[r][1])
            streak[:, 0] = np.where(ints[:, 0] == ints[:, 3], streak[:, 0] + 1, 0)
        head1 = -1 if self.stalled is None or self.count <= self.stalled[0] else (self.stalled[0] << 32) | self.stalled[1]
        read = GradRead.from_buffer(hand_buffer(n, self.window, self.script[:self.count], streak, head1), self.names, self.window,
                                    self._last)
        if consume:
            self._last = read.count
            self.reads += 1
        return read

    def rebase(self, start, unit=1):
        self.base = start // unit - self.count

    def report(self, *args):          # (GradLog's own, over this fake's read)
        from spike2former_amd import GradLog
        return GradLog.report(self, *args)


class FakeStep:
    def __init__(self, model, log, grad_log, nan_at=None):
        self.model, self.log, self.grad_log, self.calls, self.nan_at = model, log, grad_log, 0, nan_at
        self.static_in, self.static_seg = torch.zeros(1), torch.zeros(1, dtype=torch.uint8)
        self.vals = {k: torch.zeros(()) for k in ("loss", "grad_norm", "clip_coef")}
        log.bind(self.vals)

    def __call__(self):
        self.vals["loss"].fill_(float("nan") if self.calls == self.nan_at else 1.0 + self.calls)
        self.log.append()
        self.grad_log.append()
        self.calls += 1


NAMES = ["stem.weight", "block.weight", "block.bias", "head.weight"]


def script_of(iters):
    """per iteration (floats [4, 4], ints [4, 4]): block.bias gets an all-zero gradient from iteration 3 on; head.weight holds most of
    sum g^2; stem.weight moves furthest relative to its size"""
    out = []
    for it in range(iters):
        dead = it >= 2
        floats = [[1.0 + it, 4.0, 0.04, 0.5], [4.0, 100.0, 0.01, 1.0], [0.0 if dead else 0.25, 1.0, 1e-6, 0.0 if dead else 0.5],
                  [100.0 * (it + 1), 400.0, 0.04, 9.0]]
        ints = [[2, 0, 0, 10], [0, 0, 0, 20], [6 if dead else 1, 0, 0, 6], [4, 0, 0, 64]]
        out.append((floats, ints))
    return out


def make_loop(tmp_path, iters, interval, window=4, patience=3, stalled=None, nan_at=None):
    import spike2former_amd as s2f
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.train import FlatAdamW, LinearThenPoly
    model = torch.nn.Sequential(torch.nn.Linear(2, 2))
    opt = FlatAdamW(model, FlatGradAllReduce(model.parameters(), 1), lr=0.01)
    assert opt.grad_log is None
    opt.grad_log = FakeGradLog(NAMES, script_of(iters), window, patience, stalled)
    sched = LinearThenPoly(opt, warmup=2, total=50, start_factor=0.1)
    step = FakeStep(model, s2f.TrainLog(window=8, device="cpu", capacity=4), opt.grad_log, nan_at)
    loop = s2f.TrainLoop(step, opt, sched, FakeAugment(), [(None, None)], max_iters=iters,
                         hooks=[dict(type="LoggerHook", interval=interval, window_size=2)], work_dir=str(tmp_path))
    assert loop.grad_log is opt.grad_log
    return loop


def test_logger_hook_grad_keys_lines_and_one_warning(tmp_path, caplog):
    loop = make_loop(tmp_path, 10, interval=4, stalled=(4, 2))
    with caplog.at_level(logging.INFO, logger="spike2former_amd"):
        loop.run()
    with open(tmp_path / "vis_data" / "scalars.json") as f:
        lines = [json.loads(line) for line in f]
    with open(tmp_path / "vis_data" / "grad.jsonl") as f:
        grad = [json.loads(line) for line in f]
    assert [r["iter"] for r in lines] == [4, 8, 10] and [r["iter"] for r in grad] == [4, 8, 10] and [r["rows"] for r in grad] == [4, 4, 2]
    assert loop.grad_log.reads == 3          # ONE read per log line
    script, first = script_of(10), 0
    for rec, gr in zip(lines, grad):
        fl = np.array([script[it][0] for it in range(first, rec["iter"])], float)          # [rows, 4, 4]
        it_ = np.array([script[it][1] for it in range(first, rec["iter"])], float)
        first = rec["iter"]
        assert set(rec) >= {"grad/min", "grad/min_name", "grad/max_share", "grad/max_name", "grad/update_ratio_max",
                            "grad/update_ratio_max_name", "grad/zero_share", "grad/stalled", "loss", "lr", "iter"}
        norm = np.sqrt(fl[:, :, 0]).mean(0)
        ratio = np.sqrt(fl[:, :, 2] / fl[:, :, 1]).mean(0)
        share = fl[:, :, 0].sum(0) / fl[:, :, 0].sum()
        assert rec["grad/min_name"] == "block.bias" and rec["grad/min"] == pytest.approx(norm[2], rel=1e-12)
        assert rec["grad/max_name"] == "head.weight" and rec["grad/max_share"] == pytest.approx(share[3], rel=1e-12)
        assert rec["grad/update_ratio_max_name"] == "stem.weight" and rec["grad/update_ratio_max"] == pytest.approx(ratio[0], rel=1e-12)
        assert rec["grad/zero_share"] == pytest.approx(it_[:, :, 0].sum() / it_[:, :, 3].sum(), rel=1e-12)
        assert set(gr) == {"iter", "rows", "grad_norm", "weight_norm", "update_ratio", "grad_max", "zero_share"}
        for key in ("grad_norm", "weight_norm", "update_ratio", "grad_max", "zero_share"):
            assert list(gr[key]) == NAMES
        for i, name in enumerate(NAMES):
            assert gr["grad_norm"][name] == pytest.approx(norm[i], rel=1e-12)
            assert gr["weight_norm"][name] == pytest.approx(np.sqrt(fl[:, i, 1]).mean(), rel=1e-12)
            assert gr["update_ratio"][name] == pytest.approx(ratio[i], rel=1e-12)
            assert gr["grad_max"][name] == fl[:, i, 3].max()
            assert gr["zero_share"][name] == pytest.approx((it_[:, i, 0] / it_[:, i, 3]).mean(), rel=1e-12)
    assert [r["grad/stalled"] for r in lines] == [1, 1, 1]
    warnings = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1 and "block.bias" in warnings[0].message and "iteration 5" in warnings[0].message
    assert sum("Iter(train)" in r.message and "grad/max_share" in r.message for r in caplog.records) == 3


def test_logger_hook_refuses_a_ring_shorter_than_the_interval(tmp_path):
    loop = make_loop(tmp_path, 6, interval=5, window=4)
    with pytest.raises(ValueError, match="GradLog of 4 rows"):
        loop.run()


def test_check_finite_names_the_tensor(tmp_path):
    loop = make_loop(tmp_path, 6, interval=2, nan_at=2)          # the loss of iteration 3 is NaN
    gl = loop.grad_log
    real = gl.read
    gl.read = lambda consume=True: real(consume)._replace(first_nonfinite=(2, "block.weight") if gl.count >= 3 else None)
    with pytest.raises(FloatingPointError, match=r"iteration 3.*first non-finite gradient is in block\.weight, iteration 3"):
        loop.run()
