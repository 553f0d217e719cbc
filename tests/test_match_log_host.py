"""CPU: the match log without a GPU -- the numpy restatement (tests/matchlog_ref.py) on tables worked by hand, the prescribed order of
its fp64 sum, the ring / streak / latch rule, MatchLog.read() and report() over rows written into its buffer by the restatement, the
ABI rows and their argument errors, and TrainLoop + LoggerHook over a fake step (match.jsonl, the keys, ONE warning)."""
import json
import logging
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matchlog_ref as R  # noqa: E402

P = 1 << 20          # a 16-byte aligned dummy address: never dereferenced on the host
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- the restatement
def hand_case():
    """L = 2, B = 2, Q = 3, K = 2.  Costs (rows: queries, columns: classes) and logits (columns: class 0, class 1, void):
        layer 0, image 0   cost [[5, 1], [2, 9], [7, 3]]   table [1, 0, -1]   logits [[0, 9, 1], [3, 2, 1], [0, 0, 5]]
            pairs (0, 1) cost 1: cheapest of class 1, says class 1: a hit;  (1, 0) cost 2: cheapest of class 0, says 0: a hit
            query 2 unmatched, says void
        layer 0, image 1   cost [[4, 4], [4, 4], [1, 8]]   table [-1, 1, -1]  logits [[1, 1, 1], [7, 0, 0], [0, 0, 0]]
            pair (1, 1) cost 4: class 1's column is 4, 4, 8: the FIRST minimum is query 0, not greedy; says class 0: a miss
            queries 0 and 2 unmatched: all-equal rows say class 0, an object: 2 false claims
        layer 1, image 0   cost as layer 0               table [1, -1, 0]   logits as layer 0
            (0, 1): as before, not moved, greedy, a hit;  (2, 0) cost 7: class 0 was query 1's: moved, not greedy, says void: a miss
            query 1 unmatched, says class 0: a false claim
        layer 1, image 1   cost as layer 0               table [0, -1, -1]  logits as layer 0
            (0, 0) cost 4: class 0 was nobody's: moved; column 4, 4, 1: query 2 is cheapest, not greedy; says class 0: a hit
            queries 1 and 2 unmatched: say class 0: 2 false claims
    layer 0: matched 3, cost (1 + 2) + 4 = 7, greedy 2, moved 0, hits 2, false 2; layer 1: matched 3, cost (1 + 7) + 4 = 12, greedy 1,
    moved 2, hits 2, false 3.  usage (layer 1): query 0 in both images, query 2 in image 0."""
    cost = np.array([[[[5, 1], [2, 9], [7, 3]], [[4, 4], [4, 4], [1, 8]]]] * 2, np.float32)
    cls = np.array([[[[0, 9, 1], [3, 2, 1], [0, 0, 5]], [[1, 1, 1], [7, 0, 0], [0, 0, 0]]]] * 2, np.float32)
    table = np.array([[[1, 0, -1], [1, -1, 0]], [[-1, 1, -1], [0, -1, -1]]], np.int32)          # [B, L, Q]
    fields = np.array([[3, np.float64(7).view(np.int64), 2, 0, 2, 2], [3, np.float64(12).view(np.int64), 1, 2, 2, 3]], np.int64)
    return cost, cls, table.reshape(2, 6), fields, np.array([2, 0, 1], np.int32)


def test_restatement_on_tables_worked_by_hand():
    cost, cls, row_class, fields, usage = hand_case()
    got, used = R.row(cost, cls, row_class)
    assert got.tolist() == fields.tolist() and used.tolist() == usage.tolist() and R.costs(got).tolist() == [7.0, 12.0]
    # a table value that is no class is an unmatched query, whatever it is
    for junk in (2, 3, 255, 1 << 30, -7):
        wrong = row_class.copy()
        wrong[0, 0] = junk          # (layer 0, image 0, query 0) no longer holds class 1
        got, _ = R.row(cost, cls, wrong)
        assert got[0].tolist() == [2, np.float64(6).view(np.int64), 1, 0, 1, 3]          # the query says class 1: a false claim
        assert got[1].tolist() == [3, np.float64(12).view(np.int64), 1, 3, 2, 3]          # ... and class 1 is new to layer 1: moved
    # a flagged problem -- its rows all -1 -- adds to unmatched_obj alone: every query but the one that says void (image 0, query 2)
    flagged = row_class.copy().reshape(2, 2, 3)
    flagged[:, 1] = -1
    got, used = R.row(cost, cls, flagged.reshape(2, 6))
    assert got[1].tolist() == [0, 0, 0, 0, 0, 5] and used.tolist() == [0, 0, 0] and got[0].tolist() == fields[0].tolist()
    # a class named twice in one layer belongs to its lowest query
    assert R.owners([1, 1, 0, 5, -1], 2) == {1: 0, 0: 2}


def test_first_index_rules():
    nan, inf = float("nan"), float("inf")
    for values, low, high in (([3.0, 1.0, 1.0, 2.0], 1, 0), ([0.0, 0.0, 0.0], 0, 0), ([nan, 1.0, 2.0], 0, 0), ([1.0, nan, 0.5, 7.0], 2, 3),
                              ([-inf, nan, -inf], 0, 0), ([2.0, inf, inf], 0, 1), ([5.0], 0, 0)):
        assert R.first_argmin(np.array(values, np.float32)) == low and R.first_argmax(np.array(values, np.float32)) == high, values


def test_the_cost_is_summed_in_the_prescribed_order():
    """2^60 + 1 - 2^60: the serial fp64 sum with q ascending is 0, any other association 1; then the images in ascending b"""
    big = np.float32(2.0 ** 60)
    cost = np.zeros((1, 3, 3, 3), np.float32)
    cls = np.zeros((1, 3, 3, 4), np.float32)
    cost[0, 0, [0, 1, 2], [0, 1, 2]] = [big, 1.0, -big]          # image 0: (2^60 + 1) - 2^60 = 0
    cost[0, 1, [0, 1, 2], [0, 1, 2]] = [big, -big, 1.0]          # image 1: (2^60 - 2^60) + 1 = 1
    cost[0, 2, [0, 1, 2], [0, 1, 2]] = [1.0, big, -big]          # image 2: (1 + 2^60) - 2^60 = 0
    table = np.tile(np.array([0, 1, 2], np.int32), (3, 1))
    got, _ = R.row(cost, cls, table)
    assert R.costs(got).tolist() == [1.0] and got[0, R.MATCHED] == 9
    # the images' sums: (2^60 + 1) + (-2^60) = 0 in this order of b, 1 in another
    cost = np.zeros((1, 3, 1, 1), np.float32)
    cost[0, :, 0, 0] = [big, 1.0, -big]
    got, _ = R.row(cost, np.zeros((1, 3, 1, 2), np.float32), np.zeros((3, 1), np.int32))
    assert R.costs(got).tolist() == [0.0] and got[0, R.COST] == 0
    got, _ = R.row(cost[:, [0, 2, 1]], np.zeros((1, 3, 1, 2), np.float32), np.zeros((3, 1), np.int32))
    assert R.costs(got).tolist() == [1.0]
    # nothing matched: +0.0, the word 0
    got, _ = R.row(cost, np.zeros((1, 3, 1, 2), np.float32), np.full((3, 1), -1, np.int32))
    assert got[0].tolist() == [0, 0, 0, 0, 0, 3]


def test_streaks_and_latch_on_a_hand_made_sequence():
    L, Q = 2, 5
    ring, idle, head = R.new_state(L, Q, 3)
    assert ring.shape == (3, 12 + 3) and head.tolist() == [0, -1, 0, 0]

    def row(used, tag):
        f = np.full((L, 6), tag, np.int64)
        u = np.zeros(Q, np.int32)
        u[list(used)] = 1
        return f, u
    R.append(*row([0, 1], 1), ring, idle, head, 2)
    assert idle.tolist() == [0, 0, 1, 1, 1] and R.first_idle(head) is None and head[0] == 1
    # queries 3 and 4 reach the patience in one row: the lowest index wins; 2 starts again
    R.append(*row([0, 2], 2), ring, idle, head, 2)
    assert idle.tolist() == [0, 1, 0, 2, 2] and R.first_idle(head) == (1, 3)
    # a later event (query 1) and a later use of query 3 do not replace the latch
    R.append(*row([3], 3), ring, idle, head, 2)
    assert idle.tolist() == [1, 2, 1, 0, 3] and R.first_idle(head) == (1, 3)
    R.append(*row([], 4), ring, idle, head, 2)          # the wrapped row 0 is overwritten
    assert head.tolist() == [4, (1 << 32) | 3, 0, 0] and ring[0, 0] == 4 and ring[1, 0] == 2 and ring[2, 0] == 3
    # the usage words: int32 pairs, the odd query count padded with a zero
    assert ring[2, 12:].view(np.int32).tolist() == [0, 0, 0, 1, 0, 0] and R.pack(*row([4], 0))[12:].view(np.int32).tolist() == [0, 0, 0, 0, 1, 0]


# ---------------------------------------------------------------------------------------------------- MatchLog over hand-made rows
def views(log):
    """numpy views INTO the log's (CPU) allocation, in the restatement's shapes: (ring, idle, head)"""
    buf = log._buf.numpy()
    Q = log.shape[2]
    return buf[4 + log.pad:].reshape(log.window, log.words), buf[4:4 + log.pad].view(np.int32)[:Q], buf[:4]


def make_rows(rng, n, L, Q, never=()):
    """n rows of plausible figures: (fields [L, 6], usage [Q]); the queries of `never` are not used"""
    rows = []
    for _ in range(n):
        f = np.zeros((L, 6), np.int64)
        for l in range(L):
            matched = int(rng.integers(3, 9))
            f[l] = [matched, 0, rng.integers(0, matched + 1), rng.integers(0, matched + 1) if l else 0, rng.integers(0, matched + 1),
                    rng.integers(0, 5)]
            f[l, R.COST] = np.float64(rng.integers(1, 4000) / 256).view(np.int64)
        u = rng.integers(1, 3, Q).astype(np.int32)
        u[list(never)] = 0
        rows.append((f, u))
    return rows


def test_matchlog_layout_read_and_wrap():
    import spike2former_amd as s2f
    assert s2f.MatchLog.prefix == "match" and s2f.MatchLog.HEAD == (0, -1) and issubclass(s2f.MatchLog, s2f.DeviceRing)
    log = s2f.MatchLog(window=3, patience=2, device="cpu")
    with pytest.raises(RuntimeError, match="bind"):
        log.read()
    log.bind(4, 2, 7, 5)
    assert log.shape == (4, 2, 7, 5) and log.window == 3 and log.head.tolist() == [0, -1, 0, 0] and log.words == 24 + 4 == R.row_words(4, 7)
    assert log.partials.shape == (4, 2, 6) and log.partials.dtype == torch.int64 and log.usage.shape == (2, 7) and log.usage.dtype == torch.int32
    assert log.head.data_ptr() == log._buf.data_ptr() and log.idle.data_ptr() == log._buf.data_ptr() + 32
    assert log.ring.data_ptr() == log._buf.data_ptr() + 8 * (4 + 4) and log.ring.shape == (3, 28) and log.idle.shape == (7,)
    empty = log.read()
    assert empty.rows.shape == (0, 4, 6) and empty.usage.shape == (0, 7) and empty.count == 0 and empty.first_idle is None
    assert empty.idle.tolist() == [0] * 7
    ring, idle, head = views(log)
    rows = make_rows(np.random.default_rng(1), 5, 4, 7, never=[2])
    for r in rows[:2]:
        R.append(*r, ring, idle, head, log.patience)
    peek = log.read(consume=False)
    assert peek.count == 2 and np.array_equal(peek.rows, np.stack([f for f, _ in rows[:2]])) and peek.first_idle == (1, 2)
    assert np.array_equal(peek.usage, np.stack([u for _, u in rows[:2]])) and peek.usage.dtype == np.int32
    assert np.array_equal(log.read().rows, peek.rows) and log.read().rows.shape[0] == 0          # consumed
    for r in rows[2:]:
        R.append(*r, ring, idle, head, log.patience)
    read = log.read()
    assert read.count == 5 and np.array_equal(read.rows, np.stack([f for f, _ in rows[2:]]))          # the three since, oldest first
    log._last = 0
    read = log.read()
    assert read.count == 5 and np.array_equal(read.usage, np.stack([u for _, u in rows[2:]]))          # a window of three: the last three
    assert read.rows.dtype == np.int64 and np.array_equal(read.idle, idle) and read.idle[2] == 5
    assert np.array_equal(s2f.MatchLog.costs(read.rows), R.costs(read.rows)) and s2f.MatchLog.costs(read.rows).shape == (3, 4)
    log.clear()
    assert log.head.tolist() == [0, -1, 0, 0] and int(log.ring.abs().sum()) == 0 and int(log.idle.abs().sum()) == 0 and log.read().count == 0
    for kw in (dict(window=0), dict(patience=0)):
        with pytest.raises(ValueError):
            s2f.MatchLog(**kw)
    for L, B, Q, K in ((0, 1, 1, 1), (17, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 257, 1), (1, 1, 1, 0), (1, 1, 1, 255)):
        with pytest.raises(ValueError):
            s2f.MatchLog(device="cpu").bind(L, B, Q, K)
    s2f.MatchLog(device="cpu").bind(16, 1, 256, 254)


def test_report_keys_line_and_warning():
    import spike2former_amd as s2f
    L, Q = 3, 6
    log = s2f.MatchLog(window=8, patience=2, device="cpu").bind(L, 2, Q, 9)
    ring, idle, head = views(log)
    rows = make_rows(np.random.default_rng(2), 5, L, Q, never=[4])
    rows[3][1][1] = rows[4][1][1] = 0          # query 1: unused in the last two rows as well
    log.rebase(100)
    for r in rows[:3]:
        R.append(*r, ring, idle, head, 2)
    keys, items, warning = log.report(103, 100)
    t = np.stack([f for f, _ in rows[:3]]).sum(0)
    cost = np.stack([R.costs(f) for f, _ in rows[:3]]).sum(0)
    used = np.stack([u for _, u in rows[:3]]).sum(0)
    assert list(keys) == ["match/class_error", "match/matched", "match/cost", "match/greedy_share", "match/moved_share", "match/false_pos",
                          "match/queries_used", "match/idle_max"]
    m = int(t[-1, 0])
    assert keys["match/class_error"] == 100.0 - 100.0 * int(t[-1, 4]) / m and keys["match/matched"] == m / 3
    assert keys["match/cost"] == float(cost[-1]) / m and keys["match/greedy_share"] == int(t[-1, 2]) / m
    assert keys["match/moved_share"] == int(t[-1, 3]) / m and keys["match/false_pos"] == int(t[-1, 5]) / 3
    assert keys["match/queries_used"] == int((used > 0).sum()) <= Q - 1 and keys["match/idle_max"] == 3
    assert items["iter"] == 103 and items["rows"] == 3 and items["usage"] == used.tolist() and len(items["layers"]) == L
    for l, layer in enumerate(items["layers"]):
        assert layer == dict(class_error=100.0 - 100.0 * int(t[l, 4]) / int(t[l, 0]), matched=int(t[l, 0]) / 3, cost=float(cost[l]) / int(t[l, 0]),
                             greedy_share=int(t[l, 2]) / int(t[l, 0]), moved_share=int(t[l, 3]) / int(t[l, 0]), false_pos=int(t[l, 5]) / 3)
    assert items["layers"][0]["moved_share"] == 0.0 and items["layers"][-1] == {k[6:]: v for k, v in list(keys.items())[:6]}
    json.dumps(items)
    # query 4 was idle from row 0 on: its streak reached 2 in row 1 -> iteration 102
    assert warning is not None and "query 4 " in warning and "iteration 102" in warning and " 2 iterations" in warning
    for r in rows[3:]:
        R.append(*r, ring, idle, head, 2)
    keys, items, again = log.report(105, 103)
    assert items["rows"] == 2 and items["iter"] == 105 and keys["match/idle_max"] == 5 and again == warning
    assert items["usage"] == (rows[3][1] + rows[4][1]).tolist() and items["usage"][1] == 0
    # nothing appended since: no keys, no line; the latch is still reported (LoggerHook issues it once)
    keys, items, again = log.report(106, 105)
    assert keys == {} and items is None and again == warning
    # rows without one matched pair: the keys whose denominator is 0 are left out
    R.append(np.array([[0, 0, 0, 0, 0, 4]] * L, np.int64), np.zeros(Q, np.int32), ring, idle, head, 2)
    keys, items, _ = log.report(107, 106)
    assert keys == {"match/matched": 0.0, "match/false_pos": 4.0, "match/queries_used": 0, "match/idle_max": 6}
    assert items["layers"] == [dict(matched=0.0, false_pos=4.0)] * L


# ---------------------------------------------------------------------------------------------------- ABI and the op
def test_abi_rows_and_argument_errors():
    from spike2former_amd import _lib, ops
    lib = _lib.lib
    sig = _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "s2f.h")) as f:
        src = f.read()
    assert lib.s2f_version() >= 56 and len(sig["s2f_match_log_partials"][1]) == 10 and len(sig["s2f_match_log_rows"][1]) == 11
    for name in ("s2f_match_log_partials", "s2f_match_log_rows"):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(decl.split(",")) == len(sig[name][1]) and hasattr(lib, name)
    assert int(re.search(r"#define S2F_MATCH_LOG_MAX_LAYERS (\d+)", src).group(1)) == ops.MATCH_LOG_MAX_LAYERS == 16
    assert int(re.search(r"#define S2F_MATCH_LOG_FIELDS (\d+)", src).group(1)) == len(ops.MATCH_LOG_FIELDS) == 6
    assert ops.MATCH_LOG_FIELDS == R.FIELDS and ops.match_log_row_words(7, 100) == 42 + 50 and ops.match_log_row_words(1, 1) == 7
    call = lib.s2f_match_log_partials
    good = [P, P, P, 3, 2, 10, 20, P, P, None]          # cost, cls, row_class, L, B, Q, K, partials, usage, stream
    for k in (0, 1, 2, 7, 8):
        args = list(good)
        args[k] = None
        assert call(*args) == -1 and b"null" in lib.s2f_last_error()
    for k, value, word in ((3, 0, b"L 0 "), (3, 17, b"L 17 "), (4, 0, b"B 0 "), (4, 65536, b"B 65536 "), (5, 0, b"Q 0 "), (5, 257, b"Q 257 "),
                           (6, 0, b"K 0 "), (6, 255, b"K 255 "), (6, -1, b"K -1 ")):
        args = list(good)
        args[k] = value
        assert call(*args) == -1 and word in lib.s2f_last_error(), (k, value, lib.s2f_last_error())
    for k, off in ((0, 2), (1, 2), (2, 2), (7, 4), (8, 2)):
        args = list(good)
        args[k] = P + off
        assert call(*args) == -2, k
    rows = lib.s2f_match_log_rows
    good = [P, P, 3, 2, 10, P, 4, P, 2, P, None]          # partials, usage, L, B, Q, ring, window, idle, patience, head, stream
    for k in (0, 1, 5, 7, 9):
        args = list(good)
        args[k] = None
        assert rows(*args) == -1 and b"null" in lib.s2f_last_error()
    for k, value, word in ((2, 0, b"L 0 "), (2, 17, b"L 17 "), (3, 0, b"B 0 "), (4, 0, b"Q 0 "), (4, 257, b"Q 257 "), (6, 0, b"window"),
                           (8, 0, b"patience")):
        args = list(good)
        args[k] = value
        assert rows(*args) == -1 and word in lib.s2f_last_error(), (k, value, lib.s2f_last_error())
    for k, off in ((0, 4), (1, 2), (5, 4), (7, 2), (9, 4)):
        args = list(good)
        args[k] = P + off
        assert rows(*args) == -2, k


def test_the_op_has_no_host_route_and_checks_its_tensors():
    import spike2former_amd as s2f
    from spike2former_amd import ops
    L, B, Q, K = 3, 2, 5, 4

    def tensors():
        return dict(cost=torch.zeros(L, B, Q, K), cls=torch.zeros(L, B, Q, K + 1), row_class=torch.zeros(B, L * Q, dtype=torch.int32),
                    partials=torch.zeros(L, B, 6, dtype=torch.int64), usage=torch.zeros(B, Q, dtype=torch.int32),
                    ring=torch.zeros(3, 18 + 3, dtype=torch.int64), idle=torch.zeros(Q, dtype=torch.int32), head=torch.tensor([0, -1, 0, 0]),
                    patience=2)
    with pytest.raises(RuntimeError, match="no CPU route"):
        ops.match_log_append(**tensors())
    for name, value in (("patience", 0), ("cost", torch.zeros(L, B, Q, K, dtype=torch.float64)), ("cost", torch.zeros(L, B, Q, K + 1)),
                        ("cost", torch.zeros(17, B, Q, K)), ("cls", torch.zeros(L, B, Q, K)), ("cls", torch.zeros(L, B, Q, K + 1).transpose(0, 1)),
                        ("row_class", torch.zeros(B, L * Q, dtype=torch.int64)), ("row_class", torch.zeros(L, B * Q, dtype=torch.int32)),
                        ("partials", torch.zeros(L, B, 6, dtype=torch.int32)), ("usage", torch.zeros(B, Q + 1, dtype=torch.int32)),
                        ("ring", torch.zeros(3, 18 + 2, dtype=torch.int64)), ("ring", torch.zeros(0, 18 + 3, dtype=torch.int64)),
                        ("idle", torch.zeros(Q + 1, dtype=torch.int32)), ("head", torch.zeros(2, dtype=torch.int64))):
        args = tensors()
        args[name] = value
        with pytest.raises(ValueError):
            ops.match_log_append(**args)
    log = s2f.MatchLog(device="cpu").bind(L, B, Q, K)
    with pytest.raises(RuntimeError, match="no CPU route"):
        log.append(torch.zeros(L, B, Q, K), torch.zeros(L, B, Q, K + 1), torch.zeros(B, L * Q, dtype=torch.int32))
    with pytest.raises(ValueError, match="bound to"):
        log.append(torch.zeros(L, B, Q + 1, K), torch.zeros(L, B, Q + 1, K + 1), torch.zeros(B, L * (Q + 1), dtype=torch.int32))


def test_the_step_takes_the_log_and_none_by_default():
    import inspect
    from spike2former_amd.graph import GraphedHungarianStep, _Captured
    assert inspect.signature(GraphedHungarianStep.__init__).parameters["match_log"].default is None and _Captured.match_log is None


# ---------------------------------------------------------------------------------------------------- TrainLoop + LoggerHook
class FakeAugment:
    rng = np.random.default_rng(0)

    def __call__(self, images, segs, out=None):
        pass


class FakeStep:
    """what the loop sees of a captured step with a TrainLog and a MatchLog: one scripted row into each per call"""

    def __init__(self, model, log, match_log, script):
        self.model, self.log, self.match_log, self.script, self.calls = model, log, match_log, script, 0
        self.static_in, self.static_seg = torch.zeros(1), torch.zeros(1, dtype=torch.uint8)
        self.vals = {k: torch.zeros(()) for k in ("loss", "grad_norm", "clip_coef")}
        log.bind(self.vals)
        match_log.bind(2, 1, 3, 4)

    def __call__(self):
        self.vals["loss"].fill_(1.0 + self.calls)
        self.log.append()
        R.append(*self.script[self.calls], *views(self.match_log), self.match_log.patience)
        self.calls += 1


def make_loop(tmp_path, script, interval, window=4, patience=3, **kw):
    import spike2former_amd as s2f
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.train import FlatAdamW, LinearThenPoly
    model = torch.nn.Linear(2, 2)
    opt = FlatAdamW(model, FlatGradAllReduce(model.parameters(), 1), lr=0.01)
    sched = LinearThenPoly(opt, warmup=2, total=50, start_factor=0.1)
    step = FakeStep(model, s2f.TrainLog(window=8, device="cpu", capacity=4), s2f.MatchLog(window=window, patience=patience, device="cpu"),
                    script)
    return s2f.TrainLoop(step, opt, sched, FakeAugment(), [(None, None)], max_iters=len(script),
                         hooks=[dict(type="LoggerHook", interval=interval, window_size=2)], work_dir=str(tmp_path), **kw)


def scripted(n):
    """query 0 is matched in every iteration, query 1 in the first two only (its streak is 3 at iteration 5), query 2 in odd ones"""
    rows = []
    for it in range(n):
        f = np.array([[2, 0, 1, 0, 1, 1], [2 + it % 2, 0, 1, it % 2, 1 + it % 2, 1]], np.int64)
        f[:, R.COST] = np.array([1.5, 2.0 + it]).view(np.int64)
        rows.append((f, np.array([1, 1 if it < 2 else 0, it % 2], np.int32)))
    return rows


def test_train_loop_picks_the_log_up_and_the_hook_writes_it(tmp_path, caplog):
    script = scripted(10)
    loop = make_loop(tmp_path, script, interval=4)
    assert loop.match_log is loop.step.match_log and loop.logs == [(loop.match_log, int)]
    with caplog.at_level(logging.INFO, logger="spike2former_amd"):
        loop.run()
    with open(tmp_path / "vis_data" / "scalars.json") as f:
        lines = [json.loads(line) for line in f]
    with open(tmp_path / "vis_data" / "match.jsonl") as f:
        match = [json.loads(line) for line in f]
    assert [r["iter"] for r in lines] == [4, 8, 10] == [r["iter"] for r in match] and [r["rows"] for r in match] == [4, 4, 2]
    first = 0
    for rec, mr in zip(lines, match):
        chunk = script[first:rec["iter"]]
        k, first = len(chunk), rec["iter"]
        t = np.stack([f for f, _ in chunk]).sum(0)[-1]
        cost = sum(float(R.costs(f)[-1]) for f, _ in chunk)
        assert set(rec) >= {"match/class_error", "match/matched", "match/cost", "match/greedy_share", "match/moved_share", "match/false_pos",
                            "match/queries_used", "match/idle_max", "loss", "lr", "iter"}
        assert rec["match/class_error"] == 100.0 - 100.0 * int(t[4]) / int(t[0]) and rec["match/matched"] == int(t[0]) / k
        assert rec["match/cost"] == cost / int(t[0]) and rec["match/false_pos"] == 1.0
        assert mr["usage"] == np.stack([u for _, u in chunk]).sum(0).tolist() and len(mr["layers"]) == 2
        assert mr["layers"][-1]["matched"] == rec["match/matched"] and mr["layers"][0]["matched"] == 2.0
    assert [r["match/queries_used"] for r in lines] == [3, 2, 2] and [r["match/idle_max"] for r in lines] == [2, 6, 8]
    warnings = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1 and "query 1 " in warnings[0].message and "iteration 5" in warnings[0].message          # once, of three lines
    assert sum("Iter(train)" in r.message and "match/class_error" in r.message for r in caplog.records) == 3


def test_logger_hook_refuses_a_ring_shorter_than_the_interval(tmp_path):
    loop = make_loop(tmp_path, scripted(6), interval=5, window=4)
    with pytest.raises(ValueError, match="MatchLog of 4 rows"):
        loop.run()


def test_a_resumed_loop_rebases_the_log_and_a_loop_without_it_has_none(tmp_path):
    import spike2former_amd as s2f
    loop = make_loop(tmp_path, scripted(2), interval=2)
    loop.step.match_log.rebase(40)
    assert loop.step.match_log.base == 40
    keys, items, _ = (R.append(*scripted(1)[0], *views(loop.step.match_log), 3), loop.step.match_log.report(41, 40))[1]
    assert items["iter"] == 41 and keys["match/matched"] == 2.0
    loop.step.match_log = None
    again = s2f.TrainLoop(loop.step, loop.optimizer, loop.scheduler, FakeAugment(), [(None, None)], max_iters=2)
    assert again.match_log is None and again.logs == []
