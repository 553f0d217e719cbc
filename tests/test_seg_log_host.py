"""CPU: the segmentation log without a GPU -- the numpy restatement (tests/seglog_ref.py) against a loop over pixels on a case worked
by hand, its arg-max rule, the ring / streak / latch rule, SegLog.read() and report() over rows written into its buffer by the
restatement, the ABI rows and their argument errors, and TrainLoop + LoggerHook over a fake step (seg.jsonl, the keys, ONE warning)."""
import ctypes
import json
import logging
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seglog_ref as R  # noqa: E402

P = 1 << 20          # a 16-byte aligned dummy address: never dereferenced on the host


# ---------------------------------------------------------------------------------------------------- the restatement
def beats(v, best):
    return v > best or (v != v and best == best)


def loop_areas(cls, masks, seg, layer):
    """the rule pixel by pixel in python floats (fp64), nothing vectorised"""
    L, B, Q, K1 = cls.shape
    K, (h, w) = K1 - 1, masks.shape[-2:]
    out = np.zeros((3, K), np.int64)
    for b in range(B):
        table = []
        for q in range(Q):
            row = [float(v) for v in cls[layer, b, q]]
            top = max(row)
            e = [math.exp(v - top) for v in row]
            table.append([v / sum(e) for v in e[:K]])
        for y in range(h):
            for x in range(w):
                score = [0.0] * K
                for q in range(Q):
                    s = 1.0 / (1.0 + math.exp(-float(masks[layer, b, q, y, x])))
                    for k in range(K):
                        score[k] += table[q][k] * s
                pred = 0
                for k in range(1, K):
                    if beats(score[k], score[pred]):
                        pred = k
                label = int(seg[b, 2 * y, 2 * x])
                if label == 255 or label >= K:
                    continue
                out[2, label] += 1
                out[1, pred] += 1
                out[0, label] += pred == label
    return out


def hand_case():
    """L = 1, B = 1, Q = 2, K = 2 on a 2 x 2 mask map.  The two queries' class rows are each other's mirror, P = [[a, b], [b, a]] with
    a > b, so with S the sigmoids of a pixel: score = (a S0 + b S1, b S0 + a S1).
        (0, 0)  S = (.8, .2)  -> class 0, label 0: a hit          (0, 1)  S = (.2, .8)  -> class 1, label 0: a miss
        (1, 0)  S = (.5, .5)  -> an exact tie: class 0, label 1   (1, 1)  label 255: counts nowhere
    -> intersect [1, 0], pred [2, 1], label [2, 1].  The label map's odd rows and columns hold 1s that the stride-2 read skips."""
    cls = np.array([[[[1.5, 0.5, 0.0], [0.5, 1.5, 0.0]]]], np.float32)
    big = math.log(4.0)
    masks = np.array([[[[[big, -big], [0.0, 3.0]], [[-big, big], [0.0, -3.0]]]]], np.float32)
    seg = np.ones((1, 4, 4), np.uint8)
    seg[0, ::2, ::2] = [[0, 0], [1, 255]]
    return cls, masks, seg, np.array([[1, 0], [2, 1], [2, 1]], np.int64)


def test_restatement_equals_the_loop_over_pixels_on_a_case_worked_by_hand():
    cls, masks, seg, want = hand_case()
    assert np.array_equal(loop_areas(cls, masks, seg, 0), want)
    assert np.array_equal(R.areas(cls, masks, seg, [0])[0], want)
    # the tie is exact in fp64: the mirrored rows add the same two products in the other order
    s = R.scores(cls[0, 0], masks[0, 0], 2)
    assert s[0, 1, 0] == s[1, 1, 0] and s[0, 0, 0] > s[1, 0, 0] and s[0, 0, 1] < s[1, 0, 1]
    assert R.near_ties(cls, masks, [0]).tolist() == [[[False, False], [True, False]]]
    # random cases, three layers, labels above K and ignored ones among them
    rng = np.random.default_rng(3)
    cls = rng.normal(size=(3, 2, 4, 4)).astype(np.float32) * 3
    masks = rng.normal(size=(3, 2, 4, 4, 6)).astype(np.float32) * 4
    seg = rng.integers(0, 5, (2, 8, 12)).astype(np.uint8)          # (K = 3: the labels 3 and 4 count nowhere)
    seg[0, :4] = 255
    rows = R.areas(cls, masks, seg, [0, 2])
    for i, l in enumerate((0, 2)):
        assert np.array_equal(rows[i], loop_areas(cls, masks, seg, l))
    assert rows[:, 2].sum() == 2 * int((seg[:, ::2, ::2] < 3).sum()) and (rows[:, 1].sum(1) == rows[:, 2].sum(1)).all()
    assert (rows[:, 0] <= np.minimum(rows[:, 1], rows[:, 2])).all()


def test_first_maximum_and_nan_rules():
    nan = float("nan")
    cases = [([1.0, 3.0, 3.0, 2.0], 1), ([0.0, 0.0, 0.0], 0), ([1.0, nan, 5.0, nan], 1), ([nan, 7.0], 0), ([-1.0, -1.0, nan], 2),
             ([float("inf"), nan], 1), ([2.0, float("inf"), float("inf")], 1), ([-3.0], 0)]
    for values, want in cases:
        best = 0
        for k in range(1, len(values)):
            if beats(values[k], values[best]):
                best = k
        assert best == want
        assert int(R.argmax_first(np.array(values)[:, None])[0]) == want, values
    stacked = np.array([[1.0, nan, 0.0], [1.0, 2.0, nan], [0.0, nan, nan]])
    assert R.argmax_first(stacked).tolist() == [0, 0, 1]
    # a NaN class score poisons its query's whole softmax row, hence every class's score: the first class wins everywhere
    cls, masks, seg, _ = hand_case()
    cls[0, 0, 1, 1] = nan
    row = R.areas(cls, masks, seg, [0])[0]
    assert row.tolist() == [[2, 0], [3, 0], [2, 1]] and np.array_equal(row, loop_areas(cls, masks, seg, 0))


def test_streaks_and_latch_on_a_hand_made_sequence():
    K = 5
    ring, streak, head = R.new_state(K, 2, 3)

    def row(labelled, hit, first_layer_hit=()):
        r = np.zeros((2, 3, K), np.int64)
        for c in labelled:
            r[:, 2, c] = 10
            r[:, 1, c] = 10
        for c in hit:
            r[1, 0, c] = 4
        for c in first_layer_hit:          # the earlier layer's hits do not count for the streaks
            r[0, 0, c] = 4
        return r
    # classes 1 and 3 are labelled and missed; 0 is hit; 2 and 4 are absent
    R.append(row([0, 1, 3], [0], first_layer_hit=[1, 3]), ring, streak, head, 2)
    assert streak.tolist() == [0, 1, 0, 1, 0] and R.first_missed(head) is None and head[0] == 1
    # 3 is absent now: its streak stays; 1 is hit: cleared; 4 is missed for the first time
    R.append(row([1, 4], [1]), ring, streak, head, 2)
    assert streak.tolist() == [0, 0, 0, 1, 1] and R.first_missed(head) is None
    # 3 and 4 reach the patience in one row: the lowest index wins; 1 starts again
    R.append(row([1, 3, 4], []), ring, streak, head, 2)
    assert streak.tolist() == [0, 1, 0, 2, 2] and R.first_missed(head) == (2, 3)
    # a later event (class 1) and a later hit of class 3 do not replace the latch; the wrapped row 0 is overwritten
    R.append(row([1, 3], [3]), ring, streak, head, 2)
    assert streak.tolist() == [0, 2, 0, 0, 2] and R.first_missed(head) == (2, 3) and head.tolist() == [4, (2 << 32) | 3, 0, 0]
    assert np.array_equal(ring[0], row([1, 3], [3])) and np.array_equal(ring[1], row([1, 4], [1]))


# ---------------------------------------------------------------------------------------------------- SegLog over hand-made rows
def views(log):
    """numpy views INTO the log's (CPU) allocation, in the restatement's shapes: (ring, streak, head)"""
    buf = log._buf.numpy()
    n, K = len(log.layers), log.K
    return buf[4 + log.pad:].reshape(log.window, n, 3, K), buf[4:4 + log.pad].view(np.int32)[:K], buf[:4]


def make_rows(rng, n, nl, K, absent=()):
    rows = []
    for _ in range(n):
        label = rng.integers(1, 50, K)
        label[list(absent)] = 0
        inter = (label * rng.random((nl, K))).astype(np.int64)
        extra = rng.integers(0, 9, (nl, K))          # predicted, labelled otherwise
        extra[:, list(absent)] = 0
        extra = extra - extra.sum(1, keepdims=True) // K          # (not a consistent confusion table; report() only adds and divides)
        r = np.zeros((nl, 3, K), np.int64)
        r[:, 0], r[:, 1], r[:, 2] = inter, inter + np.abs(extra), label
        rows.append(r)
    return rows


def test_seglog_layout_read_and_wrap():
    import spike2former_amd as s2f
    assert s2f.SegLog.prefix == "seg" and s2f.SegLog.HEAD == (0, -1) and issubclass(s2f.SegLog, s2f.DeviceRing)
    log = s2f.SegLog(5, window=3, patience=2, device="cpu")
    with pytest.raises(RuntimeError, match="bind"):
        log.read()
    log.bind(4, 2, 7, 6, 10)
    assert log.layers == [3] and log.window == 3 and log.head.tolist() == [0, -1, 0, 0]
    assert log.partials.shape == (1 * 2 * 1, 3, 5) and log.partials.dtype == torch.int32
    assert log.head.data_ptr() == log._buf.data_ptr() and log.ring.data_ptr() == log._buf.data_ptr() + 8 * (4 + 3)
    assert log.ring.shape == (3, 1, 3, 5) and log.streak.shape == (5,) and log.streak.data_ptr() == log._buf.data_ptr() + 32
    empty = log.read()
    assert empty.areas.shape == (0, 1, 3, 5) and empty.count == 0 and empty.first_missed is None and empty.streak.tolist() == [0] * 5
    ring, streak, head = views(log)
    rows = make_rows(np.random.default_rng(1), 5, 1, 5, absent=[2])
    for r in rows[:2]:
        R.append(r, ring, streak, head, log.patience)
    peek = log.read(consume=False)
    assert peek.count == 2 and np.array_equal(peek.areas, np.stack(rows[:2]))
    assert np.array_equal(log.read().areas, np.stack(rows[:2])) and log.read().areas.shape[0] == 0          # consumed
    for r in rows[2:]:
        R.append(r, ring, streak, head, log.patience)
    read = log.read()
    assert read.count == 5 and np.array_equal(read.areas, np.stack(rows[2:]))          # the three since the last read, oldest first
    log._last = 0
    read = log.read()
    assert read.count == 5 and np.array_equal(read.areas, np.stack(rows[2:]))          # five appended, a window of three: the last three
    assert read.areas.dtype == np.int64 and np.array_equal(read.streak, streak)
    log.clear()
    assert log.head.tolist() == [0, -1, 0, 0] and int(log.ring.abs().sum()) == 0 and log.read().count == 0
    with pytest.raises(ValueError):
        s2f.SegLog(255)
    with pytest.raises(ValueError):
        s2f.SegLog(4, window=0)
    with pytest.raises(ValueError):
        s2f.SegLog(4, classes=["a"])
    with pytest.raises(ValueError):
        s2f.SegLog(4, device="cpu").bind(3, 1, 2, 3, 3)          # w odd


def test_report_arithmetic_is_total_area_to_metrics():
    import spike2former_amd as s2f
    K = 6
    names = [f"c{i}" for i in range(K)]
    log = s2f.SegLog(K, window=8, patience=2, classes=names, device="cpu").bind(3, 1, 2, 2, 2)
    ring, streak, head = views(log)
    rows = make_rows(np.random.default_rng(2), 5, 1, K, absent=[4])
    rows[3][0, 0, 1] = rows[4][0, 0, 1] = 0          # class 1: labelled, never hit in the last two rows
    log.rebase(100)
    for r in rows[:3]:
        R.append(r, ring, streak, head, 2)
    keys, items, warning = log.report(103, 100)
    t = np.stack(rows[:3]).sum(0)[0]
    m = s2f.IoUMetric.total_area_to_metrics(t[0], t[1] + t[2] - t[0], t[1], t[2])
    on = [0, 1, 2, 3, 5]
    assert list(keys) == ["decode.acc_seg", "train/mIoU", "train/mAcc", "train/classes"] and warning is None
    assert keys["decode.acc_seg"] == float(m["aAcc"] * 100) == t[0].sum() / t[2].sum() * 100          # (aAcc first, then percent)
    assert keys["train/mIoU"] == round(float(np.mean(m["IoU"][on])) * 100, 2)
    assert keys["train/mAcc"] == round(float(np.mean(m["Acc"][on])) * 100, 2) and keys["train/classes"] == 5
    assert items["iter"] == 103 and items["rows"] == 3 and list(items["classes"]) == [names[c] for c in on]
    for c in on:
        assert items["classes"][names[c]] == dict(IoU=float(t[0][c] / (t[1][c] + t[2][c] - t[0][c])), Acc=float(t[0][c] / t[2][c]),
                                                  pixels=int(t[2][c]))
    json.dumps(items)
    # the next line is over the rows since: two of them, and the latch of class 1 (missed in rows 3 and 4 -> iteration 105)
    for r in rows[3:]:
        R.append(r, ring, streak, head, 2)
    keys, items, warning = log.report(105, 103)
    t = np.stack(rows[3:]).sum(0)[0]
    m = s2f.IoUMetric.total_area_to_metrics(t[0], t[1] + t[2] - t[0], t[1], t[2])
    assert keys["decode.acc_seg"] == float(m["aAcc"] * 100) and items["rows"] == 2 and items["iter"] == 105
    assert items["classes"]["c1"]["IoU"] == 0.0 and "c4" not in items["classes"]
    assert warning is not None and "class c1 " in warning and "iteration 105" in warning and " 2 iterations" in warning
    # nothing appended since: no keys, no line; the latch is still reported (LoggerHook issues it once)
    keys, items, again = log.report(106, 105)
    assert keys == {} and items is None and again == warning
    # rows without one labelled pixel: the count of classes, and no figure
    R.append(np.zeros((1, 3, K), np.int64), ring, streak, head, 2)
    keys, items, _ = log.report(107, 106)
    assert keys == {"train/classes": 0} and items is None
    # without names the class index is the name
    bare = s2f.SegLog(K, window=2, patience=1, device="cpu").bind(1, 1, 1, 2, 2)
    r = np.zeros((1, 3, K), np.int64)
    r[0, 1, 0] = r[0, 2, 3] = 4
    R.append(r, *views(bare), 1)
    keys, items, warning = bare.report(1, 0)
    assert keys["decode.acc_seg"] == 0.0 and list(items["classes"]) == ["3"] and "class 3 " in warning and "iteration 1" in warning


def test_all_layers_report_the_earlier_layers_accuracy():
    import spike2former_amd as s2f
    K = 4
    log = s2f.SegLog(K, window=4, patience=3, layers="all", device="cpu").bind(3, 2, 5, 4, 4)
    assert log.layers == [0, 1, 2] and log.ring.shape == (4, 3, 3, K) and log.partials.shape == (3 * 2 * 1, 3, K)
    ring, streak, head = views(log)
    rows = make_rows(np.random.default_rng(11), 2, 3, K)
    for r in rows:
        R.append(r, ring, streak, head, 3)
    keys, items, warning = log.report(2, 0)
    t = np.stack(rows).sum(0)
    assert list(keys) == ["decode.acc_seg", "train/mIoU", "train/mAcc", "train/classes", "decode.d0.acc_seg", "decode.d1.acc_seg"]
    for i, key in enumerate(("decode.d0.acc_seg", "decode.d1.acc_seg", "decode.acc_seg")):
        assert keys[key] == t[i][0].sum() / t[i][2].sum() * 100
    assert len({keys["decode.d0.acc_seg"], keys["decode.d1.acc_seg"], keys["decode.acc_seg"]}) == 3 and warning is None
    m = s2f.IoUMetric.total_area_to_metrics(t[2][0], t[2][1] + t[2][2] - t[2][0], t[2][1], t[2][2])
    assert keys["train/mIoU"] == round(float(np.nanmean(m["IoU"])) * 100, 2) and items["rows"] == 2
    picked = s2f.SegLog(K, layers=[0, -1], device="cpu").bind(5, 1, 1, 2, 2)
    assert picked.layers == [0, 4]
    with pytest.raises(ValueError):
        s2f.SegLog(K, layers=[7], device="cpu").bind(5, 1, 1, 2, 2)
    with pytest.raises(ValueError):
        s2f.SegLog(K, layers="first")


# ---------------------------------------------------------------------------------------------------- ABI and the op
def test_abi_rows_and_argument_errors():
    from spike2former_amd import _lib, ops
    lib = _lib.lib
    sig = _lib.SIGNATURES
    assert lib.s2f_version() >= 53 and len(sig["s2f_seg_log_partials"][1]) == 13 and len(sig["s2f_seg_log_rows"][1]) == 10
    assert lib.s2f_seg_log_tile_pixels() == 256 and ops.seg_log_tiles(16, 24) == 2 and ops.seg_log_tiles(2, 2) == 1
    assert ops.seg_log_tiles(16, 16) == 1 and ops.seg_log_tiles(24, 26) == 3 and ops.seg_log_tiles(256, 256) == 256
    assert ops.SEG_LOG_MAX_LAYERS == 32 and ops.SEG_LOG_MAX_CLASSES == 254
    table = (ctypes.c_int32 * 3)(0, 1, 2)
    T = ctypes.cast(table, ctypes.c_void_p)
    call = lib.s2f_seg_log_partials
    good = [P, P, P, T, 3, 3, 2, 5, 19, 10, 14, P, None]          # mask, cls, seg, layers, nl, L, B, Q, K, h, w, partials, stream
    for k in (0, 1, 2, 3, 11):
        args = list(good)
        args[k] = None
        assert call(*args) == -1 and b"null" in lib.s2f_last_error()

    def bad(k, value, word):
        args = list(good)
        args[k] = value
        assert call(*args) == -1 and word in lib.s2f_last_error(), (k, value, lib.s2f_last_error())
    for K in (0, 255, -1):
        bad(8, K, b"K ")
    bad(7, 0, b"Q ")
    bad(10, 13, b"w must be even")          # w odd
    bad(9, 1, b"multiple of 4")          # h*w = 14
    bad(4, 0, b"scored layers")
    bad(4, 33, b"scored layers")
    bad(5, 2, b"layer 2 outside")          # the table names layer 2 of a decoder of 2
    table[1] = -1
    bad(5, 3, b"layer -1 outside")
    table[1] = 1
    bad(5, 0, b"L ")
    bad(6, 0, b"B ")
    assert call(P + 2, P, P, T, 3, 3, 2, 5, 19, 10, 14, P, None) == -2 and call(P, P, P, T, 3, 3, 2, 5, 19, 10, 14, P + 1, None) == -2
    rows = lib.s2f_seg_log_rows
    good = [P, 3, 2, 19, P, 4, P, 2, P, None]          # partials, nl, per_layer, K, ring, window, streak, patience, head, stream
    for k in (0, 4, 6, 8):
        args = list(good)
        args[k] = None
        assert rows(*args) == -1 and b"null" in lib.s2f_last_error()
    for k, value, word in ((1, 0, b"scored layers"), (2, 0, b"per layer"), (3, 0, b"K "), (3, 255, b"K "), (5, 0, b"window"),
                           (7, 0, b"patience")):
        args = list(good)
        args[k] = value
        assert rows(*args) == -1 and word in lib.s2f_last_error(), (k, value)
    assert rows(P, 3, 2, 19, P + 4, 4, P, 2, P, None) == -2 and rows(P, 3, 2, 19, P, 4, P + 2, 2, P, None) == -2
    assert rows(P, 3, 2, 19, P, 4, P, 2, P + 4, None) == -2


def test_the_op_has_no_host_route_and_checks_its_tensors():
    from spike2former_amd import ops
    B, L, Q, K, h, w = 2, 3, 5, 4, 2, 4

    def tensors():
        return dict(pred=torch.zeros(B, L * Q, h * w), cls=torch.zeros(L, B, Q, K + 1), seg_u8=torch.zeros(B, 2 * h, 2 * w, dtype=torch.uint8),
                    layers=[2], partials=torch.zeros(B, 3, K, dtype=torch.int32), ring=torch.zeros(3, 1, 3, K, dtype=torch.int64),
                    streak=torch.zeros(K, dtype=torch.int32), head=torch.tensor([0, -1, 0, 0]), patience=2)
    with pytest.raises(RuntimeError, match="no CPU route"):
        ops.seg_log_append(**tensors())
    for name, value in (("layers", [3]), ("layers", []), ("patience", 0), ("partials", torch.zeros(B, 3, K, dtype=torch.int64)),
                        ("ring", torch.zeros(3, 2, 3, K, dtype=torch.int64)), ("streak", torch.zeros(K + 1, dtype=torch.int32)),
                        ("seg_u8", torch.zeros(B, 2 * h, 2 * w, dtype=torch.int64)), ("pred", torch.zeros(B, L * Q, h * w + 4)),
                        ("cls", torch.zeros(L, B, Q, 256)), ("head", torch.zeros(2, dtype=torch.int64))):
        args = tensors()
        args[name] = value
        with pytest.raises(ValueError):
            ops.seg_log_append(**args)
    log_append = __import__("spike2former_amd").SegLog(K, device="cpu").bind(L, B, Q, h, w).append
    with pytest.raises(RuntimeError, match="no CPU route"):
        log_append(torch.zeros(L, B, Q, K + 1), torch.zeros(L, B, Q, h, w), torch.zeros(B, 2 * h, 2 * w, dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------------- TrainLoop + LoggerHook
class FakeAugment:
    rng = np.random.default_rng(0)

    def __call__(self, images, segs, out=None):
        pass


class FakeStep:
    """what the loop sees of a captured step with a TrainLog and a SegLog: one scripted row into each per call"""

    def __init__(self, model, log, seg_log, script):
        self.model, self.log, self.seg_log, self.script, self.calls = model, log, seg_log, script, 0
        self.static_in, self.static_seg = torch.zeros(1), torch.zeros(1, dtype=torch.uint8)
        self.vals = {k: torch.zeros(()) for k in ("loss", "grad_norm", "clip_coef")}
        log.bind(self.vals)
        seg_log.bind(2, 1, 3, 2, 2)

    def __call__(self):
        self.vals["loss"].fill_(1.0 + self.calls)
        self.log.append()
        R.append(self.script[self.calls], *views(self.seg_log), self.seg_log.patience)
        self.calls += 1


def make_loop(tmp_path, script, interval, window=4, patience=3, **kw):
    import spike2former_amd as s2f
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.train import FlatAdamW, LinearThenPoly
    model = torch.nn.Linear(2, 2)
    opt = FlatAdamW(model, FlatGradAllReduce(model.parameters(), 1), lr=0.01)
    sched = LinearThenPoly(opt, warmup=2, total=50, start_factor=0.1)
    step = FakeStep(model, s2f.TrainLog(window=8, device="cpu", capacity=4),
                    s2f.SegLog(3, window=window, patience=patience, classes=["road", "tree", "sky"], device="cpu"), script)
    return s2f.TrainLoop(step, opt, sched, FakeAugment(), [(None, None)], max_iters=len(script),
                         hooks=[dict(type="LoggerHook", interval=interval, window_size=2)], work_dir=str(tmp_path), **kw)


def scripted(n):
    """road is always hit; tree is labelled and missed from iteration 3 on (streak 3 at iteration 5); sky is absent in odd iterations"""
    rows = []
    for it in range(n):
        r = np.zeros((1, 3, 3), np.int64)
        r[0, 2] = [8, 4, 4 if it % 2 == 0 else 0]
        r[0, 0] = [6 + it % 2, 2 if it < 2 else 0, 1 if it % 2 == 0 else 0]
        r[0, 1] = [10, 2, r[0, 2].sum() - 12]
        rows.append(r)
    return rows


def test_train_loop_picks_the_log_up_and_the_hook_writes_it(tmp_path, caplog):
    script = scripted(10)
    loop = make_loop(tmp_path, script, interval=4)
    assert loop.seg_log is loop.step.seg_log and (loop.seg_log, int) in loop.logs
    with caplog.at_level(logging.INFO, logger="spike2former_amd"):
        loop.run()
    with open(tmp_path / "vis_data" / "scalars.json") as f:
        lines = [json.loads(line) for line in f]
    with open(tmp_path / "vis_data" / "seg.jsonl") as f:
        seg = [json.loads(line) for line in f]
    assert [r["iter"] for r in lines] == [4, 8, 10] == [r["iter"] for r in seg] and [r["rows"] for r in seg] == [4, 4, 2]
    first = 0
    for rec, sr in zip(lines, seg):
        t = np.stack(script[first:rec["iter"]]).sum(0)[0]
        first = rec["iter"]
        assert set(rec) >= {"decode.acc_seg", "train/mIoU", "train/mAcc", "train/classes", "loss", "lr", "iter"}
        assert rec["decode.acc_seg"] == t[0].sum() / t[2].sum() * 100 and rec["train/classes"] == int((t[2] > 0).sum())
        iou = t[0] / (t[1] + t[2] - t[0])
        assert rec["train/mIoU"] == round(float(iou[t[2] > 0].mean()) * 100, 2)
        assert rec["train/mAcc"] == round(float((t[0] / t[2])[t[2] > 0].mean()) * 100, 2)
        assert sr["classes"]["road"] == dict(IoU=float(iou[0]), Acc=float(t[0][0] / t[2][0]), pixels=int(t[2][0]))
    assert [r["train/classes"] for r in lines] == [3, 3, 3] and list(seg[0]["classes"]) == ["road", "tree", "sky"]
    warnings = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1 and "class tree " in warnings[0].message and "iteration 5" in warnings[0].message          # once, of three lines
    assert sum("Iter(train)" in r.message and "decode.acc_seg" in r.message for r in caplog.records) == 3


def test_logger_hook_refuses_a_ring_shorter_than_the_interval(tmp_path):
    loop = make_loop(tmp_path, scripted(6), interval=5, window=4)
    with pytest.raises(ValueError, match="SegLog of 4 rows"):
        loop.run()


def test_a_loop_without_the_log_has_none(tmp_path):
    import spike2former_amd as s2f
    loop = make_loop(tmp_path, scripted(2), interval=2)
    loop.step.seg_log = None
    again = s2f.TrainLoop(loop.step, loop.optimizer, loop.scheduler, FakeAugment(), [(None, None)], max_iters=2)
    assert again.seg_log is None and again.logs == []
