"""GPU: the segmentation log -- s2f_seg_log_partials / s2f_seg_log_rows (csrc/seglog.hip) against the fp64 restatement
tests/seglog_ref.py in exact integers, saturated inputs, the ring and its latch, the launches inside a captured graph, and SegLog
inside GraphedHungarianStep and TrainLoop on the tiny configuration C1_64 (the rig of tests/step_rig.py).

Where fp32 may legitimately pick another class than fp64 -- a pixel whose fp64 top-two score gap is below 4 Q 2^-24 max(1, max score),
the accumulation bound of Q products <= 1 -- the pixel's label is set to 255 in the input handed to BOTH the kernel and the
restatement, so it counts nowhere; at most 0.5 % of the pixels may be such (asserted; the seeded inputs below have none)."""
import ctypes
import functools
import json
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seglog_ref as R  # noqa: E402
import step_rig as rig  # noqa: E402
from step_rig import reset, rigs_fixture  # noqa: E402

pytestmark = pytest.mark.gpu

L = 3
SHAPES = [(1, 1, 1, 2, 2), (2, 5, 3, 6, 10), (2, 37, 19, 10, 14), (3, 100, 150, 16, 24), (1, 100, 254, 8, 12),
          (2, 3, 4, 24, 26),          # 624 pixels: three workgroups per image, the last one ragged
          (1, 130, 65, 4, 6),          # more queries than one LDS table holds: class chunks of 76 (as K = 150), 128 queries
          (1, 130, 80, 4, 6)]          # ... and class chunks of 128 (as K = 254), 64 queries; K <= 32 runs chunks of 32
GARBAGE = 0x5A5A5A5A


# ---------------------------------------------------------------------------------------------------- the kernels
@functools.lru_cache(maxsize=None)
def case(B, Q, K, h, w):
    """seeded inputs of one shape and their fp64 rows, computed once and shared: (cls [L, B, Q, K+1], mask buffer [B, L, Q, h, w], seg
    uint8 [B, 2h, 2w] with the near-tie pixels of ANY layer ignored, rows int64 [L, 3, K] of all layers).  Labels: uniform over the
    classes, about 10 % ignored; with more than one image the last one is ignored altogether (its rows are zero)."""
    rng = np.random.default_rng(1000 * K + Q)
    cls = (rng.standard_normal((L, B, Q, K + 1)) * 3).astype(np.float32)
    buf = (rng.standard_normal((B, L, Q, h, w)) * 4).astype(np.float32)
    seg = rng.integers(0, K, (B, 2 * h, 2 * w)).astype(np.uint8)
    seg[rng.random(seg.shape) < 0.1] = 255
    if B > 1:
        seg[-1] = 255
    masks = buf.transpose(1, 0, 2, 3, 4)
    ties = R.near_ties(cls, masks, range(L))
    assert ties.mean() <= 0.005, f"{int(ties.sum())} of {ties.size} pixels are near ties"
    seg = R.mask_labels(seg, ties)
    rows = R.areas(cls, masks, seg, range(L))
    for a in (cls, buf, seg, rows):
        a.setflags(write=False)
    return cls, buf, seg, rows


def device_log(K, B, Q, h, w, layers, window=3, patience=2):
    import spike2former_amd as s2f
    log = s2f.SegLog(K, window=window, patience=patience, layers=layers, device="cuda").bind(L, B, Q, h, w)
    log.partials.fill_(GARBAGE)          # every word of the workspace is written by the first launch
    return log


def on_device(cls, buf, seg):
    """-> (cls, masks, seg) as the step hands them over: masks is the [L, B, Q, h, w] view of the head's [B, L*Q, hw] buffer"""
    cls, buf, seg = (torch.from_numpy(np.array(a)).cuda() for a in (cls, buf, seg))          # (copies: the shared cases are read-only)
    return cls, buf.permute(1, 0, 2, 3, 4), seg


@pytest.mark.parametrize("layers", ["last", "all"])
@pytest.mark.parametrize("B,Q,K,h,w", SHAPES)
def test_kernel_equals_the_restatement(B, Q, K, h, w, layers):
    cls, buf, seg, rows = case(B, Q, K, h, w)
    want = rows[-1:] if layers == "last" else rows
    log = device_log(K, B, Q, h, w, layers)
    log.append(*on_device(cls, buf, seg))
    read = log.read()
    print(f"shape {(B, Q, K, h, w)} layers {layers}: labelled {int(want[-1, 2].sum())} hits {int(want[-1, 0].sum())} "
          f"differing words {int((read.areas[0] != want).sum()) if read.count == 1 else 'n/a'}")
    assert read.count == 1 and read.areas.shape == (1, len(want), 3, K) and log.head.tolist() == [1, -1, 0, 0]
    assert np.array_equal(read.areas[0], want)
    small = seg[:, ::2, ::2]
    assert int(want[-1, 2].sum()) == int((small < K).sum()) and (B == 1 or int((small[-1] != 255).sum()) == 0)
    assert int(log.partials.eq(GARBAGE).sum()) == 0 and int(log.partials.sum()) == int(want.sum())
    assert int(log.ring[1:].ne(0).sum()) == 0          # the other rows: untouched
    # the same inputs as a contiguous [L, B, Q, h, w] tensor (the op copies it into the buffer's layout): the same row
    c, m, s = on_device(cls, buf, seg)
    log.append(c, m.contiguous(), s)
    assert np.array_equal(log.read().areas[0], want)


def saturated(B, Q, K, h, w, seed):
    """class logits +-30 and mask logits +-30: in (layer l, image b) every query scores the two classes (l + b) % K and (l + b + 2) % K
    at +30 and everything else at -30, so these two classes' scores are EXACTLY tied at every pixel, in fp32 and in fp64 alike (the same
    operations on the same numbers), above every other class: the first maximum decides."""
    rng = np.random.default_rng(seed)
    cls = np.full((L, B, Q, K + 1), -30.0, np.float32)
    for l in range(L):
        for b in range(B):
            cls[l, b, :, [(l + b) % K, (l + b + 2) % K]] = 30.0
    buf = np.where(rng.random((B, L, Q, h, w)) < 0.5, 30.0, -30.0).astype(np.float32)
    seg = rng.integers(0, K, (B, 2 * h, 2 * w)).astype(np.uint8)
    seg[rng.random(seg.shape) < 0.1] = 255
    return cls, buf, seg


def test_saturated_inputs_the_first_maximum_decides():
    B, Q, K, h, w = 2, 7, 5, 6, 10
    cls, buf, seg = saturated(B, Q, K, h, w, 4)
    masks = buf.transpose(1, 0, 2, 3, 4)
    want = R.areas(cls, masks, seg, range(L))          # no pixel left out
    for l in range(L):
        for b in range(B):
            s = R.scores(cls[l, b], masks[l, b], K)
            lo, hi = sorted(((l + b) % K, (l + b + 2) % K))
            assert (s[lo] == s[hi]).all() and (R.argmax_first(s) == lo).all()
    log = device_log(K, B, Q, h, w, "all")
    log.append(*on_device(cls, buf, seg))
    got = log.read().areas[0]
    assert np.array_equal(got, want) and int(got[:, 2].sum()) == L * int((seg[:, ::2, ::2] < K).sum())
    for l in range(L):
        assert sorted(np.flatnonzero(got[l, 1]).tolist()) == sorted({min((l + b) % K, (l + b + 2) % K) for b in range(B)})


def test_ring_wraps_and_the_latch_keeps_the_first_missed_class():
    B, Q, K, h, w = 1, 3, 5, 4, 4
    cls, buf, _ = saturated(B, Q, K, h, w, 5)          # the last layer (l = 2) predicts class min(2, 4) = 2 everywhere
    labels = [[3, 4], [3, 4], [2], [4, 0], [2, 3]]          # per append: the classes in the label map
    log = device_log(K, B, Q, h, w, "last", window=3, patience=2)
    ring, streak, head = R.new_state(K, 1, 3)
    c, m, _ = on_device(cls, buf, np.zeros((B, 2 * h, 2 * w), np.uint8))
    rows = []
    for it, names in enumerate(labels):
        seg = np.array(names, np.uint8)[(np.arange(2 * h)[:, None] // 2 + np.arange(2 * w)[None, :] // 2) % len(names)][None]
        seg[0, 0, 0] = 255
        log.append(c, m, torch.from_numpy(seg).cuda())
        rows.append(R.areas(cls, buf.transpose(1, 0, 2, 3, 4), seg, [L - 1]))
        R.append(rows[-1], ring, streak, head, 2)
        torch.cuda.synchronize()
        assert log.head.tolist() == head.tolist() and np.array_equal(log.streak.cpu().numpy(), streak), it
        assert np.array_equal(log.ring.cpu().numpy(), ring)
    assert R.first_missed(head) == (1, 3)          # classes 3 and 4 reach the patience in row 1: the lower one
    read = log.read()
    assert read.count == 5 and np.array_equal(read.areas, np.stack(rows[2:])) and read.first_missed == (1, 3)
    assert read.streak.tolist() == [1, 0, 0, 3, 3]          # class 2 is hit in rows 2 and 4; an absent class keeps its streak; 3 and 4 are never hit
    assert rows[2][0, 0, 2] > 0 and rows[4][0, 0, 2] > 0 and rows[0][0, 0].sum() == 0


# ---------------------------------------------------------------------------------------------------- under capture
def test_append_in_a_captured_graph_equals_eager():
    B, Q, K, h, w = 2, 37, 19, 10, 14
    cases = []
    for seed in (11, 12, 13):
        cls, buf, seg, _ = case(B, Q, K, h, w)          # other inputs per replay: queries and label maps rolled
        cases.append((np.roll(cls, seed, axis=2), np.roll(buf, seed, axis=2), np.roll(seg, 2 * (seed - 10), axis=2)))
    eager, graphed = device_log(K, B, Q, h, w, "all", window=4), device_log(K, B, Q, h, w, "all", window=4)
    for cls, buf, seg in cases:
        eager.append(*on_device(cls, buf, seg))
    static = on_device(*cases[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graphed.append(*static)          # (warm-up)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphed.clear()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="clear under capture"):
            graphed.clear()
        graphed.append(*static)
    torch.cuda.synchronize()
    assert graphed.head.tolist() == [0, -1, 0, 0]          # recording ran nothing
    for cls, buf, seg in cases:
        static[0].copy_(torch.from_numpy(cls))
        static[1].copy_(torch.from_numpy(buf).permute(1, 0, 2, 3, 4))
        static[2].copy_(torch.from_numpy(seg))
        graph.replay()
    torch.cuda.synchronize()
    assert graphed.head.tolist() == eager.head.tolist() and graphed.head[0] == 3
    assert torch.equal(graphed.ring, eager.ring) and torch.equal(graphed.streak, eager.streak)
    rows = graphed.read().areas
    assert rows.shape[0] == 3 and not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[1], rows[2])
    for (cls, buf, seg), row in zip(cases, rows):          # rolled queries: the scores add up in another order; labels were rolled
        assert np.array_equal(row[:, 2], R.areas(cls, buf.transpose(1, 0, 2, 3, 4), seg, range(L))[:, 2])


# ---------------------------------------------------------------------------------------------------- the step
KERNEL, MEMCPY, MEMSET = 0, 1, 2          # hipGraphNodeType


def node_types(graph):
    """{hipGraphNodeType: nodes} of a captured graph that was kept (CUDAGraph(keep_graph=True)), asked of the runtime torch uses"""
    path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    hip = ctypes.CDLL(path if os.path.exists(path) else "libamdhip64.so")
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    handle, n = ctypes.c_void_p(graph.raw_cuda_graph()), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(handle, None, ctypes.byref(n)) == 0 and n.value > 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(handle, nodes, ctypes.byref(n)) == 0
    out = {}
    for node in nodes:
        kind = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(kind)) == 0
        out[kind.value] = out.get(kind.value, 0) + 1
    return out


# plain: the rig of tests/step_rig.py (FlatAdamW, TrainLog, assign="device"); seg: the same with a SegLog over all layers.  The
# captured graphs are kept so that their nodes can be counted.
recipes = dict(plain=dict(keep_graph=True), seg=dict(keep_graph=True, seg_log=dict(window=8, patience=2, layers="all")))
rigs = rigs_fixture(recipes)


def run(r, batches, count):
    """`count` iterations from the reset rig -> per iteration the loss dictionary's values as fp32 bit patterns {term: int}"""
    reset(r)
    out = []

    def behind(it):
        torch.cuda.synchronize()
        out.append({k: float(v) for k, v in r.step.losses.items()})          # (the dictionary the step returns)
    rig.iterate(r, batches, 0, count, behind)
    return out


def test_every_replay_appends_the_row_of_its_own_outputs(rigs):
    r = rigs("seg")
    reset(r)
    sl = r.step.seg_log
    assert sl is r.seg_log and r.step.two_graphs is False and sl.read().count == 0          # the warm-up passes' rows are not row 0
    Ls, B, Q = r.step.outs[0].shape[:3]
    assert sl.layers == list(range(Ls)) and sl.shape == (Ls, B, Q, *r.step.outs[1].shape[-2:])
    for it in range(3):
        images, segs = rigs.batches[it]
        r.aug(images, segs, out=(r.step.static_in, r.step.static_seg))
        r.step()
        r.sched.step()
        torch.cuda.synchronize()
        cls, masks = (t.detach().float().cpu().numpy() for t in r.step.outs)
        seg = r.step.static_seg.cpu().numpy()
        K = r.K
        read = sl.read()
        assert read.count == it + 1 and read.areas.shape == (1, Ls, 3, K)
        row = read.areas[0]
        ties = R.near_ties(cls, masks, range(Ls))
        assert ties.mean() <= 0.005, f"{int(ties.sum())} of {ties.size} pixels are near ties"
        want = R.areas(cls, masks, R.mask_labels(seg, ties), range(Ls))          # without the near ties ...
        tied = np.bincount(seg[:, ::2, ::2][ties].astype(np.int64), minlength=256)[:K]          # ... whose labels count, whatever they predict
        print(f"iteration {it + 1}: {int(ties.sum())} near ties, labelled {int(row[-1, 2].sum())}, hits per layer {row[:, 0].sum(1).tolist()}")
        assert np.array_equal(row[:, 2], want[:, 2] + tied)
        more_pred, more_hit = row[:, 1] - want[:, 1], row[:, 0] - want[:, 0]
        assert (more_pred >= 0).all() and (more_pred.sum(1) == tied.sum()).all() and (more_hit >= 0).all() and (more_hit <= tied).all()
        assert int(row[-1, 2].sum()) == int((seg[:, ::2, ::2] < K).sum()) > 0
    assert np.isfinite(cls).all() and np.isfinite(masks).all()
    reset(r)


def test_the_two_graph_form_appends_the_row_too():
    """assign="host": graph A (forward, costs), the assignment on the host, graph B (losses, backward, the log's launches), on a model
    of its own without an optimizer; the last layer alone"""
    import spike2former_amd as s2f
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.graph import GraphedHungarianStep
    from spike2former_amd.init_utils import seeded_init
    w = s2f.WORKLOADS["C1_64"]
    crop = (w["H"], w["W"])
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C1_64"))).cuda().train()
    s2f.set_keep_membrane(model, False)
    red = FlatGradAllReduce(model.parameters(), 1)
    sl = s2f.SegLog(w["K"], window=2, patience=1)
    x = torch.randn(2, 3, *crop, generator=torch.Generator().manual_seed(5)).cuda()
    seg = torch.from_numpy(np.stack([rig.region_map(*crop, [1, 2, 3]), rig.region_map(*crop, [4, 5])])).cuda()
    step = GraphedHungarianStep(model, x, seg, red, warmup=1, assign="host", seg_log=sl)
    try:
        assert step.two_graphs and sl.read().count == 0 and sl.layers == [step.outs[0].shape[0] - 1]
        for it in range(3):          # three rows into a window of two
            step()
        torch.cuda.synchronize()
        cls, masks = (t.detach().float().cpu().numpy() for t in step.outs)
        labels = step.static_seg.cpu().numpy()
        read = sl.read()
        ties = R.near_ties(cls, masks, sl.layers)
        assert read.count == 3 and read.areas.shape == (2, 1, 3, w["K"]) and not ties.any()
        assert np.array_equal(read.areas[-1], R.areas(cls, masks, labels, sl.layers)) and int(read.areas[-1][0, 2].sum()) > 0
    finally:
        for p in model.parameters():
            p.grad = None


def test_the_graph_grows_by_the_logs_launches_and_the_losses_stay(rigs):
    plain, seg = rigs("plain"), rigs("seg")
    assert plain.step.seg_log is None and seg.step.seg_log is seg.seg_log
    a, b = node_types(plain.step.graph), node_types(seg.step.graph)
    print(f"graph nodes by type without / with the log: {a} / {b}")
    assert b[KERNEL] - a[KERNEL] == 2          # s2f_seg_log_partials, s2f_seg_log_rows: nothing else is launched, copied or cleared
    assert {k: v for k, v in a.items() if k != KERNEL} == {k: v for k, v in b.items() if k != KERNEL}
    # The step is not bit-repeatable on this rig (fp32 atomics).  The run-to-run gap of every term is measured on the step
    # WITHOUT the log; where the plain runs agree by bits the run with the log must too, elsewhere within twice the gap.
    runs = [run(plain, rigs.batches, 3) for _ in range(3)]
    with_log = run(seg, rigs.batches, 3)
    assert seg.seg_log.read().count == 3
    for it in range(3):
        for term in runs[0][it]:
            vals = [x[it][term] for x in runs]
            gap = max(vals) - min(vals)
            got = with_log[it][term]
            print(f"iteration {it + 1} {term}: plain {vals}, with the log {got}, gap {gap}")
            assert np.isfinite(got)
            if gap == 0:
                assert np.float32(got).view(np.int32) == np.float32(vals[0]).view(np.int32), (it, term, got, vals)
            else:
                assert min(abs(got - v) for v in vals) <= 2 * gap, (it, term, got, vals)
    reset(plain), reset(seg)


def test_the_loop_writes_the_rows_it_read_and_a_resumed_one_rebases(rigs, tmp_path, caplog):
    import spike2former_amd as s2f
    r = rigs("seg")
    reset(r)
    hooks = [dict(type="LoggerHook", interval=2, window_size=2), dict(type="CheckpointHook", interval=2)]
    loop = s2f.TrainLoop(r.step, r.opt, r.sched, r.aug, rigs.batches, max_iters=4, hooks=hooks, work_dir=str(tmp_path))
    assert loop.seg_log is r.seg_log and (r.seg_log, int) in loop.logs
    with caplog.at_level(logging.INFO, logger="spike2former_amd"):
        loop.run()
    rows = r.seg_log.read(consume=False)
    assert rows.count == 4 and r.seg_log.base == 0

    def lines(name):
        with open(tmp_path / "vis_data" / name) as f:
            return [json.loads(line) for line in f]
    scalars, seg = [x for x in lines("scalars.json") if "loss" in x], lines("seg.jsonl")
    assert [x["iter"] for x in scalars] == [2, 4] == [x["iter"] for x in seg] and [x["rows"] for x in seg] == [2, 2]
    r.seg_log._last = 0
    areas = r.seg_log.read(consume=False).areas
    for k, (sc, sj) in enumerate(zip(scalars, seg)):
        t = areas[2 * k:2 * k + 2].sum(0)
        m = s2f.IoUMetric.total_area_to_metrics(t[-1][0], t[-1][1] + t[-1][2] - t[-1][0], t[-1][1], t[-1][2])
        on = np.flatnonzero(t[-1][2] > 0)
        assert set(sc) >= {"decode.acc_seg", "train/mIoU", "train/mAcc", "train/classes", "decode.d0.acc_seg", "loss"}
        assert sc["decode.acc_seg"] == float(m["aAcc"] * 100) and sc["train/classes"] == on.size > 0
        assert sc["train/mIoU"] == round(float(np.nanmean(m["IoU"][on])) * 100, 2)
        assert sc["train/mAcc"] == round(float(np.nanmean(m["Acc"][on])) * 100, 2)
        assert sc["decode.d0.acc_seg"] == t[0][0].sum() / t[0][2].sum() * 100
        assert list(sj["classes"]) == [str(c) for c in on] and sj["classes"][str(on[0])]["pixels"] == int(t[-1][2][on[0]])
        assert 0.0 <= sc["decode.acc_seg"] <= 100.0
    assert sum("Iter(train)" in x.message and "decode.acc_seg" in x.message for x in caplog.records) == 2
    # a resumed run starts the ring afresh: row 0 is iteration 5
    rig.scramble(r)
    r.seg_log.clear()
    again = s2f.TrainLoop(r.step, r.opt, r.sched, r.aug, rigs.batches, max_iters=6, hooks=hooks, work_dir=str(tmp_path), resume=True)
    again.run()
    assert r.seg_log.base == 4 and r.seg_log.read(consume=False).count == 2
    assert [x["iter"] for x in lines("seg.jsonl")] == [2, 4, 6] and lines("seg.jsonl")[-1]["rows"] == 2
    reset(r)
