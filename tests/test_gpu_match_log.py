"""GPU: the match log -- s2f_match_log_partials / s2f_match_log_rows (csrc/matchlog.hip) against the numpy restatement
tests/matchlog_ref.py: every integer field equal and the `cost` word equal by BITS (both sides add the same fp32 values as doubles in
the same order), tied inputs, an image without a class, a flagged problem, table values that are no class, the ring and its latch, the
launches inside a captured graph, and MatchLog inside GraphedHungarianStep on the tiny configuration C1_64, built here from the
ingredients of tests/step_rig.py (`examples`, `make_batches`, `feed`, `reset`)."""
import ctypes
import functools
import gc
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matchlog_ref as R  # noqa: E402
import step_rig as rig  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (2, 2, 10, 20),
          (3, 2, 7, 70),          # more classes present than queries, K > 64
          (2, 1, 65, 5),          # Q > 64
          (6, 2, 100, 150), (16, 1, 256, 254)]
GARBAGE = 0x5A5A5A5A


# ---------------------------------------------------------------------------------------------------- the kernels
def crit(Q, K):
    from spike2former_amd.loss import MaskFormerLoss
    return MaskFormerLoss(K, Q)


def present_classes(rng, B, Q, K):
    """count_full [B, 256]: image b holds Q + 3 + b classes where K >= 10 Q (more classes present than queries: every query is
    matched), else about half as many as there are queries or classes (some queries stay unmatched)"""
    count = np.zeros((B, 256), np.float32)
    for b in range(B):
        n = min(K, Q + 3 + b if K >= 10 * Q else max(1, min(K, Q) // 2 + b))
        count[b, rng.permutation(K)[:n]] = 1 + rng.integers(0, 50, n)
    return count


@functools.lru_cache(maxsize=None)
def case(L, B, Q, K):
    """seeded inputs of one shape and their row, computed once and shared: (cost [L, B, Q, K], cls [L, B, Q, K+1], row_class [B, L*Q]
    from MaskFormerLoss.match_tables, fields [L, 6], usage [Q]).  Costs and logits are distinct multiples of 1/1024 within every
    column and row (exact in fp32: fewer than 2^21 of them), so the restatement has no tie to break.  An odd layer's costs are the
    layer before's plus 1 -- the same assignment, nothing moves -- and an even one's are fresh.  Every third matched query's own class
    logit and every other unmatched query's void logit is raised above its row, so hits, misses and false claims all occur."""
    rng = np.random.default_rng(7919 * L + 131 * Q + K)
    cost = ((1 + rng.permutation(L * B * Q * K)).reshape(L, B, Q, K) / 1024).astype(np.float32)
    for l in range(1, L, 2):
        cost[l] = cost[l - 1] + np.float32(1.0)
    n = L * B * Q * (K + 1)
    cls = (rng.permutation(n).reshape(L, B, Q, K + 1) / 1024).astype(np.float32)
    count = present_classes(rng, B, Q, K)
    _, row_class, _ = crit(Q, K).match_tables(cost, count)
    table = row_class.reshape(B, L, Q)
    for l in range(L):
        for b in range(B):
            for q in range(Q):
                c = int(table[b, l, q])
                if c >= 0 and q % 3 == 0:
                    cls[l, b, q, c] = np.float32((n + q) / 1024)
                elif c < 0 and q % 2 == 0:
                    cls[l, b, q, K] = np.float32((n + q) / 1024)
    assert float(np.float32((n + Q) / 1024)) * 1024 == n + Q          # (exact)
    fields, usage = R.row(cost, cls, row_class)
    for a in (cost, cls, row_class, fields, usage):
        a.setflags(write=False)
    return cost, cls, row_class, fields, usage


def device_log(L, B, Q, K, window=3, patience=2):
    import spike2former_amd as s2f
    log = s2f.MatchLog(window=window, patience=patience, device="cuda").bind(L, B, Q, K)
    log.partials.fill_(GARBAGE)          # every word of the workspace is written by the first launch
    log.usage.fill_(GARBAGE)
    return log


def on_device(*arrays):
    return tuple(torch.from_numpy(np.array(a)).cuda() for a in arrays)          # (copies: the shared cases are read-only)


def check_row(log, fields, usage, index=-1):
    """the log's row `index` of the rows read equals (fields, usage): integers equal, the cost word by bits; prints the figures first"""
    read = log.read(consume=False)
    got, used = read.rows[index], read.usage[index]
    print(f"fields {got.tolist()}\n  want {fields.tolist()}\n  cost {R.costs(got).tolist()} want {R.costs(fields).tolist()}; "
          f"usage differs in {int((used != usage).sum())} of {len(usage)}")
    assert got.dtype == np.int64 and np.array_equal(got, fields)          # (the cost column: int64 words, so equal BY BITS)
    assert used.dtype == np.int32 and np.array_equal(used, usage)
    return read


@pytest.mark.parametrize("L,B,Q,K", SHAPES)
def test_kernel_equals_the_restatement(L, B, Q, K):
    cost, cls, row_class, fields, usage = case(L, B, Q, K)
    log = device_log(L, B, Q, K)
    log.append(*on_device(cost, cls, row_class))
    read = check_row(log, fields, usage)
    assert read.count == 1 and read.rows.shape == (1, L, 6) and read.usage.shape == (1, Q) and log.head.tolist() == [1, -1, 0, 0]
    assert int(log.partials.eq(GARBAGE).sum()) == 0 and int(log.usage.eq(GARBAGE).sum()) == 0
    assert int(log.ring[1:].ne(0).sum()) == 0          # the other rows: untouched
    assert np.array_equal(read.idle, (usage == 0).astype(np.int32))
    table = row_class.reshape(B, L, Q)
    assert fields[:, R.MATCHED].tolist() == [(table[:, l] >= 0).sum() for l in range(L)] and fields[-1, R.MATCHED] > 0
    assert fields[0, R.MOVED] == 0 and (fields[1::2, R.MOVED] == 0).all()          # an odd layer repeats the layer before
    if L > 2:
        assert fields[2, R.MOVED] > 0
    if fields[-1, R.MATCHED] >= 6:          # hits and misses both occur
        assert 0 < fields[-1, R.CLS_HIT] < fields[-1, R.MATCHED] and fields[-1, R.GREEDY] > 0
    unmatched = int((table[:, -1] < 0).sum())
    assert (unmatched == 0) == (K >= 10 * Q or Q == 1) and 0 <= fields[-1, R.UNMATCHED_OBJ] <= unmatched
    if unmatched >= 4:          # every other unmatched query says void, the others claim an object
        assert 0 < fields[-1, R.UNMATCHED_OBJ] < unmatched
    assert (R.costs(fields) > 0).all()


def test_tied_costs_and_logits_the_first_index_decides():
    """constant cost columns: query 0 is every class's first arg-min; equal logits: index 0 is every row's first arg-max.  A NaN logit
    at index 0 stands, one elsewhere never wins; a NaN cost at q = 0 stands, one elsewhere never wins."""
    L, B, Q, K = 2, 2, 7, 5
    cost = np.tile(np.arange(1, K + 1, dtype=np.float32) / 1024, (L, B, Q, 1))
    cls = np.full((L, B, Q, K + 1), 0.25, np.float32)
    table = np.full((B, L, Q), -1, np.int32)
    table[0, 0, [0, 3, 6]] = [2, 0, 4]          # query 0 -> class 2 (greedy), query 3 -> class 0 (a hit, not greedy), query 6 -> class 4
    table[0, 1, [0, 3, 5]] = [2, 4, 0]          # class 2 stays, 4 and 0 move
    table[1, 0, [1]] = [0]
    table[1, 1, [1, 0]] = [0, 3]          # class 0 stays with query 1 (a hit), class 3 is new: moved; query 0: greedy
    cls[1, 1, 2, 0] = np.nan          # an unmatched query whose x[0] is NaN: arg-max 0, an object
    cls[1, 1, 3, 4] = np.nan          # a NaN elsewhere never wins: arg-max 0
    cls[1, 1, 4, :] = [0.25, 0.25, 0.25, 0.25, 0.25, 0.5]          # the void column alone above: no false claim
    cost[1, 0, 0, 4] = np.nan          # class 4's column starts with NaN: query 0 stands, its owner (query 3) is not greedy
    cost[1, 0, 4, 0] = np.nan          # a NaN further down class 0's column never wins: query 0 is its arg-min, not the owner 5
    row_class = table.reshape(B, L * Q)
    fields, usage = R.row(cost, cls, row_class)
    # layer 0: 4 matched, greedy 1 (query 0 / class 2), hits: class 0 pairs = 2, unmatched 10, all claim class 0
    assert fields[0, [0, 2, 3, 4, 5]].tolist() == [4, 1, 0, 2, 10]
    # layer 1: 5 matched; greedy: (0, 2) of image 0 and (0, 3) of image 1; moved: classes 4 and 0 of image 0, class 3 of image 1;
    # hits: (5, 0) of image 0 and (1, 0) of image 1; unmatched 9, query 4 of image 1 says void
    assert fields[1, [0, 2, 3, 4, 5]].tolist() == [5, 2, 3, 2, 8]
    assert usage.tolist() == [2, 1, 0, 1, 0, 1, 0]
    log = device_log(L, B, Q, K)
    log.append(*on_device(cost, cls, row_class))
    check_row(log, fields, usage)


def test_an_image_without_a_class_and_a_flagged_problem():
    L, B, Q, K = 3, 2, 10, 20
    cost, cls, _, _, _ = case(2, 2, 10, 20)
    cost, cls = np.concatenate([cost, cost[:1] + np.float32(2.0)]), np.concatenate([cls, cls[:1]])
    count = np.zeros((B, 256), np.float32)
    count[0, [1, 5, 7, 19]] = 3          # image 1: nothing but ignored pixels
    count[1, 255] = 100
    _, row_class, avg = crit(Q, K).match_tables(cost, count)
    table = row_class.reshape(B, L, Q)
    assert (table[1] == -1).all() and (table[0] >= 0).sum() == 4 * L and avg.tolist() == [5.0] * L
    fields, usage = R.row(cost, cls, row_class)
    assert fields[:, R.MATCHED].tolist() == [4] * L and usage.max() == 1 and usage.sum() == 4
    log = device_log(L, B, Q, K)
    log.append(*on_device(cost, cls, row_class))
    check_row(log, fields, usage)
    # what the assignment does with a problem it flags (a non-finite cost in a present column): that problem's rows are all -1.  It
    # adds to `unmatched_obj` alone; the layer behind it sees every one of its own pairs as moved
    flagged = row_class.copy().reshape(B, L, Q)
    flagged[0, 1] = -1
    flagged = flagged.reshape(B, L * Q)
    f2, u2 = R.row(cost, cls, flagged)
    assert f2[1, :5].tolist() == [0, 0, 0, 0, 0] and f2[1, R.UNMATCHED_OBJ] > fields[1, R.UNMATCHED_OBJ]
    assert f2[2, R.MOVED] == f2[2, R.MATCHED] == 4 and np.array_equal(f2[0], fields[0]) and np.array_equal(u2, usage)
    log.append(*on_device(cost, cls, flagged))
    check_row(log, f2, u2)
    flagged = flagged.reshape(B, L, Q).copy()
    flagged[0, 2] = -1          # the LAST layer flagged: no query is used
    f3, u3 = R.row(cost, cls, flagged.reshape(B, L * Q))
    assert u3.sum() == 0 and f3[2, :5].tolist() == [0] * 5
    log.append(*on_device(cost, cls, flagged.reshape(B, L * Q)))
    read = check_row(log, f3, u3)
    assert np.array_equal(read.idle, np.where(usage > 0, 1, 3))          # nobody was matched in the last row


def test_a_table_value_that_is_no_class_counts_as_unmatched():
    L, B, Q, K = 2, 2, 10, 20
    cost, cls, row_class, fields, usage = case(L, B, Q, K)
    table = row_class.copy().reshape(B, L, Q)
    bad = [K, K + 1, 255, 1 << 30, np.iinfo(np.int32).max, -2, np.iinfo(np.int32).min]
    hit = 0
    for b in range(B):
        for l in range(L):
            matched = np.flatnonzero(table[b, l] >= 0)
            for i, q in enumerate(matched[:4]):
                table[b, l, q] = bad[(hit + i) % len(bad)]
            hit += 4
    wrong = table.reshape(B, L * Q)
    f2, u2 = R.row(cost, cls, wrong)
    assert (f2[:, R.MATCHED] < fields[:, R.MATCHED]).all() and (f2[:, R.MATCHED] > 0).all()
    log = device_log(L, B, Q, K)
    log.append(*on_device(cost, cls, wrong))
    check_row(log, f2, u2)
    assert log.head.tolist() == [1, -1, 0, 0]


def test_ring_wraps_and_the_latch_keeps_the_first_idle_query():
    L, B, Q, K = 2, 2, 5, 4
    rng = np.random.default_rng(3)
    cost = (rng.permutation(L * B * Q * K).reshape(L, B, Q, K) / 1024).astype(np.float32)
    cls = (rng.permutation(L * B * Q * (K + 1)).reshape(L, B, Q, K + 1) / 1024).astype(np.float32)
    # per append: the queries the LAST layer matches in (image 0, image 1).  Query 4 is never used, query 3 only in row 2, query 2
    # not in rows 0 and 1: queries 2, 3 and 4 reach the patience of 2 in row 1 -- the lowest one is latched, and stays
    used = [([0], [1]), ([0, 1], []), ([2, 3], [0]), ([0], [0, 1]), ([1], [2])]
    log = device_log(L, B, Q, K, window=3, patience=2)
    ring, idle, head = R.new_state(L, Q, 3)
    c, s = on_device(cost, cls)
    rows = []
    for it, per_image in enumerate(used):
        table = np.full((B, L, Q), -1, np.int32)
        for b, queries in enumerate(per_image):
            table[b, 1, queries] = np.arange(len(queries))
            table[b, 0, 4] = 1          # (the first layer uses query 4: that is not the last layer's usage)
        row_class = table.reshape(B, L * Q)
        log.append(c, s, torch.from_numpy(row_class).cuda())
        rows.append(R.row(cost, cls, row_class))
        R.append(*rows[-1], ring, idle, head, 2)
        torch.cuda.synchronize()
        assert log.head.tolist() == head.tolist() and np.array_equal(log.idle.cpu().numpy(), idle), it
        assert np.array_equal(log.ring.cpu().numpy(), ring), it
    assert R.first_idle(head) == (1, 2)
    read = log.read()
    assert read.count == 5 and read.first_idle == (1, 2) and read.idle.tolist() == [1, 0, 0, 2, 5]
    assert np.array_equal(read.rows, np.stack([f for f, _ in rows[2:]])) and np.array_equal(read.usage, np.stack([u for _, u in rows[2:]]))
    assert read.usage.tolist() == [[1, 0, 1, 1, 0], [2, 1, 0, 0, 0], [0, 1, 1, 0, 0]]


# ---------------------------------------------------------------------------------------------------- under capture
def test_append_in_a_captured_graph_equals_eager():
    L, B, Q, K = 2, 2, 10, 20
    cost, cls, row_class, _, _ = case(L, B, Q, K)
    cases = [(np.roll(cost, s, axis=2), np.roll(cls, s, axis=2), np.roll(row_class.reshape(B, L, Q), s, axis=2).reshape(B, L * Q))
             for s in (0, 1, 3)]          # the queries rolled: the same pairs under other names, added in another order
    eager, graphed = device_log(L, B, Q, K, window=4), device_log(L, B, Q, K, window=4)
    for arrays in cases:
        eager.append(*on_device(*arrays))
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
    for arrays in cases:
        for t, a in zip(static, arrays):
            t.copy_(torch.from_numpy(np.array(a)))
        graph.replay()
    torch.cuda.synchronize()
    assert graphed.head.tolist() == eager.head.tolist() and graphed.head[0] == 3
    assert torch.equal(graphed.ring, eager.ring) and torch.equal(graphed.idle, eager.idle)
    read = graphed.read()
    for arrays, fields, usage in zip(cases, read.rows, read.usage):
        want, used = R.row(*arrays)
        assert np.array_equal(fields, want) and np.array_equal(usage, used)
    assert not np.array_equal(read.usage[0], read.usage[1]) and np.array_equal(read.rows[0][:, [0, 2, 3, 4, 5]], read.rows[1][:, [0, 2, 3, 4, 5]])


# ---------------------------------------------------------------------------------------------------- the step
KERNEL = 0          # hipGraphNodeType


def node_types(graph):
    """{hipGraphNodeType: nodes} of a captured graph that was kept (CUDAGraph(keep_graph=True)), asked of the runtime torch uses:
    counted as tests/test_gpu_seg_log.py counts them"""
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


def build(match_log=None, assign="device", optimizer=True, keep_graph=False):
    """a captured step of this file's own on C1_64, from the ingredients of tests/step_rig.py: its seeded model, FlatAdamW, scheduler,
    TrainLog, TrainAugment and example inputs, with `match_log` handed to the step.  The namespace is the one `rig.feed` and
    `rig.reset` take."""
    import spike2former_amd as s2f
    from spike2former_amd.augment import TrainAugment
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.graph import GraphedHungarianStep
    from spike2former_amd.init_utils import seeded_init
    from spike2former_amd.train import FlatAdamW, LinearThenPoly
    w = s2f.WORKLOADS["C1_64"]
    crop = (w["H"], w["W"])
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C1_64"))).cuda().train()
    s2f.set_keep_membrane(model, False)
    r = types.SimpleNamespace(model=model, K=w["K"], crop=crop, seed=0, eager=False, firing=None, seg_log=None)
    r.sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    r.red = FlatGradAllReduce(model.parameters(), 1)
    r.opt = r.sched = r.log = None
    if optimizer:
        r.opt = FlatAdamW(model, r.red, lr=0.001, weight_decay=0.005, clip_grad=rig.CLIP, paramwise_cfg=rig.PARAMWISE)
        r.sched = LinearThenPoly(r.opt, warmup=4, total=20, start_factor=0.1)
        r.log = s2f.TrainLog(window=8)
    r.aug = TrainAugment(crop_size=crop, scale=(2 * crop[1], crop[0]), ratio_range=(0.5, 2.0), cat_max_ratio=0.75, photometric=True,
                         batch_size=2, max_source_pixels=70 * 90, seed=11, rank=0, **rig.NORM)
    r.match_log = None if match_log is None else s2f.MatchLog(**match_log)
    extra = {} if r.match_log is None else dict(match_log=r.match_log)
    example_in, example_seg = (t.cuda() for t in rig.examples(crop))
    plain_graph = torch.cuda.CUDAGraph
    if keep_graph:
        torch.cuda.CUDAGraph = lambda: plain_graph(keep_graph=True)
    try:
        r.step = GraphedHungarianStep(model, example_in, example_seg, r.red, warmup=1, optimizer=r.opt, assign=assign, log=r.log, **extra)
    finally:
        torch.cuda.CUDAGraph = plain_graph
    reset(r)
    return r


def reset(r):
    rig.reset(r)
    if r.match_log is not None:
        r.match_log.clear()
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def steps():
    import spike2former_amd as s2f
    recipes = dict(plain=dict(keep_graph=True), match=dict(keep_graph=True, match_log=dict(window=8, patience=2)))
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = build(**recipes[name])
        return cache[name]
    get.batches = rig.make_batches(s2f.WORKLOADS["C1_64"]["K"])
    yield get
    for r in cache.values():
        for p in r.model.parameters():
            p.grad = None
    cache.clear()
    gc.collect()


def restated(step):
    """the row of the step's last replay, restated from what the step holds on the device"""
    torch.cuda.synchronize()
    cost = step.match_inputs[0].float().cpu().numpy()
    cls = step.outs[0].detach().float().cpu().numpy()
    return R.row(cost, cls, step.row_class.cpu().numpy())


def test_every_replay_appends_the_row_of_its_own_assignment(steps):
    r = steps("match")
    reset(r)
    ml = r.step.match_log
    assert ml is r.match_log and r.step.two_graphs is False and ml.read().count == 0          # the warm-up passes' rows are not row 0
    Ls, B, Q = r.step.outs[0].shape[:3]
    assert ml.shape == (Ls, B, Q, r.K) and tuple(r.step.match_inputs[0].shape) == (Ls, B, Q, r.K) and r.step.match_inputs[0].is_contiguous()
    assert tuple(r.step.match_inputs[1].shape) == (B, 256)
    for it in range(3):
        rig.feed(r, steps.batches[it])
        r.step()
        r.sched.step()
        fields, usage = restated(r.step)
        read = check_row(ml, fields, usage)
        assert read.count == it + 1 and len(read.rows) == it + 1
        present = (r.step.match_inputs[1][:, :r.K] != 0).sum(1).cpu().numpy()
        assert fields[-1, R.MATCHED] == np.minimum(present, Q).sum() > 0 and (fields[:, R.MATCHED] == fields[-1, R.MATCHED]).all()
        assert usage.sum() == fields[-1, R.MATCHED] and np.isfinite(R.costs(fields)).all()
    r.step.check()
    reset(r)


def test_the_two_graph_form_appends_the_row_too():
    """assign="host": graph A (forward, costs), the assignment on the host, graph B (losses, backward, the log's launches behind the
    tables' upload), on a model of its own without an optimizer"""
    r = build(match_log=dict(window=2, patience=1), assign="host", optimizer=False)
    try:
        ml = r.step.match_log
        assert r.step.two_graphs and ml.read().count == 0
        for it in range(3):          # three rows into a window of two
            rig.feed(r, rig.make_batches(r.K)[it])
            r.step()
        fields, usage = restated(r.step)
        # the cost the host assigned on is the cost the log read
        assert np.array_equal(r.step.host_cost.numpy(), r.step.match_inputs[0].cpu().numpy())
        read = check_row(ml, fields, usage)
        assert read.count == 3 and read.rows.shape[0] == 2 and fields[-1, R.MATCHED] > 0
    finally:
        for p in r.model.parameters():
            p.grad = None


def run(r, batches, count):
    """`count` iterations from the reset step -> per iteration the loss dictionary's values"""
    reset(r)
    out = []

    def behind(it):
        torch.cuda.synchronize()
        out.append({k: float(v) for k, v in r.step.losses.items()})
    rig.iterate(r, batches, 0, count, behind)
    return out


def test_the_graph_grows_by_the_logs_launches_and_the_losses_stay(steps):
    plain, match = steps("plain"), steps("match")
    assert plain.step.match_log is None and not hasattr(plain.step, "match_inputs") and match.step.match_log is match.match_log
    a, b = node_types(plain.step.graph), node_types(match.step.graph)
    print(f"graph nodes by type without / with the log: {a} / {b}")
    assert b[KERNEL] - a[KERNEL] == 2          # s2f_match_log_partials, s2f_match_log_rows: nothing else is launched, copied or cleared
    assert {k: v for k, v in a.items() if k != KERNEL} == {k: v for k, v in b.items() if k != KERNEL}
    # The rule of test_gpu_seg_log.py: the step is not bit-repeatable on this rig (fp32 atomics).  The run-to-run gap of every term
    # is measured on the step WITHOUT the log; where the plain runs agree by bits the run with the log must too, elsewhere within
    # twice the gap.
    runs = [run(plain, steps.batches, 3) for _ in range(3)]
    with_log = run(match, steps.batches, 3)
    assert match.match_log.read().count == 3
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
    reset(plain), reset(match)
