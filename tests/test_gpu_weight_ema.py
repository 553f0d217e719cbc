"""GPU: the weight average (csrc/ema.hip, ema.WeightEMA, FlatAdamW(ema=...), runner.EMAHook) -- the two kernels on synthetic parameter
lists against the numpy restatement of tests/ema_ref.py by bits, eager and as replays of captured launches; the average inside the
optimizer's update on the tiny configuration C1_64 (the rigs of tests/step_rig.py), eager and under GraphedHungarianStep replay, with
and without accumulative_counts; TrainLoop with EMAHook: what validation sees, what the checkpoint holds, resume and load_from."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_ref as ref          # noqa: E402
import step_rig as rig          # noqa: E402
from step_rig import CLIP, KINDS, PARAMWISE, Elementwise, gaps, new_loop, reset, rigs_fixture, scramble, state_of          # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = -7.25
EMA_CFG = dict(momentum=0.25, begin_iter=2)


# ---------------------------------------------------------------------------------------------------- the kernels
def chunk_elems():
    from spike2former_amd._lib import lib
    return int(lib.s2f_adamw_chunk_elems())


def sizes():
    C = chunk_elems()
    return [1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 7]


NONFINITE_IN = (3, 5)          # the parameters (indices into sizes()) that carry +-inf and NaN: sizes 5 and C


def values(n, seed, nonfinite):
    """arbitrary mantissas over twelve decades, with +-0 and denormals at the front and in a tail position of every tensor that has
    room; `nonfinite`: also +-inf and NaNs (a quiet one with a payload, a signalling one)"""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-42, -1e-40], dtype=np.float32)
    k = min(n, 4)
    v[:k] = np.roll(special, seed % 4)[:k]
    if n > 8:
        v[-1] = np.float32(-1e-45)
    if nonfinite:
        odd = np.array([np.inf, -np.inf, np.nan], dtype=np.float32)
        v[n // 2:n // 2 + 3] = np.roll(odd, seed % 3)[:len(v[n // 2:n // 2 + 3])]
        v.view(np.uint32)[-1] = 0x7FC12345 if seed % 2 else 0x7F812345
        if n > 64:
            v[17], v[33] = np.inf, -np.inf
    return v


class Table:
    """a synthetic parameter list behind FlatAdamW's tables: every size of sizes(), the last one a view that starts at element 1 of
    a larger tensor (4-byte but not 16-byte aligned); the flat buffer with guard words in its pads and behind its end"""

    def __init__(self):
        self.sizes, self.chunk = sizes(), chunk_elems()
        self.bigs, self.params, slots, chunks, off = [], [], [], [], 0
        for i, n in enumerate(self.sizes):
            if i == len(self.sizes) - 1:
                big = torch.full((n + 9,), GUARD, dtype=torch.float32, device="cuda")
                p = big[1:1 + n]
                assert p.data_ptr() % 16 == 4 and big.data_ptr() % 16 == 0
            else:
                big = torch.full((n,), GUARD, dtype=torch.float32, device="cuda")
                p = big
            self.bigs.append(big)
            self.params.append(p)
            slots.append((p.data_ptr(), off, n))
            chunks += [(i, s) for s in range(0, n, self.chunk)]
            off += (n + 3) // 4 * 4
        self.total = off
        self.offsets = [s[1] for s in slots]
        self.slots = torch.tensor(slots, dtype=torch.int64).cuda()
        self.chunks = torch.tensor(chunks, dtype=torch.int32).cuda()
        self.buf = torch.full((off + 64,), GUARD, dtype=torch.float32, device="cuda")
        self.ema = self.buf[:off]
        self.state = torch.zeros(8, dtype=torch.float32, device="cuda")
        self.partials = torch.full((len(chunks) + 2, 2), -1.0, dtype=torch.float64, device="cuda")
        self.covered = np.zeros(off + 64, bool)
        for o, n in zip(self.offsets, self.sizes):
            self.covered[o:o + n] = True

    def put(self, params=None, emas=None):
        for i, n in enumerate(self.sizes):
            if params is not None:
                self.params[i].copy_(torch.from_numpy(params[i]))
            if emas is not None:
                self.ema[self.offsets[i]:self.offsets[i] + n].copy_(torch.from_numpy(emas[i]))

    def get(self):
        """-> (params, emas) as numpy, after checking that nothing outside them was written"""
        torch.cuda.synchronize()
        buf = self.buf.cpu().numpy()
        assert (buf[~self.covered] == GUARD).all(), "a pad word of the flat buffer was written"
        big = self.bigs[-1].cpu().numpy()
        assert big[0] == GUARD and (big[1 + self.sizes[-1]:] == GUARD).all(), "an element next to the unaligned parameter was written"
        return ([p.cpu().numpy() for p in self.params], [buf[o:o + n].copy() for o, n in zip(self.offsets, self.sizes)])


def launch(fn, mode):
    """`fn()` queues launches on the current stream: run them now, or capture them into a hipGraph and replay that once"""
    if mode == "eager":
        fn()
    else:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        graph.replay()
    torch.cuda.synchronize()


def same_bits(got, want):
    return all(np.array_equal(ref.bits(g), ref.bits(w)) for g, w in zip(got, want))


@pytest.fixture(scope="module")
def table():
    return Table()


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_update_equals_the_restatement_by_bits(table, mode):
    """copy, m = 0.5, m = 2e-4, the clamped tail of a 3-entry table, an `interval` skip, the tail again: after every launch the
    average equals ema_ref by bits (through int32 views: NaNs included), the parameters are untouched, the partials of chunks with
    finite inputs are within 1e-12 of numpy fp64 (n * 2^-53 for n <= 4 096 terms is 4.5e-13) and a skipped update leaves both the
    average and the partials as they were"""
    from spike2former_amd import ops
    t = table
    tab_np = np.array([0.9, 0.5, 2e-4], dtype=np.float32)
    tab = torch.from_numpy(tab_np).cuda()
    emas = [values(n, 900 + i, i in NONFINITE_IN) for i, n in enumerate(t.sizes)]
    t.put(emas=emas)
    t.partials.fill_(-1.0)
    first_chunk = np.cumsum([0] + [-(-n // t.chunk) for n in t.sizes])
    steps = [(1, 1, "copy", None), (2, 1, "lerp", 0.5), (3, 1, "lerp", 2e-4), (4, 3, "lerp", 2e-4), (5, 3, "skip", None),
             (7, 2, "lerp", 2e-4)]
    for k, (count, interval, action, m) in enumerate(steps):
        assert ref.decide(count, 0, interval)[0] == action
        params = [values(n, 10 * k + i, i in NONFINITE_IN) for i, n in enumerate(t.sizes)]
        t.put(params=params)
        t.state[4] = float(count)
        before = t.partials.clone()
        launch(lambda: ops.ema_update(t.slots, t.chunks, t.ema, t.state, tab, 0, interval, t.partials[:-2]), mode)
        got_p, got_e = t.get()
        want = [ref.update(e, p, count, tab_np, 0, interval)[0] for e, p in zip(emas, params)]
        assert same_bits(got_p, params), (k, "the parameters were written")
        assert same_bits(got_e, want), (k, action, [i for i in range(len(want)) if not same_bits([got_e[i]], [want[i]])])
        if action == "lerp":          # the momentum it used is the table's entry, not a neighbour's
            i = 6
            assert np.array_equal(ref.bits(want[i]), ref.bits(ref.lerp(emas[i], params[i], np.float32(m))))
        parts = t.partials.cpu().numpy()
        assert (parts[-2:] == -1.0).all()          # nothing behind the table's rows
        if action == "skip":
            assert np.array_equal(ref.bits(parts), ref.bits(before.cpu().numpy())) and same_bits(got_e, emas)
        else:
            want_parts = ref.drift_partials(params, want, t.chunk)
            assert want_parts.shape == parts[:-2].shape
            for i in range(len(t.sizes)):
                rows = slice(first_chunk[i], first_chunk[i + 1])
                if i in NONFINITE_IN:
                    assert not np.isfinite(parts[rows]).all(), i
                else:
                    assert np.isfinite(want_parts[rows]).all()
                    err = np.abs(parts[rows] - want_parts[rows])
                    assert (err <= 1e-12 * want_parts[rows]).all(), (k, i, err, want_parts[rows])
        emas = want
    # without partials: the same average, and no row written
    params = [values(n, 77 + i, i in NONFINITE_IN) for i, n in enumerate(t.sizes)]
    t.put(params=params)
    t.state[4] = 9.0
    t.partials.fill_(-1.0)
    launch(lambda: ops.ema_update(t.slots, t.chunks, t.ema, t.state, tab, 0, 1, None), mode)
    assert same_bits(t.get()[1], [ref.update(e, p, 9, tab_np, 0, 1)[0] for e, p in zip(emas, params)])
    assert bool((t.partials == -1.0).all())


@pytest.mark.parametrize("begin", [0, 1, 3])
def test_begin_decides_on_the_device_as_in_the_restatement(table, begin):
    """updates 1 .. 6 at interval 2 from one launch configuration: what a captured launch does as the optimizer's count moves"""
    from spike2former_amd import ops
    t = table
    tab_np = np.array([0.9, 0.5, 0.125], dtype=np.float32)
    tab = torch.from_numpy(tab_np).cuda()
    emas = [values(n, 300 + i, False) for i, n in enumerate(t.sizes)]
    t.put(emas=emas)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.ema_update(t.slots, t.chunks, t.ema, t.state, tab, begin, 2, t.partials[:-2])
    actions = []
    for count in range(1, 7):
        params = [values(n, 400 + 10 * count + i, False) for i, n in enumerate(t.sizes)]
        t.put(params=params)
        t.state[4] = float(count)
        graph.replay()
        emas = [ref.update(e, p, count, tab_np, begin, 2)[0] for e, p in zip(emas, params)]
        assert same_bits(t.get()[1], emas), (begin, count)
        actions.append(ref.decide(count, begin, 2)[0])
    assert actions == {0: ["copy", "skip", "lerp", "skip", "lerp", "skip"], 1: ["copy", "skip", "lerp", "skip", "lerp", "skip"],
                       3: ["copy", "copy", "copy", "skip", "lerp", "skip"]}[begin]


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_swap_exchanges_bits_and_twice_is_the_identity(table, mode):
    from spike2former_amd import ops
    t = table
    params = [values(n, 500 + i, True) for i, n in enumerate(t.sizes)]          # NaN payloads in every tensor
    emas = [values(n, 600 + i, True) for i, n in enumerate(t.sizes)]
    t.put(params=params, emas=emas)
    launch(lambda: ops.ema_swap(t.slots, t.chunks, t.ema), mode)
    got_p, got_e = t.get()
    assert same_bits(got_p, emas) and same_bits(got_e, params)
    launch(lambda: ops.ema_swap(t.slots, t.chunks, t.ema), mode)
    got_p, got_e = t.get()
    assert same_bits(got_p, params) and same_bits(got_e, emas)


def test_state_copy_serves_the_average(table):
    """loading and saving the buffer needs no kernel of its own: s2f_state_copy's word-counted tables are these tables"""
    from spike2former_amd import ops
    t = table
    params = [values(n, 700 + i, True) for i, n in enumerate(t.sizes)]
    t.put(params=params, emas=[values(n, 800 + i, False) for i, n in enumerate(t.sizes)])
    ops.state_copy(t.params, t.slots, t.chunks, t.ema.view(torch.int32))
    got_p, got_e = t.get()
    assert same_bits(got_e, params) and same_bits(got_p, params)


# ---------------------------------------------------------------------------------------------------- through the optimizer
def params_of(r):
    torch.cuda.synchronize()
    return [p.detach().cpu().numpy().reshape(-1).copy() for p in r.opt.params]


def average_of(r):
    torch.cuda.synchronize()
    flat = r.opt.ema.ema.cpu().numpy()
    return [flat[off:off + p.numel()].copy() for p, off in zip(r.opt.params, r.red.offsets)]


def iterate(r, batches, iterations, watch=None):
    """`iterations` iterations from the rig's start (step_rig.iterate: an eager rig's update is launched there) -> the state, with
    the loss terms of every iteration; `watch(iteration, updated)` runs behind each"""
    reset(r)
    counts = 1 if r.opt.accum is None else r.opt.accum.counts
    losses = {}

    def behind(it):
        for k, v in r.step.losses.items():
            losses[f"loss:{it}:{k}"] = v.detach().clone().reshape(-1)
        if watch is not None:
            watch(it, (it + 1) % counts == 0)
    rig.iterate(r, batches, 0, iterations, behind)
    return {**state_of(r), **losses}


def follow(r, batches, iterations, begin_iter=2, momentum=0.25):
    """run the rig and hold the average against ema_ref applied to the parameters read back after each update -> the final state"""
    tab = ref.table("ExponentialMovingAverage", momentum)
    seen = types.SimpleNamespace(avg=None, updates=0)

    def watch(it, updated):
        if seen.avg is None:
            seen.avg = [np.array(v.cpu().numpy().reshape(-1)) for v in (r.sd0[g["name"]] for g in r.opt.param_groups)]
        got = average_of(r)
        if updated:
            seen.updates += 1
            params = params_of(r)
            seen.avg = [ref.update(e, p, seen.updates, tab, begin_iter, 1)[0] for e, p in zip(seen.avg, params)]
            rep = r.opt.ema.report(seen.updates)
            want = ref.drift(ref.drift_partials(params, seen.avg, chunk_elems()))
            assert abs(rep["ema/drift"] - want) <= 4e-12 * want and rep["ema/momentum"] == (1.0 if seen.updates <= begin_iter else momentum)
        assert same_bits(got, seen.avg), (it, updated)          # (an iteration without an update leaves the average alone)
    out = iterate(r, batches, iterations, watch)
    assert float(r.opt.state[4]) == seen.updates
    moved = sum(not np.array_equal(a, b) for a, b in zip(seen.avg, params_of(r)))
    assert moved > len(seen.avg) // 2          # the average lags the weights: the lerp steps did something
    return out


recipes = dict(ema=dict(ema=EMA_CFG), eager=dict(ema=EMA_CFG, step_optimizer=False, log=False), none=dict(),
               ema_acc2=dict(ema=EMA_CFG, counts=2), acc2=dict(counts=2))
rigs = rigs_fixture(recipes)


def test_without_the_argument_nothing_is_allocated(rigs):
    r = rigs("none")
    assert r.opt.ema is None and r.step.optimizer is r.opt


def test_average_under_replay_follows_the_restatement(rigs):
    r = rigs("ema")
    assert r.opt.ema is not None and r.step._update_in_graph() and r.opt.ema.args["begin_iter"] == 2
    rigs.runs["ema"] = follow(r, rigs.batches, 4)


def test_average_on_the_eager_path_follows_the_restatement(rigs):
    r = rigs("eager")
    assert r.step.optimizer is None
    follow(r, rigs.batches, 4)


def test_average_moves_on_updates_only_under_accumulation(rigs):
    r = rigs("ema_acc2")
    assert r.opt.accum.counts == 2
    rigs.runs["ema_acc2"] = follow(r, rigs.batches, 6)
    assert float(r.opt.state[4]) == 3.0


@pytest.mark.parametrize("pair", [("none", "ema", 4), ("acc2", "ema_acc2", 6)])
def test_the_step_is_what_it_is_without_the_average(rigs, pair):
    """Parameters, moments and every iteration's loss terms against a rig built without `ema`.  The comparison is bit equality
    where the step repeats itself: the rig WITHOUT the argument is run twice first (A, A'), and where A equals A' by bits the rig
    with the average has to equal A by bits.  On C1_64 the backward adds with fp32 atomics and A differs from A' (DESIGN.md section
    9 items 20, 26: 1e-7 on the weights): there no two runs are bit-equal, whatever was built, and the bound is twice the largest
    |A - A'| of that kind of tensor (test_gpu_grad_accum.py's oracle A) -- the bit comparison itself is made on a step without
    atomics, in test_a_step_without_atomics_is_bit_equal_with_and_without_the_average.  Measured on the MI355X: |A - A'| 2.4e-7 ..
    4.0e-7 on the weights, 1.0e-10 .. 1.7e-10 and 1.0e-15 .. 1.4e-15 on the moments, 0 on the loss terms and the count; the rig
    with the average against A: 2.4e-7, 1.2e-10 .. 2.2e-10, 7.5e-16 .. 1.6e-15, 0."""
    plain, with_ema, iterations = pair
    a = iterate(rigs(plain), rigs.batches, iterations)
    a2 = iterate(rigs(plain), rigs.batches, iterations)
    b = rigs.runs.get(with_ema) or follow(rigs(with_ema), rigs.batches, iterations)
    d0, d = gaps(a, a2), gaps(a, b)
    print(f"{plain}: |A - A'| {d0}; {with_ema}: |A - B| {d}")
    assert float(a["step:"]) == float(b["step:"]) and any(k.startswith("loss:") for k in a)
    for k in a:
        kind = next(x for x in KINDS if k.startswith(x))
        if d0[kind] == 0.0:
            assert torch.equal(a[k], b[k]), k
        elif a[k].numel():
            assert float((a[k].double() - b[k].double()).abs().max()) <= 2.0 * d0[kind], (k, d0[kind])


def test_a_step_without_atomics_is_bit_equal_with_and_without_the_average():
    """Four iterations of a captured GraphedStep (the update, and with `ema` the average, inside the graph): weights, moments,
    state words and losses are BIT-equal to a rig built without the argument -- after the premise, that the rig without the argument
    equals itself run twice -- and the average equals ema_ref over the weights read back after each update."""
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.graph import GraphedStep
    from spike2former_amd.train import FlatAdamW, LinearThenPoly
    g = torch.Generator().manual_seed(6)
    inputs = [torch.randn(2, 3, 33, 35, generator=g).cuda() for _ in range(4)]

    def rig(**extra):
        m = Elementwise().cuda()
        red = FlatGradAllReduce(m.parameters(), 1)
        opt = FlatAdamW(m, red, lr=0.001, weight_decay=0.005, clip_grad=CLIP, paramwise_cfg=PARAMWISE, **extra)
        sched = LinearThenPoly(opt, warmup=2, total=10, start_factor=0.1)
        start = {k: v.clone() for k, v in m.state_dict().items()}
        step = GraphedStep(m, lambda y: (y * y).mean(), inputs[0], grad_buffer=red, warmup=1, optimizer=opt)

        def run():
            m.load_state_dict(start)
            opt.exp_avg.zero_(), opt.exp_avg_sq.zero_(), opt.state.zero_()
            if opt.ema is not None:
                opt.ema.reset()
            sched.t = 0
            sched._apply()
            opt.mark_updated()
            losses, history = [], []
            for x in inputs:
                losses.append(step(x).clone())
                sched.step()
                torch.cuda.synchronize()
                history.append([p.detach().cpu().numpy().reshape(-1).copy() for p in opt.params])
            return [p.detach().clone() for p in m.parameters()] + [opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.state.clone()] + losses, history
        return run, opt, start
    none, opt0, start = rig()
    with_ema, opt1, _ = rig(ema=EMA_CFG)
    (a, _), (a2, _), (b, history) = none(), none(), with_ema()
    assert opt0.ema is None and float(a[5][4]) == 4.0 and not torch.equal(a[0], start["backbone_w"])
    for x, y in zip(a, a2):          # the premise: this step repeats itself
        assert torch.equal(x, y)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    tab = ref.table("ExponentialMovingAverage", 0.25)
    avg = [start[g["name"]].cpu().numpy().reshape(-1) for g in opt1.param_groups]
    for t, params in enumerate(history, 1):
        avg = [ref.update(e, p, t, tab, 2, 1)[0] for e, p in zip(avg, params)]
    flat = opt1.ema.ema.cpu().numpy()
    assert same_bits([flat[off:off + p.numel()] for p, off in zip(opt1.params, opt1.red.offsets)], avg)


# ---------------------------------------------------------------------------------------------------- through the loop
HOOKS = [dict(type="EMAHook", **EMA_CFG), dict(type="LoggerHook", interval=3, window_size=2), dict(type="CheckpointHook", interval=3)]


class Spy:
    """reads the parameters back after every iteration (priority 0: ahead of every other hook)"""
    priority = 0

    def __init__(self, r):
        self.r, self.history, self.loaded = r, [], None

    def before_run(self, loop):
        self.loaded = (params_of(self.r), average_of(self.r))

    def after_train_iter(self, loop):
        self.history.append(params_of(self.r))


def picture(seed, B, H, W):
    return (16.0 * torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed))).cuda()


def logits_of(model, x, graph):
    """eval-mode logits, stateless; `graph`: through test_cfg['graph'] (captured at the first call, a replay afterwards)"""
    import spike2former_amd as s2f
    cfg, training = model.test_cfg, model.training
    model.test_cfg = dict(mode="whole", **(dict(graph=dict(capture_after=1)) if graph else {}))
    if not graph:
        kept = model.__dict__.pop("_graphed_predict", None)
    model.eval()
    try:
        with torch.no_grad():
            s2f.reset_net(model)
            return model(x, mode="logits").clone()
    finally:
        model.test_cfg = cfg
        model.train(training)
        if not graph and kept is not None:
            model.__dict__["_graphed_predict"] = kept


@pytest.fixture(scope="module")
def whole_run(rigs, tmp_path_factory):
    """six iterations in the loop on the rig with the average: validation after 3 and 6 -> what each validation saw"""
    r = rigs("ema")
    reset(r)
    work = tmp_path_factory.mktemp("ema_whole")
    spy, seen = Spy(r), []
    x = picture(3, 2, *r.crop)

    def validate():
        assert r.opt.ema.swapped
        params, train, logits = params_of(r), average_of(r), logits_of(r.model, x, graph=True)
        seen.append(types.SimpleNamespace(params=params, train=train, logits=logits,
                                          census=dict(r.model.__dict__["_graphed_predict"].census)))
        return dict(mIoU=float(len(seen)))
    loop = new_loop(r, rigs.batches, 6, [spy] + HOOKS, work_dir=str(work), val_interval=3, validate=validate, async_write=False)
    loop.run()
    start = [r.sd0[g["name"]].cpu().numpy().reshape(-1) for g in r.opt.param_groups]
    tab = ref.table("ExponentialMovingAverage", 0.25)
    avgs, avg = [], start
    for t, params in enumerate(spy.history, 1):
        avg = [ref.update(e, p, t, tab, 2, 1)[0] for e, p in zip(avg, params)]
        avgs.append(avg)
    return types.SimpleNamespace(r=r, work=work, spy=spy, seen=seen, avgs=avgs, x=x, final=(params_of(r), average_of(r)),
                                 state=state_of(r))


def test_validation_sees_the_average(whole_run):
    w = whole_run
    assert len(w.spy.history) == 6 and len(w.seen) == 2 and not w.r.opt.ema.swapped and w.r.model.training
    for k, n in enumerate((3, 6)):
        # per tensor, by bits: the model held the average of n updates, the buffer the training weights
        assert same_bits(w.seen[k].params, w.avgs[n - 1]) and same_bits(w.seen[k].train, w.spy.history[n - 1]), n
    assert not same_bits(w.seen[1].params, w.spy.history[5])          # (the average is not the weights)
    # the training weights after the run are those the last iteration left: validation changed nothing
    assert same_bits(w.final[0], w.spy.history[5]) and same_bits(w.final[1], w.avgs[5])
    assert w.seen[0].census["captures"] == 1 and w.seen[1].census == dict(w.seen[0].census, replays=w.seen[0].census["replays"] + 1)
    import json
    with open(w.work / "vis_data" / "scalars.json") as f:
        lines = [rec for rec in map(json.loads, f) if "lr" in rec]
    assert [rec["iter"] for rec in lines] == [3, 6]
    for rec, n in zip(lines, (3, 6)):
        want = ref.drift(ref.drift_partials(w.spy.history[n - 1], w.avgs[n - 1], chunk_elems()))
        assert rec["ema/momentum"] == 0.25 and abs(rec["ema/drift"] - want) <= 4e-12 * want


def test_the_weights_come_back_when_validation_raises(rigs, tmp_path):
    r = rigs("ema")
    reset(r)
    spy, seen = Spy(r), []

    def validate():
        seen.append(params_of(r))
        raise KeyError("validation failed")
    loop = new_loop(r, rigs.batches, 3, [spy, dict(type="EMAHook", **EMA_CFG)], work_dir=str(tmp_path), val_interval=3, validate=validate)
    with pytest.raises(KeyError, match="validation failed"):
        loop.run()
    assert len(seen) == 1 and not r.opt.ema.swapped
    assert same_bits(params_of(r), spy.history[2]) and not same_bits(seen[0], spy.history[2])


def test_the_checkpoint_holds_the_average_and_the_training_weights(whole_run):
    w = whole_run
    names = [g["name"] for g in w.r.opt.param_groups]
    for n in (3, 6):
        ck = torch.load(w.work / f"iter_{n}.pth", weights_only=True)
        assert list(ck["state_dict"]) == list(w.r.model.state_dict()) and int(ck["ema_state_dict"]["steps"]) == n - 1
        assert list(ck["ema_state_dict"]) == ["steps"] + [f"module.{k}" for k in ck["state_dict"]]
        assert same_bits([ck["state_dict"][k].numpy().reshape(-1) for k in names], w.avgs[n - 1])
        assert same_bits([ck["ema_state_dict"][f"module.{k}"].numpy().reshape(-1) for k in names], w.spy.history[n - 1])
        for k, v in ck["state_dict"].items():
            if k not in names:
                assert torch.equal(v, ck["ema_state_dict"][f"module.{k}"]), k
    final = torch.load(w.work / "iter_6.pth", weights_only=True)
    for k in final["state_dict"]:          # buffers: the training model's, as the run left them (the rig has moved on since)
        if k not in names:
            assert torch.equal(final["state_dict"][k], w.state[f"model:{k}"].cpu()), k


def test_load_from_gives_the_average_and_its_logits(whole_run):
    """the file in a fresh model: the averaged weights by bits, and the eager logits of that model are the logits the swapped
    validation computed through its captured graph after iteration 6"""
    import spike2former_amd as s2f
    from spike2former_amd.init_utils import seeded_init
    w = whole_run
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C1_64"))).cuda().eval()
    s2f.set_keep_membrane(model, False)
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.5)
    s2f.TrainState(model, None).load(str(w.work / "iter_6.pth"))
    got = {k: v.detach().cpu().numpy().reshape(-1) for k, v in model.named_parameters()}
    assert same_bits([got[g["name"]] for g in w.r.opt.param_groups], w.avgs[5])
    logits = logits_of(model, w.x, graph=False)
    assert torch.equal(logits, w.seen[1].logits), float((logits - w.seen[1].logits).abs().max())
    assert not torch.equal(w.seen[0].logits, w.seen[1].logits)          # the replay followed the weights
    # ... and they are not the training weights' logits
    assert not torch.equal(logits_of(w.r.model, w.x, graph=False), logits)


def test_a_resumed_run_continues_the_uninterrupted_one(rigs, whole_run, tmp_path):
    """B: three iterations, a checkpoint, the rig put somewhere else, resumed, three iterations -- against A, the uninterrupted run
    of whole_run.  What the resume itself does is exact and asserted by bits: behind the load the parameters are the file's
    `ema_state_dict`, the average its `state_dict`, and from there the average follows ema_ref over the parameters read back.
    B against A is bit equality where the step repeats itself -- A' (six iterations again) against A says whether it does -- and
    4 x |A - A'| per kind of tensor otherwise, the average counted with the weights (tests/test_gpu_train_loop.py's bound; C1_64's
    backward adds with fp32 atomics).  Measured on the MI355X: |A - A'| 3.1e-7 / 3.6e-7 on the weights in two runs, |B - A| 3.6e-7."""
    w, r = whole_run, rigs("ema")
    a = dict(w.state, **{f"model:ema:{i}": torch.from_numpy(v) for i, v in enumerate(w.final[1])})
    reset(r)
    new_loop(r, rigs.batches, 6).run()
    a2 = dict(state_of(r), **{f"model:ema:{i}": torch.from_numpy(v) for i, v in enumerate(average_of(r))})
    d0 = gaps(a, a2)
    reset(r)
    new_loop(r, rigs.batches, 3, HOOKS, work_dir=str(tmp_path)).run()
    scramble(r)
    spy = Spy(r)
    loop = new_loop(r, rigs.batches, 6, [spy] + HOOKS, work_dir=str(tmp_path), resume=True)
    loop.run()
    assert loop.resumed["meta"]["iter"] == 3 and float(r.opt.state[4]) == 6.0 and "ema_state_dict" not in loop.resumed
    ck = torch.load(tmp_path / "iter_3.pth", weights_only=True)
    names = [g["name"] for g in r.opt.param_groups]
    assert same_bits(spy.loaded[0], [ck["ema_state_dict"][f"module.{k}"].numpy().reshape(-1) for k in names])
    assert same_bits(spy.loaded[1], [ck["state_dict"][k].numpy().reshape(-1) for k in names])
    tab, avg = ref.table("ExponentialMovingAverage", 0.25), spy.loaded[1]
    for t, params in enumerate(spy.history, 4):
        avg = [ref.update(e, p, t, tab, 2, 1)[0] for e, p in zip(avg, params)]
    assert same_bits(average_of(r), avg)
    b = dict(state_of(r), **{f"model:ema:{i}": torch.from_numpy(v) for i, v in enumerate(average_of(r))})
    d = gaps(a, b)
    print("d0 (A against A'):", d0, "largest |B - A|:", d)
    for k in a:
        kind = next(x for x in KINDS if k.startswith(x))
        if d0[kind] == 0.0:
            assert torch.equal(a[k], b[k]), k
        elif a[k].numel():
            assert float((a[k].double() - b[k].double()).abs().max()) <= 4.0 * d0[kind], (k, d0[kind])
