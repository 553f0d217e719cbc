"""GPU: gradient accumulation (FlatAdamW(accumulative_counts=k), train.GradAccum) -- the two kernels of csrc/optim.hip against the
numpy restatement of tests/accum_ref.py by bits, the captured step on the tiny configuration C1_64 against two oracles, the
default path against a rig built without the argument, TrainLoop at counts 3 over 7 iterations with a resume on a group boundary,
and two ranks on one GPU.  The rigs are tests/step_rig.py's (the pictures, seeds and schedule of tests/test_gpu_train_loop.py)."""
import json
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accum_ref as ref          # noqa: E402
from step_rig import CLIP, KINDS, Elementwise, feed, gaps, new_loop, reset, rigs_fixture, scramble, state_of          # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -7.25
SIZES = (1, 3, 4, 5, 1023, 1024, 16383, 16384, 16385, 2 * 16384 + 7)


def rtol(numel):
    """tests/test_gpu_grad_log.py's bound for a sum of `numel` exact non-negative fp64 terms, restated: only the order of the
    additions differs"""
    return numel * 2.0 ** -53


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def gradient(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)


def guarded(values, extra=64):
    """a device buffer of the values followed by guard words -> (the whole buffer, the view of the values)"""
    buf = torch.full((len(values) + extra,), GUARD, dtype=torch.float32, device="cuda")
    buf[:len(values)].copy_(torch.from_numpy(values))
    return buf, buf[:len(values)]


def run_accumulate(g, acc, out, scale, partials):
    from spike2former_amd._lib import check, lib
    from spike2former_amd.ops.core import _stream
    check(lib.s2f_grad_accumulate(g.data_ptr(), None if acc is None else acc.data_ptr(), out.data_ptr(), g.numel(), scale,
                                  None if partials is None else partials.data_ptr(), _stream()), "s2f_grad_accumulate")


def run_sqnorm(g):
    from spike2former_amd._lib import check, lib
    from spike2former_amd.ops.core import _stream
    part = torch.full((ref.parts(g.numel()) + 2,), -1.0, dtype=torch.float64, device="cuda")
    check(lib.s2f_grad_sqnorm(g.data_ptr(), g.numel(), part.data_ptr(), _stream()), "s2f_grad_sqnorm")
    return part


# (acc given, where the result goes)
ALIASING = ((False, "g"), (False, "new"), (True, "g"), (True, "acc"), (True, "new"))


# ---------------------------------------------------------------------------------------------------- the accumulate kernel
@pytest.mark.parametrize("scale", [0.5, 1.0 / 3.0])
@pytest.mark.parametrize("n", SIZES)
def test_accumulate_equals_the_restatement_by_bits(n, scale):
    from spike2former_amd._lib import lib
    assert lib.s2f_grad_sqnorm_parts(n) == ref.parts(n)
    g0, a0 = gradient(n, n), gradient(n, n + 1)
    want_parts = ref.sq_partials(g0)
    gbuf, g = guarded(g0)
    sq = run_sqnorm(g).cpu().numpy()
    assert np.array_equal(bits(sq[:-2]), bits(want_parts)) and (sq[-2:] == -1.0).all()          # (the restatement is s2f_grad_sqnorm's)
    for with_acc, where in ALIASING:
        gbuf, g = guarded(g0)
        abuf, a = guarded(a0) if with_acc else (None, None)
        obuf, o = {"g": (gbuf, g), "acc": (abuf, a)}.get(where) or guarded(np.zeros(n, np.float32))
        part = torch.full((ref.parts(n) + 2,), -1.0, dtype=torch.float64, device="cuda")
        run_accumulate(g, a, o, scale, part)
        want = ref.accumulate(g0, a0 if with_acc else None, scale)
        case = (n, scale, with_acc, where)
        assert np.array_equal(bits(o.cpu().numpy()), bits(want)), case
        for buf in (gbuf, abuf, obuf):          # nothing behind the n-th element was written
            assert buf is None or bool((buf[n:] == GUARD).all()), case
        if where != "g":
            assert np.array_equal(bits(g.cpu().numpy()), bits(g0)), case
        if with_acc and where != "acc":
            assert np.array_equal(bits(a.cpu().numpy()), bits(a0)), case
        got = part.cpu().numpy()
        assert np.array_equal(bits(got[:-2]), bits(sq[:-2])) and (got[-2:] == -1.0).all(), case          # of the INPUT g, as s2f_grad_sqnorm
    # without partials: the same result, nothing else written
    gbuf, g = guarded(g0)
    obuf, o = guarded(np.zeros(n, np.float32))
    run_accumulate(g, None, o, scale, None)
    assert np.array_equal(bits(o.cpu().numpy()), bits(ref.accumulate(g0, None, scale))) and bool((obuf[n:] == GUARD).all())


def test_non_finite_values_propagate():
    n = 16385
    g0, a0 = gradient(n, 7), gradient(n, 8)
    g0[5], g0[100], g0[16384], g0[9000] = np.inf, -np.inf, np.nan, np.nan
    a0[9000], a0[7] = 1.0, np.inf
    for with_acc in (False, True):
        (_, g), (_, a), (obuf, o) = guarded(g0), guarded(a0), guarded(np.zeros(n, np.float32))
        part = torch.zeros(ref.parts(n), dtype=torch.float64, device="cuda")
        run_accumulate(g, a if with_acc else None, o, 1.0 / 3.0, part)
        got, want = o.cpu().numpy(), ref.accumulate(g0, a0 if with_acc else None, 1.0 / 3.0)
        nan = np.isnan(want)
        assert nan.sum() == 2 and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan]))
        assert np.isposinf(got[5]) and np.isneginf(got[100]) and (not with_acc or np.isposinf(got[7]))
        assert bool((obuf[n:] == GUARD).all())
        assert np.array_equal(part.cpu().numpy(), run_sqnorm(g).cpu().numpy()[:-2], equal_nan=True)


def exact_gradient(n, seed):
    """gradients on which the kernel's fp32 steps are exact: k * 2^e with integers |k| <= 15 and e in -2 .. 2.  A square is a multiple
    of 2^-4 below 2^12, a thread's sum of 64 of them a multiple of 2^-4 below 2^18: 22 significant bits, no fp32 rounding anywhere"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-15, 16, n) * 2.0 ** rng.integers(-2, 3, n)).astype(np.float32)


def test_partials_against_fp64():
    """Against numpy fp64 the partials stay within rtol(numel) = numel * 2^-53, the bound tests/test_gpu_grad_log.py applies to sums
    of that length.  That bound's premise is that every TERM is exact and only the order of the additions differs.  The partials
    are s2f_grad_sqnorm's bits (asserted above), and that kernel squares and adds 64 values per thread in fp32: on gradients of
    arbitrary mantissas its error is of the order of 2^-24 (test_partials_against_fp64_by_the_fp32_bound measures that), and no
    kernel that keeps s2f_grad_sqnorm's bits can do better.  So the premise is met by the data: on `exact_gradient` no fp32 step
    rounds, only the order differs, and the bound checks what it checks in the gradient log's test -- that every element enters
    exactly one partial exactly once, at every size, tail and run boundary of SIZES."""
    worst = {}
    for n in SIZES:
        for err, exact, numel in partial_errors(n, exact_gradient):
            assert err <= rtol(numel) * exact, (n, err, exact)
            worst[n] = max(worst.get(n, 0.0), err)
    print("largest absolute error of a partial per n:", worst)


def partial_errors(n, make, cache={}):
    """[(absolute error of partial i against numpy fp64, the fp64 sum, elements of run i)] of the accumulate launch over make(n, n)"""
    if (n, make) not in cache:
        g0 = make(n, n)
        _, g = guarded(g0)
        part = torch.zeros(ref.parts(n), dtype=torch.float64, device="cuda")
        run_accumulate(g, None, torch.empty_like(g), 0.5, part)
        got, out = part.cpu().numpy(), []
        for i in range(ref.parts(n)):
            run = g0[i * ref.RUN:(i + 1) * ref.RUN].astype(np.float64)
            exact = float(np.sum(run * run))
            out.append((abs(got[i] - exact), exact, len(run)))
        cache[(n, make)] = out
    return cache[(n, make)]


def test_partials_against_fp64_by_the_fp32_bound():
    """The bound the arithmetic of s2f_grad_sqnorm does keep, derived: every term fl(x * x) is off by at most u = 2^-24 relative;
    a thread adds at most 64 of them, all non-negative, in fp32 in sequence -- 63 additions, each off by at most u of a partial sum
    that never exceeds the total: (1 + u)^64 - 1 < 65 u relative on a thread's sum, hence on the partial (a sum of non-negative
    thread sums; the fp64 tree adds 8 roundings of 2^-53, far below one u)."""
    worst = 0.0
    for n in SIZES:
        for err, exact, _ in partial_errors(n, gradient):
            assert err <= 65 * 2.0 ** -24 * exact, (n, err, exact)
            worst = max(worst, err / exact)
    print("largest relative error of a partial on gradients of arbitrary mantissas:", worst)


# ---------------------------------------------------------------------------------------------------- the stats kernel
@pytest.mark.parametrize("nparts", [1, 255, 256, 257, 2101])
@pytest.mark.parametrize("rows", [1, 3])
def test_stats_equal_the_restatement_by_bits(rows, nparts):
    from spike2former_amd._lib import check, lib
    from spike2former_amd.ops.core import _stream
    rng = np.random.default_rng(100 * rows + nparts)
    micro = rng.random((rows, nparts)) * 10.0 ** rng.uniform(-6, 12, (rows, nparts))
    accum = rng.random(nparts) * 10.0 ** rng.uniform(-6, 12, nparts)
    d_micro, d_accum = torch.from_numpy(micro).cuda(), torch.from_numpy(accum).cuda()
    stats = torch.full((6,), GUARD, dtype=torch.float32, device="cuda")
    for _ in range(2):          # bit-repeatable
        check(lib.s2f_grad_accum_stats(d_micro.data_ptr(), rows, d_accum.data_ptr(), nparts, stats.data_ptr(), _stream()),
              "s2f_grad_accum_stats")
        got = stats.cpu().numpy()
        assert np.array_equal(bits(got[:4]), bits(ref.stats(micro, accum))) and (got[4:] == GUARD).all()
    assert got[2] == rows and got[3] == 0.0


# ---------------------------------------------------------------------------------------------------- the captured step
recipes = dict(acc2=dict(counts=2), plain=dict(step_optimizer=False, log=False), one=dict(counts=1, log=False),
               none=dict(log=False), acc3=dict(counts=3, grad_log=dict(window=8, patience=200)))
rigs = rigs_fixture(recipes)


@pytest.fixture(scope="module")
def two_calls(rigs):
    """the accumulating rig's two calls on two batches, instrumented: a spy in front of `accum.add` copies the micro-batch gradient
    the step has just packed (a device-to-device copy on the step's stream: nothing waits) -> (state, [g1, g2], final flat, stats)"""
    r = rigs("acc2")
    reset(r)
    assert r.opt.accum is not None and r.step.log_captured is False and r.step.two_graphs is False
    accum, seen = r.opt.accum, []
    add = accum.add

    def spy():
        seen.append(r.red.flat.clone())
        return add()
    accum.add = spy
    versions = [p._version for p in r.opt.params]
    try:
        for it in range(2):
            feed(r, rigs.batches[it])
            r.step()
            if it == 0:          # no update behind the first call: the weights are untouched, their versions too
                assert [p._version for p in r.opt.params] == versions
            r.sched.step()
    finally:
        accum.add = add
    state = state_of(r)
    assert [p._version for p in r.opt.params] != versions and accum.count == 2
    return types.SimpleNamespace(state=state, grads=seen, flat=r.red.flat.clone(), stats=accum.stats.cpu().numpy(),
                                 norm=float(r.opt.grad_norm), log=r.log.read())


def test_captured_accumulation_oracle_a(rigs, two_calls):
    """Oracle A: the plain step (no optimizer) on batch 1, copy flat; on batch 2, copy flat; flat = fl(fl(0.5 g1) + fl(0.5 g2)) with
    torch fp32 ops; an eager FlatAdamW.step().  Bit-equal weights and moments -- IF the step is bit-repeatable from replay to
    replay, which is measured first (two replays of the plain step from the same state on the same input); if that gap of the flat
    gradient is not zero, twice the gap is the bound, and the gap is printed (DESIGN.md section 9 records it)."""
    p = rigs("plain")
    flats = []
    for _ in range(2):
        reset(p)
        feed(p, rigs.batches[0])
        p.step()
        flats.append(p.red.flat.clone())
    gap = float((flats[0].double() - flats[1].double()).abs().max())
    print("replay-to-replay gap of the plain step's flat gradient:", gap, "of max |g|", float(flats[0].abs().max()))
    reset(p)
    grads = []
    for it in range(2):
        feed(p, rigs.batches[it])
        p.step()
        grads.append(p.red.flat.clone())
        if it == 0:
            p.sched.step()
    p.red.flat.copy_(grads[0] * 0.5 + grads[1] * 0.5)
    p.opt.step()
    p.sched.step()
    want, got = state_of(p), two_calls.state
    worst = gaps(got, want)
    print("largest |captured accumulation - oracle A| per kind of tensor:", worst)
    assert float(got["step:"]) == 1.0 and float(want["step:"]) == 1.0
    for k in want:
        if gap == 0.0:
            assert torch.equal(got[k], want[k]), k
        elif want[k].numel():
            assert float((got[k].double() - want[k].double()).abs().max()) <= 2.0 * gap, k
    # what the accumulating rig computed from ITS OWN two gradients is exact: flat, the micro partials' mean and the norm
    g1, g2 = (g.cpu().numpy() for g in two_calls.grads)
    flat = ref.accumulate(g2, ref.accumulate(g1, None, 0.5), 0.5)
    assert np.array_equal(bits(two_calls.flat.cpu().numpy()), bits(flat))
    stats = ref.stats(np.stack([ref.sq_partials(g1), ref.sq_partials(g2)]), ref.sq_partials(flat))
    assert np.array_equal(bits(two_calls.stats), bits(stats))
    assert two_calls.norm == float(np.float32(np.sqrt(ref.ordered_sum(ref.sq_partials(flat)))))
    # the log: one row per call; the first one's update terms are the zeros of "no update yet", the second one's the update's
    read = two_calls.log
    assert read.names[-5:] == ["loss", "grad_norm", "clip_coef", "grad_sq_micro", "grad_sq_accum"] and read.count == 2
    assert (read.rows[0, -4:] == 0).all() and read.rows[1, -4] == np.float32(two_calls.norm)
    assert read.rows[1, -2] == stats[0] and read.rows[1, -1] == stats[1] and np.isfinite(read.rows).all()


def test_captured_accumulation_oracle_b(rigs, two_calls):
    """Oracle B: the same two iterations through OptimWrapper(accumulative_counts=2), the eager torch path (torch's clip_grad_norm_
    and AdamW, one group per parameter): each micro-batch gradient of the accumulating rig enters as the gradient of the linear
    loss sum <p, g>, which `update_params` scales and autograd accumulates.  Bound: tests/test_gpu_round5.py's for FlatAdamW against
    torch.optim.AdamW."""
    from spike2former_amd.train import LinearThenPoly, OptimWrapper
    r = rigs("acc2")

    class Bag(torch.nn.Module):          # the rig's parameters at their start, under their names ('.' is not allowed in one)
        def __init__(self):
            super().__init__()
            for g, p in zip(r.opt.param_groups, r.opt.params):
                self.register_parameter(g["name"].replace(".", "/"), torch.nn.Parameter(r.sd0[g["name"]].clone()))
    bag = Bag()
    wrap = OptimWrapper(bag, dict(type="AdamW", lr=0.001, betas=(0.9, 0.999), weight_decay=0.005), clip_grad=CLIP,
                        paramwise_cfg=dict(custom_keys={"backbone": dict(lr_mult=0.1, decay_mult=1.0)}), accumulative_counts=2)
    wrap.initialize_count_status(None)
    sched = LinearThenPoly(wrap.optimizer, warmup=4, total=20, start_factor=0.1)
    params = list(bag.parameters())
    skipped = set(r.red.missing)          # parameters the step gives no gradient: FlatAdamW skips them, as torch does for grad None
    norms = []
    for flat in two_calls.grads:
        views = [flat[off:off + p.numel()].view_as(p) for p, off in zip(r.opt.params, r.red.offsets)]
        norms.append(wrap.update_params(sum((p * g).sum() for i, (p, g) in enumerate(zip(params, views)) if i not in skipped)))
        sched.step()
    assert norms[0] is None and abs(float(norms[1]) - two_calls.norm) <= 1e-6 * float(norms[1])
    moved = 0
    for g, q in zip(r.opt.param_groups, params):
        got = two_calls.state[f"model:{g['name']}"]
        q = q.detach()
        assert float((got - q).abs().max()) <= 1e-6 * max(float(q.abs().max()), 1e-3), g["name"]
        moved += int(not torch.equal(q.detach(), r.sd0[g["name"]]))
    assert moved > len(params) // 2


def test_counts_one_allocates_nothing(rigs):
    one, none = rigs("one"), rigs("none")
    assert one.opt.accum is None and none.opt.accum is None
    assert one.step.optimizer is one.opt and one.step.accum is None and one.step._update_in_graph()


def test_counts_one_updates_bit_equal_from_equal_gradients():
    """what the C1_64 comparison below cannot show, because that step's backward is not bit-repeatable: from the SAME gradients,
    three updates of FlatAdamW(accumulative_counts=1) leave the bits of FlatAdamW without the argument"""
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.train import FlatAdamW, LinearThenPoly

    def toy():
        g = torch.Generator().manual_seed(0)
        return torch.nn.ParameterDict({"backbone_a": torch.nn.Parameter(torch.randn(3, 4099, generator=g)),
                                       "head": torch.nn.Parameter(torch.randn(130, 66, generator=g)),
                                       "scalar": torch.nn.Parameter(torch.randn(1, generator=g))}).cuda()
    sides = []
    for extra in ({}, dict(accumulative_counts=1)):
        m = toy()
        red = FlatGradAllReduce(m.parameters(), 1)
        opt = FlatAdamW(m, red, lr=0.001, weight_decay=0.005, clip_grad=CLIP,
                        paramwise_cfg=dict(custom_keys={"backbone": dict(lr_mult=0.1, decay_mult=1.0)}), **extra)
        sched = LinearThenPoly(opt, warmup=2, total=10, start_factor=0.1)
        g = torch.Generator(device="cuda").manual_seed(5)
        for it in range(3):
            for p in m.parameters():
                p.grad = torch.randn(p.shape, device="cuda", generator=g) * 10.0 ** (it - 1)
            red.gather()
            opt.step()
            sched.step()
        assert opt.accum is None
        sides.append([p.detach().clone() for p in m.parameters()] + [opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.state.clone()])
    for a, b in zip(*sides):
        assert torch.equal(a, b)


def test_counts_one_is_the_step_without_the_argument():
    """Three iterations of the captured step (GraphedStep with the update inside the graph) leave weights and moments BIT-equal to
    a rig built without the argument.  Bit equality between two rigs presupposes a step that repeats itself bit for bit, which
    the C1_64 step does not (fp32 atomics in its backward: the rig built without the argument differs from ITSELF by 1.2e-7 ..
    2.4e-7 on the weights after three iterations), so the rigs here are built over a model without
    atomics -- and the premise is asserted first: the rig without the argument, run twice, equals itself."""
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.graph import GraphedStep
    from spike2former_amd.train import FlatAdamW, LinearThenPoly
    g = torch.Generator().manual_seed(6)
    inputs = [torch.randn(2, 3, 33, 35, generator=g).cuda() for _ in range(3)]

    def rig(**extra):
        m = Elementwise().cuda()
        red = FlatGradAllReduce(m.parameters(), 1)
        opt = FlatAdamW(m, red, lr=0.001, weight_decay=0.005, clip_grad=CLIP,
                        paramwise_cfg=dict(custom_keys={"backbone": dict(lr_mult=0.1, decay_mult=1.0)}), **extra)
        sched = LinearThenPoly(opt, warmup=2, total=10, start_factor=0.1)
        start = {k: v.clone() for k, v in m.state_dict().items()}
        step = GraphedStep(m, lambda y: (y * y).mean(), inputs[0], grad_buffer=red, warmup=1, optimizer=opt)
        assert opt.accum is None and step.accum is None

        def run():
            m.load_state_dict(start)
            opt.exp_avg.zero_(), opt.exp_avg_sq.zero_(), opt.state.zero_()
            sched.t = 0
            sched._apply()
            opt.mark_updated()
            losses = []
            for x in inputs:
                losses.append(step(x).clone())
                sched.step()
            torch.cuda.synchronize()
            return [p.detach().clone() for p in m.parameters()] + [opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.state.clone()] + losses
        return run, start
    none, start = rig()
    one, _ = rig(accumulative_counts=1)
    a, a2, b = none(), none(), one()
    assert float(a[5][4]) == 3.0 and not torch.equal(a[0], start["backbone_w"]) and len({float(v) for v in a[-3:]}) == 3
    for x, y in zip(a, a2):          # the premise: this step repeats itself
        assert torch.equal(x, y)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------- the loop
def test_train_loop_counts_3_over_7_iterations(rigs, tmp_path):
    r = rigs("acc3")
    reset(r)
    r.opt.grad_log.clear()
    hooks = [dict(type="LoggerHook", interval=3, window_size=2)]
    loop = new_loop(r, rigs.batches, 7, hooks, work_dir=str(tmp_path))
    rows0 = loop.log.read().count
    loop.run()
    torch.cuda.synchronize()
    assert float(r.opt.state[4]) == 3.0 and r.sched.t == 7 and r.opt.accum.count == 7 and r.opt.accum.total == 7
    read = r.log.read()
    assert read.count - rows0 == 7 and len(read.rows) >= 7
    rows = read.rows[-7:]
    norm = rows[:, read.names.index("grad_norm")]
    assert [i + 1 for i in range(7) if norm[i] != (norm[i - 1] if i else 0.0)] == [3, 6, 7], norm
    glog = r.opt.grad_log.read(consume=False)
    assert glog.count == 3 and r.opt.grad_log.base == 0
    with open(tmp_path / "vis_data" / "scalars.json") as f:
        lines = [json.loads(line) for line in f]
    assert [rec["iter"] for rec in lines] == [3, 6, 7]
    jm, jM = read.names.index("grad_sq_micro"), read.names.index("grad_sq_accum")
    seen = 0
    for rec, at in zip(lines, ([2], [5], [6])):          # the update rows since the last line
        assert rec["grad/accum"] == 3 and "grad_sq_micro" not in rec and "grad_sq_accum" not in rec and "clip_coef" not in rec
        m, M = (float(np.mean(rows[at, j].astype(np.float64))) for j in (jm, jM))
        want = ref.noise_scale(m, M, 2, 6)[0]
        assert rec.get("grad/noise_scale") == want, (rec, m, M, want)
        seen += want is not None
    print("grad/noise_scale in", seen, "of 3 lines:", [rec.get("grad/noise_scale") for rec in lines])
    with open(tmp_path / "vis_data" / "grad.jsonl") as f:
        assert [json.loads(line)["iter"] for line in f] == [3, 6, 7]          # named after the update's iteration
    # the trailing group is ONE micro-batch at full weight: its two |g|^2 are the same number
    assert rows[6, jm] == rows[6, jM] and rows[6, jm] > 0


def test_resume_on_a_group_boundary_continues_the_run(rigs, tmp_path):
    """tests/test_gpu_train_loop.py's continuation pattern: A, A' -- seven iterations twice from the same state, uninterrupted; d0,
    their largest difference per kind of tensor, is the run-to-run spread.  B: six iterations (two groups), a checkpoint, the rig
    put somewhere else, resumed, the seventh iteration (a trailing group of one).  |B - A| <= 4 d0, bit equality where d0 = 0."""
    r = rigs("acc3")
    runs = []
    for _ in range(2):
        reset(r)
        new_loop(r, rigs.batches, 7).run()
        runs.append(state_of(r))
    a = runs[0]
    d0 = gaps(a, runs[1])
    print("d0 (A against A'):", d0)
    reset(r)
    hooks = [dict(type="CheckpointHook", interval=3)]
    new_loop(r, rigs.batches, 6, hooks, work_dir=str(tmp_path)).run()
    assert open(tmp_path / "last_checkpoint").read() == str(tmp_path / "iter_6.pth")
    scramble(r)
    loop = new_loop(r, rigs.batches, 7, hooks, work_dir=str(tmp_path), resume=True)
    loop.run()
    assert loop.resumed["meta"]["iter"] == 6 and r.opt.accum.count == 7
    b = state_of(r)
    worst = gaps(b, a)
    print("largest |B - A|:", worst)
    for k in a:
        if a[k].numel():
            kind = next(x for x in KINDS if k.startswith(x))
            assert float((b[k].double() - a[k].double()).abs().max()) <= 4.0 * d0[kind], (k, d0[kind])
    assert float(b["step:"]) == 3.0 and r.sched.t == 7
    # a file inside a group cannot be resumed from
    bad = new_loop(r, rigs.batches, 9, [], work_dir=str(tmp_path), load_from=str(tmp_path / "iter_7.pth"), resume=True)
    with pytest.raises(ValueError, match="inside a group"):
        bad.run()


def test_two_ranks_reduce_once_per_group(tmp_path):
    """two fresh child processes (torch.distributed.run, gloo, both on GPU 0) run tests/_accum_dist_worker.py: four iterations at
    accumulative_counts=2 -- two all-reduces and two updates per rank, bit-equal weights on both ranks"""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, S2F_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "_accum_dist_worker.py"), str(tmp_path)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)      # children only: nothing is re-exec'ed
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "RANK 0 OK" in r.stdout and "RANK 1 OK" in r.stdout, r.stdout[-2000:]
