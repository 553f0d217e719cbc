"""CPU: gradient accumulation without a GPU -- the plan (train.GradAccum.plan) against a brute-force statement of mmengine's rule,
the two kernels' argument errors, OptimWrapper(accumulative_counts=2) against one step on the mean loss, the ValueErrors of
CheckpointHook and of a run resumed inside a group, and LoggerHook's noise-scale arithmetic on a hand-made LogRead."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accum_ref as ref          # noqa: E402

P = 1 << 20          # a 16-byte aligned dummy address: never dereferenced on the host


def fake_buffer(n=8):
    return types.SimpleNamespace(flat=torch.zeros(n))


# ---------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("counts,total", [(1, 5), (3, 7), (4, 8), (4, None), (5, 3)])
def test_plan_restates_the_rule(counts, total):
    from spike2former_amd.train import GradAccum
    acc = GradAccum(fake_buffer(), counts, total)
    for i in range(total if total is not None else 13):
        scale, first, last = acc.plan(i)
        want = ref.plan(i, counts, total)
        assert (first, last) == want[1:] and scale == want[0], (i, (scale, first, last), want)


def test_plan_of_counts_3_total_7():
    from spike2former_amd.train import GradAccum
    acc = GradAccum(fake_buffer(), 3, 7)
    plans = [acc.plan(i) for i in range(7)]
    assert [i + 1 for i, p in enumerate(plans) if p[2]] == [3, 6, 7]
    assert [i for i, p in enumerate(plans) if p[1]] == [0, 3, 6]
    assert [p[0] for p in plans] == [1 / 3] * 6 + [1.0]


def test_counts_below_one_and_the_default():
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.train import FlatAdamW, GradAccum, OptimWrapper
    for bad in (0, -2):
        with pytest.raises(ValueError):
            GradAccum(fake_buffer(), bad)
    m = torch.nn.Linear(3, 2)
    red = FlatGradAllReduce(m.parameters(), 1)
    assert FlatAdamW(m, red).accum is None and FlatAdamW(m, red, accumulative_counts=1).accum is None
    opt = FlatAdamW(m, red, accumulative_counts=3)
    assert isinstance(opt.accum, GradAccum) and opt.accum.counts == 3 and opt.accum.acc.shape == red.flat.shape
    assert opt.accum.micro.shape == (3, opt.partials.numel()) and opt.accum.micro.dtype == torch.float64
    assert opt.accum.stats.shape == (4,) and opt.accum.partials is opt.partials
    with pytest.raises(ValueError):
        FlatAdamW(m, red, accumulative_counts=0)
    with pytest.raises(ValueError):
        OptimWrapper(m, accumulative_counts=0)
    # rebuild only at a group boundary
    opt.accum.count = 4
    with pytest.raises(RuntimeError, match="inside a group"):
        opt.accum.rebuild()
    opt.accum.count = 6
    opt.accum.rebuild()


# ---------------------------------------------------------------------------------------------------- argument errors
def test_abi_rows():
    from spike2former_amd import _lib
    assert _lib.lib.s2f_version() >= 51
    assert len(_lib.SIGNATURES["s2f_grad_accumulate"][1]) == 7 and len(_lib.SIGNATURES["s2f_grad_accum_stats"][1]) == 6


def test_grad_accumulate_argument_errors():
    from spike2former_amd._lib import lib
    call = lib.s2f_grad_accumulate
    for args in ((None, P, P, 8, 0.5, P, None), (P, P, None, 8, 0.5, P, None), (None, None, None, 8, 0.5, None, None)):
        assert call(*args) == -1 and b"null" in lib.s2f_last_error()
    assert call(P, P, P, -1, 0.5, P, None) == -1 and b"n < 0" in lib.s2f_last_error()
    for off in (4, 8, 12):
        for args in ((P + off, P, P), (P, P + off, P), (P, P, P + off), (P + off, None, P)):
            assert call(*args, 8, 0.5, P, None) == -2 and b"aligned" in lib.s2f_last_error(), (off, args)
    assert call(P, P, P, 8, 0.5, P + 4, None) == -2 and b"8-byte" in lib.s2f_last_error()
    # nothing to do is no error, and no launch: with and without an accumulator, with and without partials
    assert call(P, P, P, 0, 0.5, P, None) == 0 and call(P, None, P, 0, 0.5, None, None) == 0


def test_grad_accum_stats_argument_errors():
    from spike2former_amd._lib import lib
    call = lib.s2f_grad_accum_stats
    for args in ((None, 1, P, 1, P, None), (P, 1, None, 1, P, None), (P, 1, P, 1, None, None)):
        assert call(*args) == -1 and b"null" in lib.s2f_last_error()
    for rows in (0, -1):
        assert call(P, rows, P, 1, P, None) == -1 and b"at least 1" in lib.s2f_last_error()
    for nparts in (0, -5):
        assert call(P, 1, P, nparts, P, None) == -1 and b"at least 1" in lib.s2f_last_error()


# ---------------------------------------------------------------------------------------------------- OptimWrapper
class TwoParameters(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(2)
        self.w = torch.nn.Parameter(torch.randn(7, 5, generator=g))
        self.b = torch.nn.Parameter(torch.randn(5, generator=g))

    def forward(self, x):
        return torch.tanh(x @ self.w + self.b).pow(2).mean()


def test_optim_wrapper_accumulates_like_one_step_on_the_mean_loss():
    """torch's own AdamW both ways: two update_params calls at accumulative_counts=2 against ONE step on (l1 + l2) / 2"""
    from spike2former_amd.train import OptimWrapper
    cfg = dict(type="AdamW", lr=0.01, betas=(0.9, 0.999), weight_decay=0.005)
    clip = dict(max_norm=0.01, norm_type=2)
    a, b = TwoParameters(), TwoParameters()
    acc, one = OptimWrapper(a, cfg, clip_grad=clip, accumulative_counts=2), OptimWrapper(b, cfg, clip_grad=clip)
    acc.initialize_count_status(4)
    g = torch.Generator().manual_seed(3)
    for _ in range(2):
        x1, x2 = torch.randn(9, 7, generator=g), torch.randn(9, 7, generator=g)
        before = [p.detach().clone() for p in a.parameters()]
        assert acc.update_params(a(x1)) is None
        assert all(torch.equal(p, q) for p, q in zip(a.parameters(), before)) and a.w.grad is not None          # no step, no zero_grad
        n1 = acc.update_params(a(x2))
        n2 = one.update_params(0.5 * (b(x1) + b(x2)))
        assert a.w.grad is None and abs(float(n1) - float(n2)) <= 1e-6 * float(n2)
        for p, q, p0 in zip(a.parameters(), b.parameters(), before):
            assert not torch.equal(p, p0)
            assert float((p - q).detach().abs().max()) <= 1e-7 * float(q.detach().abs().max())
    assert acc.count == 4
    # a trailing group of one: full weight, update at once
    c, d = TwoParameters(), TwoParameters()
    tail = OptimWrapper(c, cfg, accumulative_counts=2)
    tail.initialize_count_status(3, count=2)
    x = torch.randn(9, 7, generator=g)
    d(x).backward()
    seen = {}
    tail.optimizer.register_step_pre_hook(lambda *args: seen.update(g=c.w.grad.clone()))
    tail.update_params(c(x))
    assert torch.equal(seen["g"], d.w.grad) and c.w.grad is None


# ---------------------------------------------------------------------------------------------------- the loop's errors
class FakeStep:
    def __init__(self, model, optimizer, log):
        self.model, self.optimizer, self.log, self.calls = model, optimizer, log, 0
        self.static_in, self.static_seg = torch.zeros(2, 1), torch.zeros(1, dtype=torch.uint8)
        self.vals = {k: torch.zeros(()) for k in ("loss", "grad_norm", "clip_coef", "grad_sq_micro", "grad_sq_accum")}
        self.log_captured = False
        log.bind(self.vals)

    def __call__(self):
        self.optimizer.accum.count += 1          # (what accum.add() does on the host)
        self.log.append()
        self.calls += 1


class FakeAugment:
    def __init__(self):
        self.rng = np.random.default_rng(0)

    def __call__(self, images, segs, out=None):
        pass


def make_loop(tmp_path, counts, max_iters, hooks, **kw):
    import spike2former_amd as s2f
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.train import FlatAdamW, LinearThenPoly
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.BatchNorm1d(5))
    red = FlatGradAllReduce(model.parameters(), 1)
    opt = FlatAdamW(model, red, lr=0.01, accumulative_counts=counts)
    sched = LinearThenPoly(opt, warmup=2, total=50, start_factor=0.1)
    step = FakeStep(model, opt, s2f.TrainLog(window=16, device="cpu", capacity=8))
    return s2f.TrainLoop(step, opt, sched, FakeAugment(), [(None, None)], max_iters=max_iters, hooks=hooks, work_dir=str(tmp_path), **kw)


def test_checkpoint_interval_must_be_a_multiple_of_the_count(tmp_path):
    loop = make_loop(tmp_path, 3, 6, [dict(type="CheckpointHook", interval=4)])
    with pytest.raises(ValueError, match="multiple of accumulative_counts=3"):
        loop.run()
    assert loop.step.calls == 0
    loop = make_loop(tmp_path, 3, 7, [dict(type="CheckpointHook", interval=3)])
    loop.run()
    assert loop.accum.total == 7 and loop.accum.count == 7 and loop.scheduler.t == 7          # the scheduler steps every iteration
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".pth")) == ["iter_3.pth", "iter_6.pth", "iter_7.pth"]
    assert loop.update_iteration(1) == 3 and loop.update_iteration(2) == 6 and loop.update_iteration(3) == 7


def test_a_run_resumed_inside_a_group_raises(tmp_path):
    make_loop(tmp_path, 2, 3, [dict(type="CheckpointHook", interval=2)]).run()          # files of iterations 2 and 3 (the last)
    again = make_loop(tmp_path, 2, 6, [], resume=True)          # last_checkpoint names iteration 3: inside the group {2, 3}
    with pytest.raises(ValueError, match="inside a group"):
        again.run()
    assert again.step.calls == 0
    ok = make_loop(tmp_path, 2, 6, [], load_from=str(tmp_path / "iter_2.pth"), resume=True)
    ok.run()
    assert ok.step.calls == 4 and ok.accum.count == 6


def test_the_optimizer_has_to_be_the_steps_own(tmp_path):
    import spike2former_amd as s2f
    loop = make_loop(tmp_path, 2, 2, [])
    loop.step.optimizer = None
    with pytest.raises(ValueError, match="step's own"):
        s2f.TrainLoop(loop.step, loop.optimizer, loop.scheduler, loop.augment, [(None, None)], max_iters=2)


# ---------------------------------------------------------------------------------------------------- the log line
def test_logger_hook_noise_scale_arithmetic():
    import spike2former_amd as s2f
    from spike2former_amd.runner import LogRead, noise_scale
    names = ["loss", "grad_norm", "clip_coef", "grad_sq_micro", "grad_sq_accum"]
    rng = np.random.default_rng(4)
    rows = rng.random((8, 5)).astype(np.float32)
    rows[:, 3] += 2.0          # micro-batch |g|^2 above the accumulated one's: a positive noise term ...
    rows[:, 4] += 1.0          # ... and the accumulated one's above its share of it: a positive estimate of |G|^2 in every row
    counts, b, world = 3, 2, 2
    loop = types.SimpleNamespace(accum=types.SimpleNamespace(counts=counts), max_iters=20, world=world,
                                 step=types.SimpleNamespace(static_in=torch.zeros(b, 3, 4, 4)))
    hook = s2f.LoggerHook(interval=5, window_size=2)
    assert set(hook.HIDDEN) >= {"clip_coef", "grad_sq_micro", "grad_sq_accum"}
    # the line of iteration 10, the last one at 5: the ring holds iterations 3 .. 10, the updates since the last line are 6 and 9
    hook._last = 5
    record = {}
    hook._accum(loop, 10, LogRead(names, rows, 10, None), record)
    at = [3, 6]          # rows of iterations 6 and 9
    m, M = (float(np.mean(rows[at, j].astype(np.float64))) for j in (3, 4))
    want = ref.noise_scale(m, M, b, counts * b * world)
    assert record["grad/accum"] == 3 and want[0] is not None and record["grad/noise_scale"] == want[0]
    assert noise_scale(m, M, b, counts * b * world) == want
    # the ratio of the means, not the mean of the ratios
    each = [ref.noise_scale(float(rows[i, 3]), float(rows[i, 4]), b, counts * b * world)[0] for i in at]
    assert record["grad/noise_scale"] != float(np.mean(each))
    # the trailing group's update (iteration 20 = max_iters, not a multiple of 3) counts; one that the ring has lost does not
    hook._last = 18
    record = {}
    hook._accum(loop, 20, LogRead(names, rows[:2], 20, None), record)
    assert record["grad/noise_scale"] == ref.noise_scale(float(rows[1, 3]), float(rows[1, 4]), b, counts * b * world)[0]
    hook._last = 15
    record = {}
    hook._accum(loop, 17, LogRead(names, rows[:2], 17, None), record)          # iterations 16, 17: no update in reach
    assert record == {"grad/accum": 3}
    # G2 <= 0: omitted
    small = rows.copy()
    small[:, 4] = 0.0
    hook._last = 5
    record = {}
    hook._accum(loop, 10, LogRead(names, small, 10, None), record)
    assert record == {"grad/accum": 3}
    # an identity of the estimate: gradients that are pure noise around G with per-image covariance trace S
    G2, S = 0.7, 5.0
    got = ref.noise_scale(G2 + S / 2, G2 + S / 12, 2, 12)
    assert got[0] == pytest.approx(S / G2, rel=1e-12) and got[1] == pytest.approx(G2, rel=1e-12)
