"""CPU: the weight average without a GPU -- the momentum table against the formula, the copy / skip / lerp rule against two
restatements of mmengine's, the argument errors, the registry, tests/ema_ref.py's lerp against torch's, the ABI rows, and
WeightEMA / EMAHook / TrainState / TrainLoop driven by a fake step over the torch routes of ops.ema_update / ops.ema_swap."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_ref as ref          # noqa: E402

P = 1 << 20          # a 16-byte aligned dummy address: never dereferenced on the host


# ---------------------------------------------------------------------------------------------------- ABI
def test_abi_rows_and_argument_errors():
    from spike2former_amd import _lib
    lib = _lib.lib
    assert lib.s2f_version() >= 52
    assert len(_lib.SIGNATURES["s2f_ema_update"][1]) == 11 and len(_lib.SIGNATURES["s2f_ema_swap"][1]) == 5
    ok = [P, P, 1, P, P, P, 1, 0, 1, None, None]
    for i in (0, 1, 3, 4, 5):
        args = list(ok)
        args[i] = None
        assert lib.s2f_ema_update(*args) == -1 and b"null" in lib.s2f_last_error()
    for i, v, word in ((2, 0, b"no chunks"), (6, 0, b"table"), (7, -1, b"begin"), (8, 0, b"interval")):
        args = list(ok)
        args[i] = v
        assert lib.s2f_ema_update(*args) == -1 and word in lib.s2f_last_error(), word
    args = list(ok)
    args[3] = P + 4
    assert lib.s2f_ema_update(*args) == -2 and b"aligned" in lib.s2f_last_error()
    args = list(ok)
    args[9] = P + 4
    assert lib.s2f_ema_update(*args) == -2 and b"partials" in lib.s2f_last_error()
    assert lib.s2f_ema_swap(None, P, 1, P, None) == -1 and lib.s2f_ema_swap(P, P, 0, P, None) == -1
    assert lib.s2f_ema_swap(P, P, 1, P + 8, None) == -2
    from spike2former_amd import ops
    assert callable(ops.ema_update) and callable(ops.ema_swap)


# ---------------------------------------------------------------------------------------------------- the schedule
@pytest.mark.parametrize("kind,base,gamma", [("ExponentialMovingAverage", 0.0002, 2000), ("ExponentialMovingAverage", 0.25, 7),
                                             ("ExpMomentumEMA", 0.0002, 2000), ("ExpMomentumEMA", 0.01, 3), ("ExpMomentumEMA", 0.5, 100)])
def test_table_is_the_formula(kind, base, gamma):
    from spike2former_amd.ema import momentum_table
    got = momentum_table(kind, base, gamma)
    assert got.dtype == np.float32 and got.ndim == 1
    want = np.array([ref.momentum(kind, base, gamma, c) for c in range(len(got))], dtype=np.float32)
    assert np.array_equal(ref.bits(got), ref.bits(want))
    assert np.array_equal(ref.bits(got), ref.bits(ref.table(kind, base, gamma)))
    if kind == "ExponentialMovingAverage":
        assert len(got) == 1 and got[0] == np.float32(base)


@pytest.mark.parametrize("base,gamma", [(0.0002, 2000), (0.01, 3), (0.5, 100)])
def test_table_ends_where_fp32_stops_changing(base, gamma):
    from spike2former_amd.ema import momentum_table
    got = momentum_table("ExpMomentumEMA", base, gamma)
    n = len(got)
    assert got[-1] == np.float32(base) and (n == 1 or got[-2] != got[-1])
    assert (np.diff(got.astype(np.float64)) <= 0).all()          # falls, never rises
    for c in (n, n + 1, 2 * n, 100 * n):          # every later entry is the last one
        assert ref.momentum("ExpMomentumEMA", base, gamma, c) == got[-1]
    # the issue's "roughly gamma * ln((1 - m) * 2^25 / m)": the half-ulp of m taken as m * 2^-25.  It lies between m * 2^-25 and
    # m * 2^-24, so the table is no shorter than the estimate less gamma * ln 2; how much LONGER depends on where the fp64 m lies
    # between its fp32 neighbours (the term has to fall below half an ulp less that offset): a factor 16 is allowed for it
    est = gamma * math.log((1.0 - base) * 2.0 ** 25 / base)
    assert est - gamma * math.log(2.0) - 2 <= n <= est + gamma * math.log(16.0) + 2, (n, est)


def test_default_table_length():
    from spike2former_amd.ema import momentum_table
    n = len(momentum_table("ExpMomentumEMA", 0.0002, 2000))
    assert 40000 < n < 60000, n


# ---------------------------------------------------------------------------------------------------- the rule
def mmengine_actions(updates, begin_iter, interval):
    """EMAHook.after_train_iter + BaseAveragedModel.update_parameters, as code with mmengine's own counter"""
    steps, out = 0, []
    for i in range(updates):          # runner.iter
        if i + 1 >= begin_iter:          # EMAHook._ema_started
            if steps == 0:
                out.append(("copy", 0))
            elif steps % interval == 0:
                out.append(("lerp", steps))
            else:
                out.append(("skip", steps))
            steps += 1
        else:
            out.append(("copy", None))          # ema_params.data.copy_(src_params.data)
    return out, steps


@pytest.mark.parametrize("interval", [1, 2])
@pytest.mark.parametrize("begin_iter", [0, 1, 3])
def test_the_first_12_decisions(begin_iter, interval):
    from spike2former_amd.ema import WeightEMA, ema_plan
    want, steps = mmengine_actions(12, begin_iter, interval)
    for t in range(1, 13):
        action, c = ema_plan(t, begin_iter, interval)
        assert (action, c) == ref.decide(t, begin_iter, interval)
        assert action == want[t - 1][0] and (want[t - 1][1] is None or want[t - 1][1] == c), (t, action, c, want[t - 1])
    assert WeightEMA.steps(type("E", (), dict(begin_iter=begin_iter))(), 12) == steps


def test_argument_errors():
    from spike2former_amd.ema import WeightEMA, momentum_table
    for m in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="momentum"):
            WeightEMA(None, momentum=m)
    with pytest.raises(NotImplementedError):
        WeightEMA(None, update_buffers=True)
    with pytest.raises(NotImplementedError):
        WeightEMA(None, begin_epoch=2)
    with pytest.raises(NotImplementedError):
        WeightEMA(None, type="StochasticWeightAverage")
    with pytest.raises(ValueError):
        WeightEMA(None, type="Median")
    with pytest.raises(ValueError):
        WeightEMA(None, interval=0)
    with pytest.raises(ValueError, match="entries"):
        momentum_table("ExpMomentumEMA", 0.0002, 1e6)          # ~2.6e7 entries
    assert len(momentum_table("ExpMomentumEMA", 0.0002, 1e5)) < 1 << 22          # ~2.6e6: still a table


def test_the_hook_is_registered():
    import spike2former_amd as s2f
    assert s2f.HOOKS.get("EMAHook") is s2f.EMAHook and s2f.WeightEMA is not None
    hook = s2f.HOOKS.build(dict(type="EMAHook", momentum=0.01))
    assert isinstance(hook, s2f.EMAHook) and hook.priority == 50
    assert hook.args == dict(type="ExponentialMovingAverage", momentum=0.01, gamma=2000.0, interval=1, begin_iter=0, update_buffers=False)
    hook = s2f.HOOKS.build(dict(type="EMAHook", ema_type="ExpMomentumEMA", momentum=0.0002, gamma=2000, begin_iter=5))
    assert hook.args["type"] == "ExpMomentumEMA" and hook.args["begin_iter"] == 5
    for bad, err in ((dict(update_buffers=True), NotImplementedError), (dict(begin_epoch=1), NotImplementedError),
                     (dict(ema_type="StochasticWeightAverage"), NotImplementedError), (dict(momentum=1.0), ValueError)):
        with pytest.raises(err):
            s2f.HOOKS.build(dict(type="EMAHook", **bad))


# ---------------------------------------------------------------------------------------------------- the lerp
def test_ref_lerp_against_torch():
    """tests/ema_ref.py's unfused lerp against torch.Tensor.lerp_ on the CPU: |p - e| from 2^-20 to 2^20.  torch evaluates
    e + m (p - e) (m < 0.5) or p - (p - e)(1 - m) in fp32, possibly fused: against the three separately rounded operations that is
    at most one rounding of the product and one of the sum apart, each at most half an ulp of a value no larger than
    max(|e|, |p|) (m <= 1: the product is no larger than |p - e| <= 2 max, its rounding error at most 2^-24 * 2 max; the sum lies
    between e and p) -- within 2^-23 * max(|e|, |p|) per element."""
    rng = np.random.default_rng(3)
    n = 1 << 16
    e = (rng.standard_normal(n) * 2.0 ** rng.uniform(-4, 20, n)).astype(np.float32)
    gap = (2.0 ** rng.uniform(-20, 20, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    p = (e + gap).astype(np.float32)
    seen = np.abs(p.astype(np.float64) - e.astype(np.float64))
    assert seen[seen > 0].min() <= 2.0 ** -19 and seen.max() >= 2.0 ** 19
    for m in (0.0002, 0.25, 0.5, 0.75, 0.999):
        got = ref.lerp(e, p, m)
        want = torch.from_numpy(e.copy()).lerp_(torch.from_numpy(p), float(np.float32(m))).numpy()
        bound = 2.0 ** -23 * np.maximum(np.abs(e), np.abs(p)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        assert (err <= bound).all(), (m, float((err / bound).max()))
    # exact cases: m = 0.5 between neighbours, e == p, and the one NaN
    assert ref.lerp(np.float32(1.0), np.float32(3.0), 0.5) == np.float32(2.0)
    assert np.array_equal(ref.bits(ref.lerp(e, e, 0.3)), ref.bits(e + np.float32(0)))
    odd = ref.lerp(np.array([np.inf, 1.0, np.nan], np.float32), np.array([np.inf, np.nan, 2.0], np.float32), 0.5)
    assert (ref.bits(odd) == 0x7FC00000).all()


# ---------------------------------------------------------------------------------------------------- the classes on a fake step
def make_rig(ema, seed=0):
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.train import FlatAdamW, LinearThenPoly
    torch.manual_seed(seed)
    model = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.BatchNorm1d(5))
    red = FlatGradAllReduce(model.parameters(), 1)
    opt = FlatAdamW(model, red, lr=0.01, **({} if ema is None else dict(ema=ema)))
    sched = LinearThenPoly(opt, warmup=2, total=50, start_factor=0.1)
    return model, opt, sched


class FakeAugment:
    def __init__(self, seed=0):
        self.rng = np.random.default_rng(seed)

    def __call__(self, images, segs, out=None):
        self.rng.random(3)


class FakeStep:
    """what the loop sees of a captured step with the update inside: the weights move, the optimizer's count advances, the
    average's launch follows -- and a log row"""

    def __init__(self, model, opt, log):
        self.model, self.optimizer, self.log, self.calls = model, opt, log, 0
        self.static_in, self.static_seg = torch.zeros(1), torch.zeros(1, dtype=torch.uint8)
        self.vals = {k: torch.ones(()) for k in ("loss_cls", "loss", "grad_norm", "clip_coef")}
        log.bind(self.vals)
        self.history = []          # the parameters after every update, as numpy

    def __call__(self):
        self.calls += 1
        with torch.no_grad():
            for i, p in enumerate(self.model.parameters()):
                p.mul_(1.0 + 0.1 * (i + 1)).add_(0.01 * self.calls)
            self.model[1].num_batches_tracked.add_(1)
        self.optimizer.state[4] += 1
        if self.optimizer.ema is not None:
            self.optimizer.ema.update()
        self.history.append([p.detach().numpy().copy() for p in self.optimizer.params])
        self.log.append()

    def check(self):
        pass


def make_loop(tmp_path, ema, hooks, max_iters, seed=0, **kw):
    import spike2former_amd as s2f
    model, opt, sched = make_rig(ema, seed)
    step = FakeStep(model, opt, s2f.TrainLog(window=16, device="cpu", capacity=8))
    return s2f.TrainLoop(step, opt, sched, FakeAugment(), [(None, None)] * 3, max_iters=max_iters, hooks=hooks,
                         work_dir=str(tmp_path), async_write=False, **kw)


def averaged(opt):
    return [opt.ema.ema[off:off + p.numel()].numpy().reshape(p.shape).copy() for p, off in zip(opt.params, opt.red.offsets)]


def replay(history, start, first_update, tab, begin_iter, interval):
    """ema_ref over the parameters read back after each update"""
    avg = [a.copy() for a in start]
    for k, params in enumerate(history):
        avg = [ref.update(e, p, first_update + k, tab, begin_iter, interval)[0] for e, p in zip(avg, params)]
    return avg


def test_without_the_argument_nothing_is_there():
    _, opt, _ = make_rig(None)
    assert opt.ema is None
    _, opt, _ = make_rig(False)
    assert opt.ema is None


@pytest.mark.parametrize("cfg", [dict(momentum=0.25, begin_iter=2), dict(type="ExpMomentumEMA", momentum=0.1, gamma=2, interval=2)])
def test_weight_ema_follows_the_restatement_on_the_torch_route(cfg, tmp_path):
    from spike2former_amd.ema import WeightEMA
    model, opt, _ = make_rig(cfg)
    ema = opt.ema
    assert isinstance(ema, WeightEMA) and ema.ema.shape == opt.exp_avg.shape and not ema.swapped
    start = [p.detach().numpy().copy() for p in opt.params]
    for a, b in zip(averaged(opt), start):          # starts as a copy
        assert np.array_equal(ref.bits(a), ref.bits(b))
    assert ema.report(0) == {}
    import spike2former_amd as s2f
    step = FakeStep(model, opt, s2f.TrainLog(window=4, device="cpu", capacity=8))
    tab = ref.table(cfg.get("type", "ExponentialMovingAverage"), cfg["momentum"], cfg.get("gamma", 2000))
    assert np.array_equal(ref.bits(ema.momenta), ref.bits(tab))
    for t in range(1, 8):
        step()
        want = replay(step.history, start, 1, tab, cfg.get("begin_iter", 0), cfg.get("interval", 1))
        for a, b in zip(averaged(opt), want):
            assert np.array_equal(ref.bits(a), ref.bits(b)), t
        rep = ema.report(t)
        action, c = ref.decide(t, cfg.get("begin_iter", 0), cfg.get("interval", 1))
        if action != "skip":
            parts = ref.drift_partials(step.history[-1], want, 4096)
            assert rep["ema/drift"] == pytest.approx(ref.drift(parts), rel=1e-12, abs=1e-300)
            assert rep["ema/momentum"] == (1.0 if action == "copy" else float(tab[min(c, len(tab) - 1)]))
    # swap: the average is in the model, the weights are in the buffer, and nothing else may happen until the way back
    train, avg = [p.detach().numpy().copy() for p in opt.params], averaged(opt)
    versions = [p._version for p in opt.params]
    ema.swap()
    assert ema.swapped and all(p._version > v for p, v in zip(opt.params, versions))
    for p, a, e, t in zip(opt.params, avg, averaged(opt), train):
        assert np.array_equal(ref.bits(p.detach().numpy()), ref.bits(a)) and np.array_equal(ref.bits(e), ref.bits(t))
    for call in (ema.update, ema.swap, ema.reset, ema.rebuild, s2f.TrainState(model, opt).snapshot):
        with pytest.raises(RuntimeError, match="swapped"):
            call()
    ema.restore()
    assert not ema.swapped
    for p, a, e, t in zip(opt.params, avg, averaged(opt), train):
        assert np.array_equal(ref.bits(p.detach().numpy()), ref.bits(t)) and np.array_equal(ref.bits(e), ref.bits(a))
    with pytest.raises(RuntimeError):
        ema.restore()


def test_the_hook_wants_the_optimizers_average(tmp_path):
    for ema in (None, dict(momentum=0.02)):
        loop = make_loop(tmp_path, ema, [dict(type="EMAHook", momentum=0.01)], 2)
        with pytest.raises(ValueError, match=r"FlatAdamW\(ema="):
            loop.run()
    make_loop(tmp_path, dict(momentum=0.01), [dict(type="EMAHook", momentum=0.01)], 2).run()
    make_loop(tmp_path, True, [dict(type="EMAHook")], 2).run()


def test_validation_sees_the_average_and_the_weights_come_back(tmp_path):
    cfg = dict(momentum=0.25, begin_iter=2)
    seen = []

    def validate():
        opt = loop.optimizer
        assert opt.ema.swapped
        seen.append([p.detach().numpy().copy() for p in opt.params])
        if len(seen) == 2:
            raise KeyError("validation failed")
        return dict(mIoU=float(len(seen)))
    hooks = [dict(type="EMAHook", **cfg), dict(type="LoggerHook", interval=3, window_size=2),
             dict(type="CheckpointHook", interval=3, save_best="mIoU")]
    loop = make_loop(tmp_path, cfg, hooks, 6, val_interval=3, validate=validate)
    start = [p.detach().numpy().copy() for p in loop.optimizer.params]
    with pytest.raises(KeyError, match="validation failed"):
        loop.run()
    opt, hist = loop.optimizer, loop.step.history
    assert len(hist) == 6 and len(seen) == 2 and not opt.ema.swapped
    tab = ref.table("ExponentialMovingAverage", 0.25)
    for k, n in enumerate((3, 6)):          # the closure saw the average of n updates
        for a, b in zip(seen[k], replay(hist[:n], start, 1, tab, 2, 1)):
            assert np.array_equal(ref.bits(a), ref.bits(b)), n
    for p, w in zip(opt.params, hist[-1]):          # the training weights are back, also behind the validation that raised
        assert np.array_equal(ref.bits(p.detach().numpy()), ref.bits(w))
    # the files: iter_3, best (after the first validation), iter_6
    names = [g["name"] for g in opt.param_groups]
    for fname, n in (("iter_3.pth", 3), ("best_mIoU_iter_3.pth", 3), ("iter_6.pth", 6)):
        ck = torch.load(tmp_path / fname, weights_only=True)
        assert list(ck["state_dict"]) == list(loop.step.model.state_dict())
        assert list(ck["ema_state_dict"]) == ["steps"] + [f"module.{k}" for k in ck["state_dict"]]
        assert int(ck["ema_state_dict"]["steps"]) == n - 1          # begin_iter 2: updates 2 .. n
        avg = replay(hist[:n], start, 1, tab, 2, 1)
        for name, a, w in zip(names, avg, hist[n - 1]):
            assert np.array_equal(ref.bits(ck["state_dict"][name].numpy()), ref.bits(a)), (fname, name)
            assert np.array_equal(ref.bits(ck["ema_state_dict"][f"module.{name}"].numpy()), ref.bits(w)), (fname, name)
        for k, v in ck["state_dict"].items():          # buffers: the training model's, in both
            if k not in names:
                assert torch.equal(v, ck["ema_state_dict"][f"module.{k}"])
    with open(tmp_path / "vis_data" / "scalars.json") as f:
        import json
        lines = [json.loads(line) for line in f]
    train = [rec for rec in lines if "lr" in rec]
    assert [rec["iter"] for rec in train] == [3, 6] and all(rec["ema/momentum"] == 0.25 and rec["ema/drift"] > 0 for rec in train)


def test_resume_restores_both_copies_and_load_from_reads_the_average(tmp_path):
    import spike2former_amd as s2f
    cfg = dict(type="ExpMomentumEMA", momentum=0.1, gamma=2)
    hooks = [dict(type="EMAHook", ema_type="ExpMomentumEMA", momentum=0.1, gamma=2), dict(type="CheckpointHook", interval=3)]
    whole = make_loop(tmp_path / "a", cfg, hooks, 6)
    whole.run()
    first = make_loop(tmp_path / "b", cfg, hooks, 3)
    first.run()
    second = make_loop(tmp_path / "b", cfg, hooks, 6, seed=5, resume=True)          # other weights: the file decides
    second.step.calls = 3          # (the fake step's own script position)
    second.run()
    for a, b in zip(whole.optimizer.params, second.optimizer.params):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(whole.optimizer.ema.ema.view(torch.int32), second.optimizer.ema.ema.view(torch.int32))
    assert float(second.optimizer.state[4]) == 6.0
    # load_from: the averaged weights, into a model without an optimizer and into a rig whose average then starts from them
    path = str(tmp_path / "a" / "iter_6.pth")
    avg = averaged(whole.optimizer)
    model, _, _ = make_rig(None, seed=9)
    s2f.TrainState(model, None).load(path)
    for p, a in zip(model.parameters(), avg):
        assert np.array_equal(ref.bits(p.detach().numpy()), ref.bits(a))
    model, opt, sched = make_rig(cfg, seed=9)
    s2f.TrainState(model, opt, sched).load(path)
    for p, a, e in zip(opt.params, avg, averaged(opt)):
        assert np.array_equal(ref.bits(p.detach().numpy()), ref.bits(a)) and np.array_equal(ref.bits(e), ref.bits(a))
    # a file of a run without an average resumes into a run with one: the average starts from the loaded weights
    plain = make_loop(tmp_path / "c", None, [dict(type="CheckpointHook", interval=3)], 3)
    plain.run()
    ck = torch.load(tmp_path / "c" / "iter_3.pth", weights_only=True)
    assert sorted(ck) == ["augment", "best", "meta", "optimizer", "param_schedulers", "state_dict"]          # the keys of today
    model, opt, sched = make_rig(cfg, seed=9)
    s2f.TrainState(model, opt, sched).load(str(tmp_path / "c" / "iter_3.pth"), resume=True)
    for p, w, e in zip(opt.params, plain.optimizer.params, averaged(opt)):
        assert torch.equal(p, w) and np.array_equal(ref.bits(e), ref.bits(w.detach().numpy()))


def test_rebuild_keeps_the_values_per_parameter():
    model, opt, _ = make_rig(dict(momentum=0.5))
    with torch.no_grad():
        for i, p in enumerate(opt.params):
            p.add_(float(i + 1))
    before = {id(p): a for p, a in zip(opt.params, averaged(opt))}          # the start's copy, not the weights of now
    opt.rebuild()
    assert opt.ema.ema.shape == opt.exp_avg.shape
    for p, a in zip(opt.params, averaged(opt)):
        assert np.array_equal(ref.bits(a), ref.bits(before[id(p)]))
    opt.state[4] = 1.0
    opt.ema.update()          # the tables fit again
