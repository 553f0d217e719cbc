"""CPU: the training loop's pieces without a GPU -- the two new ABI rows and their argument errors, the torch routes of
ops.state_copy / ops.train_log_append against plain indexing, and LoggerHook / CheckpointHook / TrainState driven by a fake step
with scripted losses (runner.py)."""
import json
import logging
import os

import numpy as np
import pytest
import torch

P = 1 << 20          # a 16-byte aligned dummy address: never dereferenced on the host


# ---------------------------------------------------------------------------------------------------- ABI
def test_abi_rows():
    from spike2former_amd import _lib
    assert _lib.lib.s2f_version() >= 44
    assert len(_lib.SIGNATURES["s2f_state_copy"][1]) == 6 and len(_lib.SIGNATURES["s2f_train_log_append"][1]) == 7
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s2f.h")).read()
    assert "#define S2F_TRAIN_LOG_MAX_TERMS 256" in src
    from spike2former_amd import ops
    assert ops.TRAIN_LOG_MAX_TERMS == 256


def test_state_copy_argument_errors():
    from spike2former_amd._lib import lib
    for args in ((None, P, 1, P, 0, None), (P, None, 1, P, 0, None), (P, P, 1, None, 0, None)):
        assert lib.s2f_state_copy(*args) == -1 and b"null" in lib.s2f_last_error()
    for n in (0, -3):
        assert lib.s2f_state_copy(P, P, n, P, 0, None) == -1 and b"no chunks" in lib.s2f_last_error()
    for t in (2, -1):
        assert lib.s2f_state_copy(P, P, 1, P, t, None) == -1 and b"to_params" in lib.s2f_last_error()
    for off in (4, 8, 12):
        assert lib.s2f_state_copy(P, P, 1, P + off, 1, None) == -2 and b"aligned" in lib.s2f_last_error()


def test_train_log_append_argument_errors():
    from spike2former_amd._lib import lib
    call = lib.s2f_train_log_append
    for args in ((None, 1, P, 1, 1, P, None), (P, 1, None, 1, 1, P, None), (P, 1, P, 1, 1, None, None)):
        assert call(*args) == -1 and b"null" in lib.s2f_last_error()
    for n in (0, -1, 257):
        assert call(P, n, P, 4, 300, P, None) == -1 and b"outside 1 .. 256" in lib.s2f_last_error()
    assert call(P, 5, P, 4, 4, P, None) == -1 and b"stride" in lib.s2f_last_error()
    assert call(P, 5, P, 0, 5, P, None) == -1 and b"window" in lib.s2f_last_error()
    assert call(P, 5, P, 2, 5, P + 4, None) == -2 and call(P + 4, 5, P, 2, 5, P, None) == -2 and call(P, 5, P + 2, 2, 5, P, None) == -2


# ---------------------------------------------------------------------------------------------------- CPU routes
GUARD = 0x5A5A5A5A


def test_state_copy_cpu_route():
    from spike2former_amd import ops
    g = torch.Generator().manual_seed(3)
    store = torch.randn(64, generator=g)
    tensors = [torch.randn(5, generator=g), torch.arange(3, dtype=torch.int64) * (1 << 40) + 7, store[1:4], store[6:8], store[11:12],
               torch.randn(2, 3, generator=g), torch.zeros(0)]
    tensors[0][1], tensors[0][2] = float("nan"), 1e-42          # a NaN and a denormal travel as bits
    slots, chunks, words = ops.state_table(tensors)
    assert words % 4 == 0 and all(off % 4 == 0 for _, off, _ in slots.tolist())
    assert [n for _, _, n in slots.tolist()] == [5, 6, 3, 2, 1, 6, 0]
    flat = torch.full((words + 8,), GUARD, dtype=torch.int32)
    ops.state_copy(tensors, slots, chunks, flat)
    covered = torch.zeros(words + 8, dtype=torch.bool)
    for t, (_, off, n) in zip(tensors, slots.tolist()):
        assert torch.equal(flat[off:off + n], t.reshape(-1).view(torch.int32))
        covered[off:off + n] = True
    assert bool((flat[~covered] == GUARD).all()) and int((~covered).sum()) > 8
    want = [t.clone() for t in tensors]
    before = store.clone()
    for t in tensors:
        t.view(-1).view(torch.int32).fill_(GUARD)
    untouched = torch.ones(64, dtype=torch.bool)
    untouched[1:4] = untouched[6:8] = untouched[11:12] = False
    ops.state_copy(tensors, slots, chunks, flat, to_params=True)
    for t, w in zip(tensors, want):
        assert torch.equal(t.reshape(-1).view(torch.int32), w.reshape(-1).view(torch.int32))
    assert torch.equal(store[untouched], before[untouched])
    with pytest.raises(TypeError):
        ops.state_table([torch.zeros(3, dtype=torch.uint8)])
    with pytest.raises(ValueError):
        ops.state_copy(tensors, slots, chunks, flat.to(torch.float32))


def test_train_log_append_cpu_route():
    from spike2former_amd import ops
    n, window, stride = 5, 3, 7
    srcs = [torch.zeros(()) for _ in range(n)]
    ring = torch.full((window, stride), -7.0)
    head = torch.tensor([0, -1], dtype=torch.int64)
    rows = []
    for it in range(window + 3):
        for j, s in enumerate(srcs):
            s.fill_(10.0 * it + j)
        if it == 2:
            srcs[4].fill_(float("inf"))
        if it == 4:
            srcs[0].fill_(float("nan"))
        rows.append([float(s) for s in srcs])
        ops.train_log_append(srcs, ring, head)
        assert head.tolist() == [it + 1, -1 if it < 2 else 2]
        assert ring[it % window, :n].tolist() == pytest.approx(rows[-1], nan_ok=True)
    assert bool((ring[:, n:] == -7.0).all())
    for it in range(window + 3 - window, window + 3):
        assert ring[it % window, :n].tolist() == pytest.approx(rows[it], nan_ok=True)
    with pytest.raises(ValueError):
        ops.train_log_append(srcs, ring[:, :4].contiguous(), head)


# ---------------------------------------------------------------------------------------------------- the loop on a fake step
class FakeAugment:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.calls = 0

    def __call__(self, images, segs, out=None):
        self.rng.random(3)
        self.calls += 1


class FakeStep:
    """what the loop sees of a captured step: static inputs, the model, a log it appends one scripted row to per call"""

    def __init__(self, model, script, log):
        self.model, self.script, self.log, self.calls = model, script, log, 0
        self.static_in, self.static_seg = torch.zeros(1), torch.zeros(1, dtype=torch.uint8)
        self.vals = {k: torch.zeros(()) for k in ("loss_cls", "loss_mask", "loss", "grad_norm", "clip_coef")}
        log.bind(self.vals)

    def __call__(self):
        a, b = self.script[self.calls]
        for k, v in (("loss_cls", a), ("loss_mask", b), ("loss", np.float32(a) + np.float32(b)), ("grad_norm", 2.0 * a), ("clip_coef", 1.0)):
            self.vals[k].fill_(float(v))
        with torch.no_grad():
            for p in self.model.parameters():
                p.add_(1.0)
            self.model[1].num_batches_tracked.add_(1)
        self.log.append()
        self.calls += 1

    def check(self):
        pass


def make_run(tmp_path, script, hooks, seed=0, max_iters=None, **kw):
    import spike2former_amd as s2f
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.train import FlatAdamW, LinearThenPoly
    torch.manual_seed(seed)
    model = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.BatchNorm1d(5))
    red = FlatGradAllReduce(model.parameters(), 1)
    opt = FlatAdamW(model, red, lr=0.01)
    sched = LinearThenPoly(opt, warmup=2, total=50, start_factor=0.1)
    log = s2f.TrainLog(window=16, device="cpu", capacity=8)
    step = FakeStep(model, script, log)
    aug = FakeAugment(seed)
    loop = s2f.TrainLoop(step, opt, sched, aug, [(None, None)] * 3, max_iters=max_iters or len(script), hooks=hooks,
                         work_dir=str(tmp_path), **kw)
    return loop


def scalars(tmp_path):
    with open(os.path.join(tmp_path, "vis_data", "scalars.json")) as f:
        return [json.loads(line) for line in f]


def test_hooks_are_registered_under_the_reference_names():
    import spike2former_amd as s2f
    assert s2f.HOOKS.get("LoggerHook") is s2f.LoggerHook and s2f.HOOKS.get("CheckpointHook") is s2f.CheckpointHook
    assert s2f.HOOKS.get("ParamSchedulerHook") is s2f.ParamSchedulerHook
    with pytest.raises(NotImplementedError):
        s2f.CheckpointHook(interval=1, by_epoch=True)
    assert s2f.CheckpointHook(interval=1, save_best="mIoU").rule == "greater"
    assert s2f.CheckpointHook(interval=1, save_best="val_loss").rule == "less"
    with pytest.raises(ValueError):
        s2f.CheckpointHook(interval=1, save_best="speed")


def test_logger_lines_and_window_means(tmp_path, caplog):
    rng = np.random.default_rng(1)
    script = [tuple(np.float32(v) for v in rng.random(2)) for _ in range(11)]
    loop = make_run(tmp_path, script, [dict(type="LoggerHook", interval=4, window_size=3), dict(type="ParamSchedulerHook")])
    lrs = []
    with caplog.at_level(logging.INFO, logger="spike2former_amd"):
        loop.run()
    lines = scalars(tmp_path)
    assert [r["iter"] for r in lines] == [4, 8, 11]          # every 4th and the last
    assert sum("Iter(train)" in r.message for r in caplog.records) == 3
    for r in lines:
        rows = script[max(r["iter"] - 3, 0):r["iter"]]
        a, b = (np.array([row[j] for row in rows], np.float32) for j in (0, 1))
        assert r["loss_cls"] == float(np.mean(a)) and r["loss_mask"] == float(np.mean(b))
        assert r["loss"] == float(np.mean(a + b)) and r["grad_norm"] == float(np.mean(np.float32(2.0) * a))
        assert "clip_coef" not in r and r["time"] >= 0 and r["eta"] >= 0 and "memory" in r
    # the learning rate of the iteration that was logged, not of the next one
    from spike2former_amd.train import LinearThenPoly

    class G:
        param_groups = [dict(lr=0.01)]
    ref = LinearThenPoly(G(), warmup=2, total=50, start_factor=0.1)
    for n in range(1, 12):
        lrs.append(G.param_groups[0]["lr"])
        ref.step()
    assert [r["lr"] for r in lines] == pytest.approx([lrs[3], lrs[7], lrs[10]], rel=1e-6)
    assert loop.augment.calls == 11 and loop.step.calls == 11 and loop.scheduler.t == 11


def test_checkpoint_iterations_last_checkpoint_and_max_keep(tmp_path):
    script = [(0.5, 0.25)] * 7
    for async_write in (True, False):
        work = tmp_path / str(async_write)
        loop = make_run(work, script, [dict(type="CheckpointHook", interval=2, max_keep_ckpts=2), dict(type="LoggerHook", interval=50)],
                        async_write=async_write)
        loop.run()
        files = sorted(f for f in os.listdir(work) if f.endswith(".pth"))
        assert files == ["iter_6.pth", "iter_7.pth"]          # 2, 4 were pruned; 7 is the last iteration (save_last)
        assert open(work / "last_checkpoint").read() == str(work / "iter_7.pth")
        assert not [f for f in os.listdir(work) if f.endswith(".tmp")]
        ck = torch.load(work / "iter_6.pth", weights_only=True)
        assert ck["meta"]["iter"] == 6 and ck["param_schedulers"] == [dict(t=6)]
        assert list(ck["state_dict"]) == list(loop.step.model.state_dict())
        # the file of iteration 6 holds iteration 6's weights although iteration 7 ran before the run ended
        live = loop.step.model.state_dict()
        assert torch.equal(ck["state_dict"]["0.weight"] + 1.0, live["0.weight"])
        assert int(ck["state_dict"]["1.num_batches_tracked"]) == 6 and ck["state_dict"]["1.num_batches_tracked"].dtype == torch.int64
        assert set(ck["optimizer"]["state"]) == {"0.weight", "0.bias", "1.weight", "1.bias"}
        assert ck["optimizer"]["state"]["0.weight"]["exp_avg"].shape == (5, 3)


def test_save_best_keeps_the_right_file(tmp_path):
    script = [(0.5, 0.25)] * 8
    scores = iter([0.2, 0.5, 0.4, 0.5])          # validations after iterations 2, 4, 6, 8: the best is 4 (a tie does not replace)
    seen = []

    def validate():
        seen.append(next(scores))
        return {"mIoU": np.float64(seen[-1]), "aAcc": 0.1}
    loop = make_run(tmp_path, script, [dict(type="CheckpointHook", interval=100, save_last=False, save_best="mIoU"),
                                       dict(type="LoggerHook", interval=50)], val_interval=2, validate=validate)
    assert loop.run() == {"mIoU": 0.5, "aAcc": 0.1}
    assert len(seen) == 4
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".pth")) == ["best_mIoU_iter_4.pth"]
    ck = torch.load(tmp_path / "best_mIoU_iter_4.pth", weights_only=True)
    assert ck["meta"]["iter"] == 4 and ck["best"]["score"] == 0.5 and ck["best"]["key"] == "mIoU"
    assert [r["mIoU"] for r in scalars(tmp_path) if "mIoU" in r] == [0.2, 0.5, 0.4, 0.5]
    # the `less` rule
    scores = iter([0.3, 0.1, 0.2])
    loop = make_run(tmp_path / "less", script[:6], [dict(type="CheckpointHook", save_last=False, save_best="val_loss"),
                                                    dict(type="LoggerHook", interval=50)],
                    val_interval=2, validate=lambda: {"val_loss": next(scores)})
    loop.run()
    assert sorted(f for f in os.listdir(tmp_path / "less") if f.endswith(".pth")) == ["best_val_loss_iter_4.pth"]


def test_non_finite_loss_names_its_iteration_and_writes_no_file(tmp_path):
    script = [(0.5, 0.25)] * 4 + [(float("inf"), 0.25)] + [(0.5, float("nan"))] + [(0.5, 0.25)] * 4
    # the checkpoint of iteration 6 comes up before the next log line (8): the checkpoint hook looks first
    loop = make_run(tmp_path, script, [dict(type="CheckpointHook", interval=3), dict(type="LoggerHook", interval=4, window_size=2)])
    with pytest.raises(FloatingPointError, match=r"iteration 5\b.*loss_cls = inf"):
        loop.run()
    assert loop.step.calls == 6
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".pth")) == ["iter_3.pth"]
    assert open(tmp_path / "last_checkpoint").read().endswith("iter_3.pth")
    assert [r["iter"] for r in scalars(tmp_path)] == [4]
    # ... and the log line alone finds it too, although the ring (two rows) has wrapped past the row
    import spike2former_amd as s2f
    loop = make_run(tmp_path / "b", [(float("nan"), 0.25)] + [(0.5, 0.25)] * 7, [dict(type="LoggerHook", interval=4, window_size=2)])
    loop.step.log = loop.log = s2f.TrainLog(loop.step.vals, window=2, device="cpu")
    with pytest.raises(FloatingPointError, match=r"iteration 1\b"):
        loop.run()
    assert loop.step.calls == 4


def test_strict_load_lists_names_and_resume_restores_everything(tmp_path):
    script = [(0.5, 0.25)] * 5
    loop = make_run(tmp_path, script, [dict(type="CheckpointHook", interval=3, save_last=False), dict(type="LoggerHook", interval=50)],
                    seed=1)
    with torch.no_grad():
        loop.optimizer.exp_avg.copy_(torch.arange(loop.optimizer.exp_avg.numel()))
        loop.optimizer.exp_avg_sq.fill_(0.5)
        loop.optimizer.state[4] = 3.0
    loop.run()
    path = str(tmp_path / "iter_3.pth")
    ck = torch.load(path, weights_only=True)
    # a resumed run, everything rebuilt from another seed
    again = make_run(tmp_path, script, [dict(type="LoggerHook", interval=2, window_size=2)], seed=2, resume=True)
    assert not torch.equal(again.step.model[0].weight, ck["state_dict"]["0.weight"])
    again.step.script = script[3:]
    again.run()
    assert again.step.calls == 2 and again.scheduler.t == 5          # iterations 4 and 5
    assert [r["iter"] for r in scalars(tmp_path)][-2:] == [4, 5]
    for (k, a), b in zip(loop.step.model.state_dict().items(), again.step.model.state_dict().values()):
        assert torch.equal(a, b), k
    for p, off in zip(loop.optimizer.params, loop.optimizer.red.offsets):          # (pads between the slots are not state)
        for name in ("exp_avg", "exp_avg_sq"):
            a, b = (getattr(o.optimizer, name)[off:off + p.numel()] for o in (again, loop))
            assert torch.equal(a, b) and float(b.abs().sum()) > 0
    assert float(again.optimizer.state[4]) == 3.0
    assert [g["lr"] for g in again.optimizer.param_groups] == [g["lr"] for g in loop.optimizer.param_groups]
    assert again.augment.rng.random() == loop.augment.rng.random()
    # strict names and shapes
    sd = dict(ck["state_dict"])
    sd["extra.weight"] = sd.pop("0.bias")
    sd["1.weight"] = torch.zeros(4)
    bad = str(tmp_path / "bad.pth")
    torch.save(dict(state_dict=sd), bad)
    with pytest.raises(RuntimeError) as e:
        again.state.load(bad)
    msg = str(e.value)
    assert "missing: ['0.bias']" in msg and "unexpected: ['extra.weight']" in msg and "1.weight: (4,) in the file, (5,) in the model" in msg
    with pytest.raises(RuntimeError, match="no optimizer state"):
        again.state.load(bad, resume=True)
    # weights only: load_from without resume starts at iteration 0 with the file's weights
    fresh = make_run(tmp_path / "w", script[:1], [], seed=3, load_from=path)
    fresh.run()
    assert fresh.step.calls == 1 and torch.equal(fresh.step.model[0].weight, ck["state_dict"]["0.weight"] + 1.0)
