"""GPU: TrainLoop, TrainLog and TrainState (runner.py) around GraphedHungarianStep(assign="device", optimizer=FlatAdamW) on the tiny
configuration C1_64, fed with seeded synthetic uint8 pictures through TrainAugment.  Three rigs (model, gradient buffer, optimizer,
scheduler, augmentation, captured step) are built once for the module:
    plain  -- log=None: the step as it was before the loop existed; the yardstick of the continuation test
    first  -- with a TrainLog
    second -- with a TrainLog, from other seeds: what a run is resumed INTO
The rig itself is tests/step_rig.py's; a rig is put back to its start between tests by code that predates the loop
(load_state_dict, zeroed moments, a fresh generator)."""
import copy
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from step_rig import NORM, SHAPES, iterate, new_loop, reset, rigs_fixture, scramble, state_of          # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

recipes = dict(plain=dict(log=False), first=dict(), second=dict(seed=3))
rigs = rigs_fixture(recipes)


def test_the_loop_logs_what_the_step_computed(rigs, tmp_path):
    r = rigs("first")
    reset(r)
    assert r.step.two_graphs is False and list(r.log.names)[-3:] == ["loss", "grad_norm", "clip_coef"]
    assert list(r.log.names)[:-3] == list(r.step.losses)
    seen = []

    class Spy:          # the instrumented twin: reads the step's static tensors back after EVERY iteration
        priority = 0

        def after_train_iter(self, loop):
            torch.cuda.synchronize()
            row = {k: v.item() for k, v in loop.step.losses.items()}
            row.update(loss=loop.step.log_terms["loss"].item(), grad_norm=loop.optimizer.grad_norm.item())
            seen.append(row)
    loop = new_loop(r, rigs.batches, 12, [Spy(), dict(type="LoggerHook", interval=4, window_size=3)], work_dir=str(tmp_path))
    loop.run()
    with open(tmp_path / "vis_data" / "scalars.json") as f:
        lines = [json.loads(line) for line in f]
    assert [rec["iter"] for rec in lines] == [4, 8, 12] and len(seen) == 12
    for rec in lines:
        rows = seen[rec["iter"] - 3:rec["iter"]]
        for k in seen[0]:
            want = float(np.mean(np.array([row[k] for row in rows], np.float32)))
            assert rec[k] == want and np.isfinite(want), (rec["iter"], k, rec[k], want)
        assert rec["memory"] > 0 and rec["time"] > 0
    assert len({rec["loss"] for rec in lines}) == 3          # the weights move: three different windows
    assert float(r.opt.state[4]) == 12.0 and r.sched.t == 12


def test_state_round_trip_is_exact(rigs, tmp_path):
    import spike2former_amd as s2f
    r, r2 = rigs("first"), rigs("second")
    reset(r)
    scramble(r2)
    iterate(r, rigs.batches, 0, 3)
    want = state_of(r)          # (waits for the device)
    r.opt.sync_hyper()
    hyper, t, rng = r.opt.hyper.clone(), r.sched.t, copy.deepcopy(r.aug.rng.bit_generator.state)
    state = s2f.TrainState(r.model, r.opt, r.sched, r.aug)
    path = str(tmp_path / "three.pth")
    state.snapshot()
    state.write(path, meta=dict(iter=3))
    iterate(r, rigs.batches, 3, 2)          # queued behind the snapshot, BEFORE the write is joined
    state.close()
    moved = state_of(r)
    assert any(not torch.equal(moved[k], want[k]) for k in want if k.startswith("model:"))
    ck = torch.load(path, weights_only=True)
    assert ck["meta"] == dict(iter=3) and ck["optimizer"]["step"] == 3 and ck["param_schedulers"] == [dict(t=3)]
    assert list(ck["state_dict"]) == list(r.model.state_dict())
    for k, v in ck["state_dict"].items():          # the staging, not the live buffers, was copied
        assert v.dtype == want[f"model:{k}"].dtype and torch.equal(v, want[f"model:{k}"].cpu()), k
    # into a rig built from other seeds
    s2f.TrainState(r2.model, r2.opt, r2.sched, r2.aug).load(path, resume=True)
    got = state_of(r2)
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    r2.opt.sync_hyper()
    torch.cuda.synchronize()
    assert torch.equal(r2.opt.hyper, hyper) and r2.sched.t == t
    r.aug.rng.bit_generator.state = rng
    a, b = r.aug.draw(SHAPES), r2.aug.draw(SHAPES)
    assert a.tobytes() == b.tobytes()


def test_a_resumed_run_continues_the_uninterrupted_one(rigs, tmp_path):
    """A, A': six iterations twice from the same seeds on the step WITHOUT a log, by code that predates the loop -- d0, their
    largest per-tensor absolute difference, is the run-to-run spread of the existing step.  B: three iterations in the loop, a
    checkpoint, everything else rebuilt from other seeds and captured separately, resume, three iterations.  |B - A| <= 4 d0 for
    every tensor (bit equality when d0 = 0); d0 is taken per kind of tensor (weights and buffers, first moments, second moments),
    which is no weaker than one d0 over all of them.  Observed d0: see DESIGN.md section 9."""
    plain, r, r2 = rigs("plain"), rigs("first"), rigs("second")
    runs = []
    for _ in range(2):
        reset(plain)
        iterate(plain, rigs.batches, 0, 6)
        runs.append(state_of(plain))
    a, a2 = runs
    kinds = ("model:", "exp_avg:", "exp_avg_sq:", "step:")
    d0 = {kind: max(float((a[k].double() - a2[k].double()).abs().max()) for k in a if k.startswith(kind) and a[k].numel())
          for kind in kinds}
    print("d0 (A against A'):", d0)
    reset(r)
    hooks = [dict(type="LoggerHook", interval=3, window_size=3), dict(type="CheckpointHook", interval=3)]
    new_loop(r, rigs.batches, 3, hooks, work_dir=str(tmp_path)).run()
    assert open(tmp_path / "last_checkpoint").read() == str(tmp_path / "iter_3.pth")
    scramble(r2)
    loop = new_loop(r2, rigs.batches, 6, hooks, work_dir=str(tmp_path), resume=True)
    loop.run()
    assert loop.resumed["meta"]["iter"] == 3 and sorted(f for f in os.listdir(tmp_path) if f.endswith(".pth")) == ["iter_3.pth", "iter_6.pth"]
    with open(tmp_path / "vis_data" / "scalars.json") as f:
        assert [json.loads(line)["iter"] for line in f] == [3, 6]
    b = state_of(r2)
    assert list(b) == list(a)
    worst = {kind: 0.0 for kind in kinds}
    for k in a:
        if a[k].numel():
            kind = next(x for x in kinds if k.startswith(x))
            d = float((b[k].double() - a[k].double()).abs().max())
            worst[kind] = max(worst[kind], d)
            assert d <= 4.0 * d0[kind], (k, d, d0[kind])
    print("largest |B - A|:", worst)
    assert float(b["step:"]) == 6.0 and r2.sched.t == 6


def test_save_best_and_load_from(rigs, tmp_path):
    import spike2former_amd as s2f
    from spike2former_amd.augment import TestAugment
    r, r2 = rigs("first"), rigs("second")
    reset(r)
    scramble(r2)
    rng = np.random.default_rng(11)
    pictures = [(rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), rng.integers(0, r.K + 1, (37, 53)).astype(np.uint8), f"img{i}.png")
                for i in range(2)]
    pipeline = [dict(type="LoadImageFromFile"), dict(type="Resize", scale=(96, 40), keep_ratio=True),
                dict(type="LoadAnnotations", reduce_zero_label=True), dict(type="PackSegInputs")]
    test_aug = TestAugment.from_cfg(pipeline, dict(type="SegDataPreProcessor", pad_val=0, seg_pad_val=255, **NORM), reduce_zero_label=True,
                                    max_source_pixels=64 * 64)

    def validate(model):
        m = s2f.IoUMetric(label_reduce_zero=True)
        m.dataset_meta = dict(classes=[str(i) for i in range(r.K)])
        return s2f.evaluate(model, (test_aug([img], [seg], [p]) for img, seg, p in pictures), m)
    reported = []

    def validate_first():
        reported.append(validate(r.model))
        return reported[-1]
    hooks = [dict(type="LoggerHook", interval=2, window_size=2), dict(type="CheckpointHook", interval=100, save_last=False, save_best="mIoU")]
    new_loop(r, rigs.batches, 6, hooks, work_dir=str(tmp_path), val_interval=2, validate=validate_first).run()
    assert r.model.training and len(reported) == 3
    best, score = None, None
    for i, rep in enumerate(reported):          # the `greater` rule: the first of the largest
        if score is None or rep["mIoU"] > score:
            best, score = 2 * (i + 1), rep["mIoU"]
    print("mIoU after 2, 4, 6 iterations:", [rep["mIoU"] for rep in reported])
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".pth")) == [f"best_mIoU_iter_{best}.pth"]
    # the weights of that file in another model evaluate to the dictionary that was reported for them
    path = str(tmp_path / f"best_mIoU_iter_{best}.pth")
    loop = new_loop(r2, rigs.batches, 0, work_dir=str(tmp_path / "other"), load_from=path)
    loop.run()
    assert loop.resumed["best"]["score"] == score and r2.sched.t == 9          # weights only: the schedule stays where it was
    again = validate(r2.model)
    want = reported[best // 2 - 1]
    assert list(again) == list(want)
    assert np.array_equal(np.array(list(again.values()), float), np.array(list(want.values()), float), equal_nan=True), (again, want)


def test_two_ranks_train_checkpoint_and_resume(tmp_path):
    """two fresh child processes (torch.distributed.run, gloo, both on GPU 0) run tests/_train_loop_worker.py: after four
    iterations only rank 0 has written files and both ranks hold bit-equal parameters; both resume from rank 0's file, each with
    its own augment generator, and continue"""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, S2F_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "_train_loop_worker.py"), str(tmp_path)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=400)      # children only: nothing is re-exec'ed
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "RANK 0 OK" in r.stdout and "RANK 1 OK" in r.stdout, r.stdout[-2000:]
    assert sorted(os.listdir(tmp_path)) == ["rank0", "rank0_resumed"]          # rank 1 wrote nothing, before or after the resume
