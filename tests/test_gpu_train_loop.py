"""GPU: TrainLoop, TrainLog and TrainState (runner.py) around GraphedHungarianStep(assign="device", optimizer=FlatAdamW) on the tiny
configuration C1_64, fed with seeded synthetic uint8 pictures through TrainAugment.  Three rigs (model, gradient buffer, optimizer,
scheduler, augmentation, captured step) are built once for the module:
    plain  -- log=None: the step as it was before the loop existed; the yardstick of the continuation test
    first  -- with a TrainLog
    second -- with a TrainLog, from other seeds: what a run is resumed INTO
A rig is put back to its start between tests by code that predates the loop (load_state_dict, zeroed moments, a fresh generator)."""
import copy
import gc
import json
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], bgr_to_rgb=True)
SHAPES = ((70, 90), (64, 48))
CLIP = dict(max_norm=0.01, norm_type=2)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def region_map(h, w, classes):
    seg = np.empty((h, w), np.uint8)
    for i, (y, x) in enumerate((y, x) for y in range(0, h, 16) for x in range(0, w, 16)):
        seg[y:y + 16, x:x + 16] = classes[i % len(classes)]
    seg[:2, 3:17] = 255
    return seg


def make_batches(K):
    rng = np.random.default_rng(50)
    out = []
    for b in range(3):
        images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]
        segs = [region_map(h, w, rng.permutation(K)[:4 + i + b]) for i, (h, w) in enumerate(SHAPES)]
        out.append((images, segs))
    return out


def build(seed, log):
    import spike2former_amd as s2f
    from spike2former_amd.augment import TrainAugment
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.graph import GraphedHungarianStep
    from spike2former_amd.init_utils import seeded_init
    from spike2former_amd.train import FlatAdamW, LinearThenPoly
    w = s2f.WORKLOADS["C1_64"]
    crop = (w["H"], w["W"])
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C1_64")))
    if seed:          # other weights than the other rigs'
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in model.parameters():
                p.mul_(1.0 + 0.05 * torch.randn(p.shape, generator=g))
    model = model.cuda().train()
    s2f.set_keep_membrane(model, False)
    r = types.SimpleNamespace(model=model, K=w["K"], crop=crop, seed=seed)
    r.sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    r.red = FlatGradAllReduce(model.parameters(), 1)
    r.opt = FlatAdamW(model, r.red, lr=0.001, weight_decay=0.005, clip_grad=CLIP,
                      paramwise_cfg=dict(custom_keys={"backbone": dict(lr_mult=0.1, decay_mult=1.0)}))
    r.sched = LinearThenPoly(r.opt, warmup=4, total=20, start_factor=0.1)
    r.aug = TrainAugment(crop_size=crop, scale=(2 * crop[1], crop[0]), ratio_range=(0.5, 2.0), cat_max_ratio=0.75, photometric=True,
                         batch_size=2, max_source_pixels=70 * 90, seed=11 + seed, rank=0, **NORM)
    r.log = s2f.TrainLog(window=8) if log else None
    example_in = torch.randn(2, 3, *crop, generator=torch.Generator().manual_seed(5)).cuda()
    example_seg = torch.from_numpy(np.stack([region_map(*crop, [1, 2, 3]), region_map(*crop, [4, 5])])).cuda()
    r.step = GraphedHungarianStep(model, example_in, example_seg, r.red, warmup=1, optimizer=r.opt, assign="device", log=r.log)
    reset(r)
    return r


def reset(r):
    """the rig at its start, by code that predates the loop"""
    r.model.load_state_dict(r.sd0)
    r.opt.exp_avg.zero_(), r.opt.exp_avg_sq.zero_(), r.opt.state.zero_()
    r.sched.t = 0
    r.sched._apply()
    r.aug.rng = np.random.default_rng(np.random.SeedSequence([r.aug.seed, r.aug.rank]))
    r.opt.mark_updated()
    torch.cuda.synchronize()


def scramble(r):
    """a rig that has been somewhere else: nothing of what a resume restores is at its start"""
    reset(r)
    with torch.no_grad():
        for t in r.model.state_dict().values():
            t.add_(3) if t.dtype == torch.int64 else t.mul_(1.25)
    r.opt.exp_avg.fill_(0.5), r.opt.exp_avg_sq.fill_(0.25), r.opt.state.fill_(7.0)
    r.sched.t = 9
    r.sched._apply()
    r.aug.rng.random(5)


def iterate(r, batches, first, count):
    """`count` iterations from the `first`-th, as a caller wrote them before the loop existed"""
    for it in range(first, first + count):
        images, segs = batches[it % len(batches)]
        r.aug(images, segs, out=(r.step.static_in, r.step.static_seg))
        r.step()
        r.sched.step()


def state_of(r):
    torch.cuda.synchronize()
    out = {f"model:{k}": v.clone() for k, v in r.model.state_dict().items()}
    for p, off, g in zip(r.opt.params, r.red.offsets, r.opt.param_groups):
        out[f"exp_avg:{g['name']}"] = r.opt.exp_avg[off:off + p.numel()].clone()
        out[f"exp_avg_sq:{g['name']}"] = r.opt.exp_avg_sq[off:off + p.numel()].clone()
    out["step:"] = r.opt.state[4:5].clone()
    return out


@pytest.fixture(scope="module")
def rigs():
    import spike2former_amd as s2f
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = build(dict(plain=0, first=0, second=3)[name], log=name != "plain")
        return cache[name]
    get.batches = make_batches(s2f.WORKLOADS["C1_64"]["K"])
    yield get
    for r in cache.values():
        for p in r.model.parameters():
            p.grad = None
    cache.clear()
    gc.collect()


def new_loop(r, batches, max_iters, hooks=(), **kw):
    import spike2former_amd as s2f
    return s2f.TrainLoop(r.step, r.opt, r.sched, r.aug, batches, max_iters=max_iters, hooks=list(hooks), **kw)


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
