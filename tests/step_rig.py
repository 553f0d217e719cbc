"""The rig of the captured-step tests, written once: the tiny configuration C1_64 behind GraphedHungarianStep(assign="device",
optimizer=FlatAdamW), fed with seeded synthetic uint8 pictures through TrainAugment.  tests/test_gpu_train_loop.py,
test_gpu_grad_accum.py, test_gpu_weight_ema.py, test_gpu_firing_log.py, test_gpu_seg_log.py and test_gpu_grad_log.py build their rigs
here, each from its own `recipes`; their two-rank workers take the ingredients.  The figures those files quote from the MI355X hold
for exactly these seeds, pictures and constructor arguments (tests/test_step_rig_host.py pins the inputs).

Nothing of the package is imported at module level: the files that use this collect where libs2f_hip.so is not built."""
import gc
import types

import numpy as np
import pytest
import torch

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], bgr_to_rgb=True)
SHAPES = ((70, 90), (64, 48))
CLIP = dict(max_norm=0.01, norm_type=2)
PARAMWISE = dict(custom_keys={"backbone": dict(lr_mult=0.1, decay_mult=1.0)})
KINDS = ("model:", "exp_avg:", "exp_avg_sq:", "step:", "loss:")          # of the keys of state_of(); "loss:": what a caller adds


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


def examples(crop):
    """-> (example_in fp32 [2, 3, *crop], example_seg uint8 [2, *crop]) on the host: what every rig is captured on"""
    example_in = torch.randn(2, 3, *crop, generator=torch.Generator().manual_seed(5))
    return example_in, torch.from_numpy(np.stack([region_map(*crop, [1, 2, 3]), region_map(*crop, [4, 5])]))


def build(seed=0, log=True, optimizer=True, step_optimizer=True, counts=None, ema=None, grad_log=None, firing=None, seg_log=None,
          keep_graph=False):
    """One rig.  An argument left at None is NOT passed on: the rig is built without it, which is what several tests are about.
    seed           -- not 0: other weights (a seeded perturbation) and another augment seed
    log            -- a TrainLog(window=8) in the step
    optimizer      -- False: no FlatAdamW, scheduler or TrainLog at all, the weights stand still
    step_optimizer -- False: the plain step; the rig's FlatAdamW is stepped by the caller (`eager`)
    counts, ema, grad_log -- FlatAdamW(accumulative_counts=, ema=, grad_log=)
    firing, seg_log       -- the arguments of a FiringLog over the model / a SegLog over its classes, handed to the step
    keep_graph     -- the step's graphs are captured with CUDAGraph(keep_graph=True), so that their nodes can be counted"""
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
    r = types.SimpleNamespace(model=model, K=w["K"], crop=crop, seed=seed, eager=not step_optimizer)
    r.sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    r.red = FlatGradAllReduce(model.parameters(), 1)
    r.opt = r.sched = r.log = None
    if optimizer:
        extra = {k: v for k, v in dict(accumulative_counts=counts, ema=ema, grad_log=grad_log).items() if v is not None}
        r.opt = FlatAdamW(model, r.red, lr=0.001, weight_decay=0.005, clip_grad=CLIP, paramwise_cfg=PARAMWISE, **extra)
        r.sched = LinearThenPoly(r.opt, warmup=4, total=20, start_factor=0.1)
        r.log = s2f.TrainLog(window=8) if log else None
    r.aug = TrainAugment(crop_size=crop, scale=(2 * crop[1], crop[0]), ratio_range=(0.5, 2.0), cat_max_ratio=0.75, photometric=True,
                         batch_size=2, max_source_pixels=70 * 90, seed=11 + seed, rank=0, **NORM)
    r.firing = None if firing is None else s2f.FiringLog(model, **firing)
    r.seg_log = None if seg_log is None else s2f.SegLog(r.K, **seg_log)
    step_extra = {k: v for k, v in dict(firing=r.firing, seg_log=r.seg_log).items() if v is not None}
    example_in, example_seg = (t.cuda() for t in examples(crop))
    plain_graph = torch.cuda.CUDAGraph
    if keep_graph:
        torch.cuda.CUDAGraph = lambda: plain_graph(keep_graph=True)
    try:
        r.step = GraphedHungarianStep(model, example_in, example_seg, r.red, warmup=1, optimizer=r.opt if step_optimizer else None,
                                      assign="device", log=r.log, **step_extra)
    finally:
        torch.cuda.CUDAGraph = plain_graph
    reset(r)
    return r


def reset(r):
    """the rig at its start, by code that predates the loop; each part where the rig has it"""
    r.model.load_state_dict(r.sd0)
    opt = r.opt
    if opt is not None:
        opt.exp_avg.zero_(), opt.exp_avg_sq.zero_(), opt.state.zero_()
        r.sched.t = 0
        r.sched._apply()
    r.aug.rng = np.random.default_rng(np.random.SeedSequence([r.aug.seed, r.aug.rank]))
    if opt is not None and opt.accum is not None:
        opt.accum.count, opt.accum.total = 0, None
        opt.accum.stats.zero_()
    if opt is not None and opt.ema is not None:
        opt.ema.reset()
        opt.ema.partials.zero_()
    if r.firing is not None:
        r.firing.clear()
    if r.seg_log is not None:
        r.seg_log.clear()
    if opt is not None:
        opt.mark_updated()
    torch.cuda.synchronize()


def scramble(r):
    """a rig that has been somewhere else: nothing of what a resume restores is at its start"""
    reset(r)
    with torch.no_grad():
        for t in r.model.state_dict().values():
            t.add_(3) if t.dtype == torch.int64 else t.mul_(1.25)
    r.opt.exp_avg.fill_(0.5), r.opt.exp_avg_sq.fill_(0.25), r.opt.state.fill_(7.0)
    if r.opt.ema is not None:
        r.opt.ema.ema.fill_(0.125)
    r.sched.t = 9
    r.sched._apply()
    r.aug.rng.random(5)


def feed(r, batch):
    images, segs = batch
    r.aug(images, segs, out=(r.step.static_in, r.step.static_seg))


def iterate(r, batches, first, count, watch=None):
    """`count` iterations from the `first`-th, as a caller wrote them before the loop existed; an eager rig's update is launched
    here; `watch(iteration)` runs behind each"""
    for it in range(first, first + count):
        feed(r, batches[it % len(batches)])
        r.step()
        if r.eager:
            r.opt.step()
        r.sched.step()
        if watch is not None:
            watch(it)


def state_of(r):
    torch.cuda.synchronize()
    out = {f"model:{k}": v.clone() for k, v in r.model.state_dict().items()}
    for p, off, g in zip(r.opt.params, r.red.offsets, r.opt.param_groups):
        out[f"exp_avg:{g['name']}"] = r.opt.exp_avg[off:off + p.numel()].clone()
        out[f"exp_avg_sq:{g['name']}"] = r.opt.exp_avg_sq[off:off + p.numel()].clone()
    out["step:"] = r.opt.state[4:5].clone()
    return out


def gaps(a, b, kinds=KINDS):
    """largest absolute difference per kind of tensor (0 for a kind without one)"""
    assert list(a) == list(b)
    return {kind: max([float((a[k].double() - b[k].double()).abs().max()) for k in a if k.startswith(kind) and a[k].numel()] or [0.0])
            for kind in kinds}


def new_loop(r, batches, max_iters, hooks=(), **kw):
    import spike2former_amd as s2f
    return s2f.TrainLoop(r.step, r.opt, r.sched, r.aug, batches, max_iters=max_iters, hooks=list(hooks), **kw)


class Elementwise(torch.nn.Module):
    """a model whose step IS bit-repeatable: element-wise products and torch's fixed-order sums, no atomics anywhere"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(4)
        self.backbone_w = torch.nn.Parameter(torch.randn(3, 33, 35, generator=g))
        self.b = torch.nn.Parameter(torch.randn(35, generator=g))
        self.gain = torch.nn.Parameter(torch.randn(1, generator=g))

    def forward(self, x):
        return (torch.tanh(x * self.backbone_w + self.b) * self.gain,)


def rigs_fixture(recipes):
    """-> the module-scoped fixture `rigs`: rigs(name) builds recipes[name] at its first use and keeps it for the module;
    rigs.batches: the pictures; rigs.runs: results one test leaves for another"""
    @pytest.fixture(scope="module")
    def rigs():
        import spike2former_amd as s2f
        cache = {}

        def get(name):
            if name not in cache:
                cache[name] = build(**recipes[name])
            return cache[name]
        get.batches = make_batches(s2f.WORKLOADS["C1_64"]["K"])
        get.runs = {}
        yield get
        for r in cache.values():
            if r.firing is not None:
                r.firing.detach()
            for p in r.model.parameters():
                p.grad = None
        cache.clear()
        gc.collect()
    return rigs
