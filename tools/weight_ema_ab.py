"""What the weight average (FlatAdamW(ema=...), ema.WeightEMA) costs per iteration (profiles/weight_ema_ab.txt):

  kernels  the --workload (C2) model's parameters behind the optimizer's tables: --reps launches between two device events of
           s2f_ema_update in its copy form (8 B per element), its lerp form with the drift partials (12 B per element) and without
           them, and of s2f_ema_swap (16 B per element); microseconds per launch and the rate that makes.
  time     graph.GraphedStep(headline loss, optimizer=FlatAdamW) -- the iteration `bench.py --optimizer` captures -- twice over one
           model: `none` built without the argument (the parent commit's iteration, launch for launch), `ema` with
           ema=dict(type='ExpMomentumEMA', momentum=0.0002, gamma=2000): --iters iterations per run after a warm-up, --runs runs per
           variant, alternated in one process; median and spread (max - min) of milliseconds per iteration.

    python tools/weight_ema_ab.py [--workload C2] [--iters 100] [--runs 3] > profiles/weight_ema_ab.txt"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spike2former_amd as s2f                                    # noqa: E402
from spike2former_amd import ops                                  # noqa: E402

EMA = dict(type="ExpMomentumEMA", momentum=0.0002, gamma=2000)


def model_of(workload):
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.init_utils import seeded_init
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg(workload))).cuda().train()
    s2f.set_keep_membrane(model, False)
    return model, FlatGradAllReduce(model.parameters(), 1)


def optimizer_of(model, red, **kw):
    """the optimizer of `bench.py --optimizer`"""
    from spike2former_amd.train import FlatAdamW
    return FlatAdamW(model, red, lr=0.001, betas=(0.9, 0.999), weight_decay=0.005, clip_grad=dict(max_norm=0.01, norm_type=2),
                     paramwise_cfg=dict(custom_keys={"backbone": dict(lr_mult=0.1, decay_mult=1.0),
                                                     "query_embed": dict(lr_mult=1.0, decay_mult=0.0),
                                                     "query_feat": dict(lr_mult=1.0, decay_mult=0.0),
                                                     "level_embed": dict(lr_mult=1.0, decay_mult=0.0)}), **kw)


def kernels(args):
    model, red = model_of(args.workload)
    optim = optimizer_of(model, red, ema=EMA)
    ema = optim.ema
    n = sum(p.numel() for p in optim.params)

    def update(count, partials):
        def fn():
            ops.ema_update(optim.slots, optim.chunks, ema.ema, optim.state, ema.table, 0, 1, partials)
        optim.state[4] = float(count)
        return fn

    def per_call_us(fn):
        for _ in range(10):
            fn()
        out = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) / args.reps * 1e3)
        return dict(median_us=round(statistics.median(out), 2), spread_us=round(max(out) - min(out), 2))
    got = dict(copy=per_call_us(update(1, ema.partials)), lerp=per_call_us(update(5, ema.partials)),
               lerp_without_partials=per_call_us(update(5, None)),
               swap=per_call_us(lambda: ops.ema_swap(optim.slots, optim.chunks, ema.ema)))          # (an even number of swaps)
    rate = {f"{k}_GB_per_s": round(b * n / got[k]["median_us"] / 1e3, 1)
            for k, b in (("copy", 8), ("lerp", 12), ("lerp_without_partials", 12), ("swap", 16))}
    print(json.dumps(dict(kernels=dict(workload=args.workload, elements=n, tensors=len(optim.params), chunks=int(optim.chunks.shape[0]),
                                       table_entries=int(ema.table.numel()), reps_between_events=args.reps, **got, **rate))), flush=True)


def timing(args):
    from spike2former_amd.graph import GraphedStep
    model, red = model_of(args.workload)
    w = s2f.WORKLOADS[args.workload]
    img = torch.randn(w["B"], 3, w["H"], w["W"], generator=torch.Generator().manual_seed(1000)).cuda()
    red.install_sinks()
    s2f.reset_net(model); red.zero()                       # one eager step: which gradients arrive through a sink (as bench.py)
    s2f.headline_loss(*model(img)).backward()
    ops.wgrad_join(); red.gather(); red.compact()
    for p in model.parameters():
        p.grad = None
    gc.collect()
    start = {k: v.clone() for k, v in model.state_dict().items()}
    optims = {"none": optimizer_of(model, red), "ema": optimizer_of(model, red, ema=EMA)}
    steps = {}
    for name, optim in optims.items():
        steps[name] = GraphedStep(model, s2f.headline_loss, img, grad_buffer=red, warmup=2, optimizer=optim)
        gc.collect()

    def run(name):
        optim, step = optims[name], steps[name]
        model.load_state_dict(start)
        optim.exp_avg.zero_(), optim.exp_avg_sq.zero_(), optim.state.zero_()
        optim.mark_updated()
        for _ in range(4):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.iters * 1e3
    ms = {name: [] for name in steps}
    for _ in range(args.runs):
        for name in steps:
            ms[name].append(run(name))
    rows = {v: dict(median_ms=round(statistics.median(x), 4), spread_ms=round(max(x) - min(x), 4), runs_ms=[round(t, 4) for t in x])
            for v, x in ms.items()}
    report = optims["ema"].ema.report()
    out = dict(workload=args.workload, batch=w["B"], iters=args.iters, without=rows["none"], with_ema=rows["ema"],
               ema_minus_without_ms=round(rows["ema"]["median_ms"] - rows["none"]["median_ms"], 4),
               ema_over_without=round(rows["ema"]["median_ms"] / rows["none"]["median_ms"], 5),
               updates=float(optims["ema"].state[4]), report=report, peak_hbm_GB=round(torch.cuda.max_memory_allocated() / 1e9, 2))
    print(json.dumps(dict(time=out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--only", choices=("kernels", "time"), default=None)
    args = ap.parse_args()
    ops.STRICT = True
    if args.only != "time":
        kernels(args)
        gc.collect()
        torch.cuda.empty_cache()
    if args.only != "kernels":
        timing(args)


if __name__ == "__main__":
    main()
