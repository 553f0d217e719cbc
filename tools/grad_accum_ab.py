"""What gradient accumulation (FlatAdamW(accumulative_counts=k), train.GradAccum) costs per iteration (profiles/grad_accum_ab.txt):

  kernels  the --workload (C2) model's gradient buffer, filled from a seed: --reps launches of s2f_grad_accumulate in its two forms
           (acc = scale * g, 8 B per element; flat = acc + scale * g, 12 B per element; both with the g^2 partials) and of
           s2f_grad_accum_stats between two device events; microseconds per launch and the rate that makes.  Run it under
           `rocprofv3 --kernel-trace --stats -- python tools/grad_accum_ab.py --only kernels` for the per-kernel table.
  time     graph.GraphedStep(headline loss, optimizer=FlatAdamW) -- the iteration `bench.py --optimizer` captures -- twice over one
           model: `k1` captured with the update inside the graph (no argument: the parent commit's iteration), `k` with
           accumulative_counts=--counts (the capture ends with the packing; add / update / stats follow eagerly): --iters
           iterations per run after a warm-up, --runs runs per variant, alternated in one process; median and spread (max - min)
           of milliseconds per iteration.

    python tools/grad_accum_ab.py [--workload C2] [--counts 4] [--iters 100] [--runs 3] > profiles/grad_accum_ab.txt"""
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
from spike2former_amd._lib import check, lib                      # noqa: E402


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
    optim = optimizer_of(model, red, accumulative_counts=args.counts)
    acc = optim.accum
    n = red.flat.numel()
    red.flat.copy_(torch.randn(n, generator=torch.Generator().manual_seed(3)).cuda() * 1e-3)
    stream = torch.cuda.current_stream().cuda_stream
    scale = 1.0 / args.counts

    def first():
        check(lib.s2f_grad_accumulate(red.flat.data_ptr(), None, acc.acc.data_ptr(), n, scale, acc.micro[0].data_ptr(), stream), "first")

    def last():
        check(lib.s2f_grad_accumulate(red.flat.data_ptr(), acc.acc.data_ptr(), red.flat.data_ptr(), n, scale, acc.micro[1].data_ptr(), stream),
              "last")

    def stats():
        check(lib.s2f_grad_accum_stats(acc.micro.data_ptr(), args.counts, optim.partials.data_ptr(), acc.parts, acc.stats.data_ptr(), stream),
              "stats")

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
    got = dict(first=per_call_us(first), last=per_call_us(last), stats=per_call_us(stats))
    out = dict(workload=args.workload, elements=n, partials=acc.parts, counts=args.counts, reps_between_events=args.reps, **got,
               first_GB_per_s=round(8 * n / got["first"]["median_us"] / 1e3, 1), last_GB_per_s=round(12 * n / got["last"]["median_us"] / 1e3, 1))
    print(json.dumps(dict(kernels=out)), flush=True)


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
    optims = {"k1": optimizer_of(model, red), "k": optimizer_of(model, red, accumulative_counts=args.counts)}
    steps = {}
    for name, optim in optims.items():
        steps[name] = GraphedStep(model, s2f.headline_loss, img, grad_buffer=red, warmup=2, optimizer=optim)
        gc.collect()

    def run(name):
        optim, step = optims[name], steps[name]
        model.load_state_dict(start)
        optim.exp_avg.zero_(), optim.exp_avg_sq.zero_(), optim.state.zero_()
        if optim.accum is not None:
            optim.accum.count = 0
        optim.mark_updated()
        for _ in range(2 * args.counts):
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
    k = optims["k"]
    out = dict(workload=args.workload, batch=w["B"], iters=args.iters, counts=args.counts, update_in_graph=rows["k1"], accumulating=rows["k"],
               accumulating_minus_in_graph_ms=round(rows["k"]["median_ms"] - rows["k1"]["median_ms"], 4),
               accumulating_over_in_graph=round(rows["k"]["median_ms"] / rows["k1"]["median_ms"], 5),
               updates_in_graph=float(optims["k1"].state[4]), updates_accumulating=float(k.state[4]),
               stats=[float(v) for v in k.accum.stats.cpu()], peak_hbm_GB=round(torch.cuda.max_memory_allocated() / 1e9, 2))
    print(json.dumps(dict(time=out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--counts", type=int, default=4)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--only", choices=("kernels", "time"), default=None)
    args = ap.parse_args()
    if args.counts < 2:
        raise SystemExit("grad_accum_ab.py: --counts is at least 2")
    ops.STRICT = True
    if args.only != "time":
        kernels(args)
        gc.collect()
        torch.cuda.empty_cache()
    if args.only != "kernels":
        timing(args)


if __name__ == "__main__":
    main()
