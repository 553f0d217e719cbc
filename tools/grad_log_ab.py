"""What logging per-parameter gradient, weight and update norms from inside the step costs (profiles/grad_log_ab.txt):

  kernels  FlatAdamW over the --workload (C2) model's gradient buffer, filled from a seed: after a few updates, --reps eager appends
           (ops.grad_log_append: s2f_grad_log_partials + s2f_grad_log_rows) and as many of each launch alone between two device
           events; microseconds per launch, the bytes the partial launch reads and the rate that makes.  Run it under
           `rocprofv3 --kernel-trace --stats -- python tools/grad_log_ab.py --only kernels` for the per-kernel table.
  time     graph.GraphedStep(headline loss, optimizer=FlatAdamW) -- the iteration `bench.py --optimizer` captures -- twice over one
           model and one optimizer: captured without a log, and captured with FlatAdamW.attach_grad_log(GradLog): --iters replays
           per run after a warm-up, --runs runs per variant, alternated in one process; median and spread (max - min) of
           milliseconds per iteration.

    python tools/grad_log_ab.py [--workload C2] [--iters 100] [--runs 5] > profiles/grad_log_ab.txt"""
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


def optimizer_of(model, red):
    """the optimizer of `bench.py --optimizer`"""
    from spike2former_amd.train import FlatAdamW
    return FlatAdamW(model, red, lr=0.001, betas=(0.9, 0.999), weight_decay=0.005, clip_grad=dict(max_norm=0.01, norm_type=2),
                     paramwise_cfg=dict(custom_keys={"backbone": dict(lr_mult=0.1, decay_mult=1.0),
                                                     "query_embed": dict(lr_mult=1.0, decay_mult=0.0),
                                                     "query_feat": dict(lr_mult=1.0, decay_mult=0.0),
                                                     "level_embed": dict(lr_mult=1.0, decay_mult=0.0)}))


def kernels(args):
    model, red = model_of(args.workload)
    optim = optimizer_of(model, red)
    red.flat.copy_(torch.randn(red.flat.numel(), generator=torch.Generator().manual_seed(3)).cuda() * 1e-3)
    log = optim.attach_grad_log(s2f.GradLog(optim, window=64))
    for _ in range(3):
        optim.step()          # (moments that are not zero; three rows)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    nspans, n = log.spans.shape[0], log.n

    def partials():
        check(lib.s2f_grad_log_partials(optim.slots.data_ptr(), optim.hyper.data_ptr(), log.spans.data_ptr(), nspans, red.flat.data_ptr(),
                                        optim.exp_avg.data_ptr(), optim.exp_avg_sq.data_ptr(), optim.state.data_ptr(), optim.eps,
                                        log.partials.data_ptr(), stream), "s2f_grad_log_partials")

    def rows():
        check(lib.s2f_grad_log_rows(log.spans.data_ptr(), nspans, log.partials.data_ptr(), n, log.ring.data_ptr(), log.window,
                                    log.streak.data_ptr(), log.patience, log.head.data_ptr(), stream), "s2f_grad_log_rows")

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
    elems = int(sum(p.numel() for p in optim.params))
    got = dict(partials=per_call_us(partials), rows=per_call_us(rows), append=per_call_us(log.append))
    read = log.read()
    spans_per = torch.bincount(log.spans[:, 0].long()).max().item()
    out = dict(workload=args.workload, parameters=n, elements=elems, spans=nspans, most_spans_of_one_parameter=int(spans_per),
               bytes_read_by_partials=16 * elems, reps_between_events=args.reps, **got,
               partials_GB_per_s=round(16 * elems / got["partials"]["median_us"] / 1e3, 1), rows_in_ring=read.count,
               total_grad_norm_last=float(read.total_grad_norm[-1]), optimizer_grad_norm=float(optim.grad_norm))
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
    optim = optimizer_of(model, red)
    for p in model.parameters():
        p.grad = None
    gc.collect()
    start = {k: v.clone() for k, v in model.state_dict().items()}
    steps = {}
    for name in ("off", "on"):          # (the step without the log first: its capture holds no append whatever is attached later)
        if name == "on":
            optim.attach_grad_log(s2f.GradLog(optim, window=64))
        steps[name] = GraphedStep(model, s2f.headline_loss, img, grad_buffer=red, warmup=2, optimizer=optim)
        gc.collect()

    def run(name):
        model.load_state_dict(start)
        optim.exp_avg.zero_(), optim.exp_avg_sq.zero_(), optim.state.zero_()
        optim.mark_updated()
        step = steps[name]
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.iters * 1e3
    ms = {"off": [], "on": []}
    before = optim.grad_log.read(consume=False).count
    for _ in range(args.runs):
        for name in ("off", "on"):
            ms[name].append(run(name))
    rows = {v: dict(median_ms=round(statistics.median(x), 4), spread_ms=round(max(x) - min(x), 4), runs_ms=[round(t, 4) for t in x])
            for v, x in ms.items()}
    read = optim.grad_log.read()
    out = dict(workload=args.workload, batch=w["B"], iters=args.iters, grad_log_off=rows["off"], grad_log_on=rows["on"],
               on_minus_off_ms=round(rows["on"]["median_ms"] - rows["off"]["median_ms"], 4),
               on_over_off=round(rows["on"]["median_ms"] / rows["off"]["median_ms"], 5), parameters=optim.grad_log.n,
               rows_appended=read.count - before, rows_expected=args.runs * (args.iters + 5),
               total_grad_norm_last=float(read.total_grad_norm[-1]), optimizer_grad_norm=float(optim.grad_norm))
    print(json.dumps(dict(time=out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
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
