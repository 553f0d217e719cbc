"""What monitoring the firing rates from inside the captured step changes (profiles/firing_log_ab.txt, docs/EXPERIMENTS.md):

  arith    graph.GraphedHungarianStep(assign="device", optimizer=FlatAdamW) at --arith-workload (C1_64), TWICE with firing=None (the
           step as it was: the reference, and its own run-to-run spread) and once with firing=FiringLog(model): --arith-iters
           iterations each from the same weights and zeroed moments -- the logged terms of every iteration and every tensor of the
           state afterwards, compared bit by bit against the first run
  time     the same two steps at --workload (C2): --iters replays per run after a warm-up, --runs runs per variant, alternated;
           median and spread (max - min) of milliseconds per iteration, and the neurons watched

Attached counters take the memoised, pre-fired and fused-neuron routes out of the step (their `stats is None` guards) and add one
launch; this measures what that costs, and whether the other routes compute the same bits.

    python tools/firing_log_ab.py [--workload C2] [--iters 100] [--runs 3] > profiles/firing_log_ab.txt"""
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
from tools.probe_lsa import bench_maps                            # noqa: E402


def build(workload):
    """-> (model, optimizer, start state, {"off": step, "on": step}, the FiringLog) as bench.py --loss hungarian builds its step"""
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.graph import GraphedHungarianStep
    from spike2former_amd.init_utils import seeded_init
    from spike2former_amd.train import FlatAdamW
    w = s2f.WORKLOADS[workload]
    B = w["B"]
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg(workload))).cuda().train()
    s2f.set_keep_membrane(model, False)
    red = FlatGradAllReduce(model.parameters(), 1)
    red.install_sinks()
    img = torch.randn(B, 3, w["H"], w["W"], generator=torch.Generator().manual_seed(1000)).cuda()
    seg = bench_maps(w, B, "synthetic", classes=min(10, w["K"])).cuda()
    s2f.reset_net(model); red.zero()                       # one eager step: which gradients arrive through a sink (as bench.py)
    sum(model(img, [seg[i] for i in range(B)], mode="loss").values()).backward()
    ops.wgrad_join(); red.gather(); red.compact()
    for p in model.parameters():
        p.grad = None
    gc.collect()
    optim = FlatAdamW(model, red, lr=0.001, betas=(0.9, 0.999), weight_decay=0.005, clip_grad=dict(max_norm=0.01, norm_type=2))
    start = {k: v.clone() for k, v in model.state_dict().items()}
    firing = s2f.FiringLog(model, window=64, patience=1000)
    steps, logs = {}, {}
    for name in ("off", "on"):          # (the step without counters first: the other one attaches them for good)
        logs[name] = s2f.TrainLog(window=64)
        steps[name] = GraphedHungarianStep(model, img, seg, red, warmup=2, optimizer=optim, assign="device", log=logs[name],
                                           firing=firing if name == "on" else None)
        steps[name].outs = tuple(o.detach() for o in steps[name].outs)          # no autograd graph alive under the next capture
        gc.collect()
    return model, optim, start, steps, logs, firing


def restart(model, optim, start):
    model.load_state_dict(start)
    optim.exp_avg.zero_(), optim.exp_avg_sq.zero_(), optim.state.zero_()
    optim.mark_updated()
    torch.cuda.synchronize()


def arith(args):
    model, optim, start, steps, logs, firing = build(args.arith_workload)
    got = {}
    for run, name in (("off", "off"), ("off_again", "off"), ("on", "on")):
        restart(model, optim, start)
        before = logs[name].read().count
        for _ in range(args.arith_iters):
            steps[name]()
        steps[name].check()
        read = logs[name].read()
        got[run] = (read.names, read.rows[-(read.count - before):].copy(), {k: v.clone() for k, v in model.state_dict().items()},
                    optim.exp_avg.clone(), optim.exp_avg_sq.clone())
    names, rows0, sd0, m0, v0 = got["off"]

    def against_off(run):
        _, rows1, sd1, m1, v1 = got[run]
        terms = {n: dict(equal=bool((rows0[:, j] == rows1[:, j]).all()), max_abs_diff=float(abs(rows0[:, j] - rows1[:, j]).max()),
                         first_iteration_that_differs=next((i + 1 for i in range(len(rows0)) if rows0[i, j] != rows1[i, j]), None),
                         off=[float(x) for x in rows0[:, j]], this=[float(x) for x in rows1[:, j]]) for j, n in enumerate(names)}
        differ = [k for k in sd0 if not torch.equal(sd0[k], sd1[k])]
        worst = max((float((sd0[k].double() - sd1[k].double()).abs().max()) for k in differ), default=0.0)
        return dict(terms_bit_identical=all(t["equal"] for t in terms.values()), state_tensors_that_differ=len(differ),
                    first_that_differ=differ[:3], state_max_abs_diff=worst, exp_avg_equal=bool(torch.equal(m0, m1)),
                    exp_avg_sq_equal=bool(torch.equal(v0, v1)), terms=terms)
    read = firing.read()
    out = dict(workload=args.arith_workload, iters=args.arith_iters, neurons=firing.n, watched=int((read.elems > 0).sum()),
               state_tensors=len(sd0), firing_rows=read.count, firing_mean_rate=float(read.rates()[:, read.elems > 0].mean()),
               off_again_against_off=against_off("off_again"), on_against_off=against_off("on"))
    print(json.dumps(dict(arith=out)), flush=True)
    firing.detach()


def timing(args):
    model, optim, start, steps, logs, firing = build(args.workload)

    def run(name):
        restart(model, optim, start)
        step = steps[name]
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.iters * 1e3
        step.check()
        return ms
    ms = {"off": [], "on": []}
    for _ in range(args.runs):
        for name in ("off", "on"):
            ms[name].append(run(name))
    rows = {v: dict(median_ms=round(statistics.median(x), 4), spread_ms=round(max(x) - min(x), 4), runs_ms=[round(t, 4) for t in x])
            for v, x in ms.items()}
    read = firing.read()
    out = dict(workload=args.workload, batch=s2f.WORKLOADS[args.workload]["B"], iters=args.iters, firing_off=rows["off"],
               firing_on=rows["on"], on_minus_off_ms=round(rows["on"]["median_ms"] - rows["off"]["median_ms"], 4),
               on_over_off=round(rows["on"]["median_ms"] / rows["off"]["median_ms"], 4),
               neurons=firing.n, watched=int((read.elems > 0).sum()), firing_rows=read.count,
               first_dead=read.first_dead, firing_mean_rate=float(read.rates()[:, read.elems > 0].mean()))
    print(json.dumps(dict(time=out)), flush=True)
    firing.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--arith-workload", default="C1_64")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--arith-iters", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", choices=("arith", "time"), default=None)
    args = ap.parse_args()
    ops.STRICT = True
    if args.only != "time":
        arith(args)
        gc.collect()
        torch.cuda.empty_cache()
    if args.only != "arith":
        timing(args)


if __name__ == "__main__":
    main()
