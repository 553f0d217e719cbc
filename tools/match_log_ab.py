"""What logging the assignment's figures from inside the captured step costs (profiles/match_log_ab.txt):

  time     graph.GraphedHungarianStep(assign="device", optimizer=FlatAdamW) at --workload (C2) with match_log=None (the step as it
           was) and match_log=MatchLog(): --iters replays per run after a warm-up, --runs runs per variant, alternated on the same
           box; median and spread (max - min) of milliseconds per iteration
  kernels  the log's two launches on the step's own costs, class scores and table, each alone, --kernel-iters launches back to back
           between two events: microseconds per launch of s2f_match_log_partials and s2f_match_log_rows, and the bytes they read
  row      what the replays logged: the report() keys

The log only reads the step's tensors; the two steps share the model and the optimizer and run from the same weights.

    python tools/match_log_ab.py [--workload C2] [--iters 100] [--runs 3] > profiles/match_log_ab.txt"""
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
from tools.probe_lsa import bench_maps                            # noqa: E402

VARIANTS = ("off", "on")


def build(workload):
    """-> (model, optimizer, start state, {"off" / "on": step}) as bench.py --loss hungarian builds its step"""
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
    steps = {}
    for name in VARIANTS:
        log = None if name == "off" else s2f.MatchLog(window=64)
        steps[name] = GraphedHungarianStep(model, img, seg, red, warmup=2, optimizer=optim, assign="device", log=s2f.TrainLog(window=64),
                                           match_log=log)
        steps[name].outs = tuple(o.detach() for o in steps[name].outs)          # no autograd graph alive under the next capture
        gc.collect()
    return model, optim, start, steps


def restart(model, optim, start):
    model.load_state_dict(start)
    optim.exp_avg.zero_(), optim.exp_avg_sq.zero_(), optim.state.zero_()
    optim.mark_updated()
    torch.cuda.synchronize()


def kernel_times(step, iters):
    """microseconds per launch of the log's two kernels on the step's tensors, each alone, back to back on the current stream"""
    log = step.match_log
    L, B, Q, K = log.shape
    cost = step.match_inputs[0]
    cls = step.outs[0].detach().float().contiguous()
    stream = torch.cuda.current_stream().cuda_stream

    def partials():
        check(lib.s2f_match_log_partials(cost.data_ptr(), cls.data_ptr(), step.row_class.data_ptr(), L, B, Q, K, log.partials.data_ptr(),
                                         log.usage.data_ptr(), stream), "s2f_match_log_partials")

    def rows():
        check(lib.s2f_match_log_rows(log.partials.data_ptr(), log.usage.data_ptr(), L, B, Q, log.ring.data_ptr(), log.window,
                                     log.idle.data_ptr(), log.patience, log.head.data_ptr(), stream), "s2f_match_log_rows")
    out = {}
    for name, launch in (("s2f_match_log_partials_us", partials), ("s2f_match_log_rows_us", rows)):
        for _ in range(5):
            launch()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            launch()
        b.record()
        torch.cuda.synchronize()
        out[name] = round(a.elapsed_time(b) / iters * 1e3, 2)
    matched = int((step.row_class >= 0).sum())
    # what the first launch reads at most: every logit, the table, and the cost columns of the matched classes
    out.update(workgroups=L * B, shape=dict(L=L, B=B, Q=Q, K=K), matched_pairs=matched,
               bytes_read_at_most=4 * (cls.numel() + step.row_class.numel() + cost.numel()), bytes_read=4 * (cls.numel() + step.row_class.numel() + matched * Q))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=200)
    args = ap.parse_args()
    ops.STRICT = True
    model, optim, start, steps = build(args.workload)

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
    ms = {name: [] for name in VARIANTS}
    for _ in range(args.runs):
        for name in VARIANTS:
            ms[name].append(run(name))
    rows = {v: dict(median_ms=round(statistics.median(x), 4), spread_ms=round(max(x) - min(x), 4), runs_ms=[round(t, 4) for t in x])
            for v, x in ms.items()}
    out = dict(workload=args.workload, batch=s2f.WORKLOADS[args.workload]["B"], iters=args.iters, **{f"match_log_{v}": rows[v] for v in VARIANTS},
               on_minus_off_ms=round(rows["on"]["median_ms"] - rows["off"]["median_ms"], 4))
    print(json.dumps(dict(time=out)), flush=True)
    keys, _, _ = steps["on"].match_log.report(0, 0)
    print(json.dumps(dict(row=dict(rows=steps["on"].match_log.read(consume=False).count, keys=keys))), flush=True)
    print(json.dumps(dict(kernels=kernel_times(steps["on"], args.kernel_iters))), flush=True)


if __name__ == "__main__":
    main()
