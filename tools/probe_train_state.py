"""What the training loop's two device-side pieces cost at the bench's C2 model (profiles/train_state_timing.txt):

  step     graph.GraphedHungarianStep(assign="device", optimizer=FlatAdamW), single process, --iters replays per run after a warm-up,
           --runs runs per variant, the variants alternated:
             (a) log=None, no snapshot                      -- the step as it was: the yardstick
             (b) the captured ops.train_log_append          -- one more launch at the end of the graph
             (c) (b) + TrainState.snapshot() and a background write every --every iterations
             (d) (c) with async_write=False                 -- what the writer thread buys
           median and spread (max - min) of milliseconds per iteration
  kernel   s2f_state_copy over the C2 table: the dispatch packets' own timestamps (s2f_time_next_call), median of --reps launches,
           against 2 x 4 bytes per word, as a share of the HBM peak

    python tools/probe_train_state.py [--workload C2] [--iters 200] [--runs 3] [--every 50] > profiles/train_state_timing.txt"""
import argparse
import ctypes
import gc
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spike2former_amd as s2f                                    # noqa: E402
from spike2former_amd import ops                                  # noqa: E402
from spike2former_amd._lib import lib                             # noqa: E402
from tools.probe_lsa import bench_maps                            # noqa: E402

HBM_PEAK_GBPS = 8000.0          # MI355X, as bench.py's roofline rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--every", type=int, default=50)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.graph import GraphedHungarianStep
    from spike2former_amd.init_utils import seeded_init
    from spike2former_amd.train import FlatAdamW
    ops.STRICT = True
    w = s2f.WORKLOADS[args.workload]
    B = w["B"]
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg(args.workload))).cuda().train()
    s2f.set_keep_membrane(model, False)
    red = FlatGradAllReduce(model.parameters(), 1)
    red.install_sinks()
    img = torch.randn(B, 3, w["H"], w["W"], generator=torch.Generator().manual_seed(1000)).cuda()
    seg = bench_maps(w, B, "synthetic").cuda()
    s2f.reset_net(model); red.zero()                       # one eager step: which gradients arrive through a sink (as bench.py)
    sum(model(img, [seg[i] for i in range(B)], mode="loss").values()).backward()
    ops.wgrad_join(); red.gather(); red.compact()
    for p in model.parameters():
        p.grad = None
    gc.collect()
    optim = FlatAdamW(model, red, lr=0.001, betas=(0.9, 0.999), weight_decay=0.005, clip_grad=dict(max_norm=0.01, norm_type=2))
    start = {k: v.clone() for k, v in model.state_dict().items()}
    log = s2f.TrainLog(window=64)
    steps = {}
    for name, lg in (("plain", None), ("logged", log)):
        steps[name] = GraphedHungarianStep(model, img, seg, red, warmup=2, optimizer=optim, assign="device", log=lg)
        steps[name].outs = tuple(o.detach() for o in steps[name].outs)          # no autograd graph alive under the next capture
        gc.collect()
    tmp = tempfile.mkdtemp(prefix="s2f_train_state_")
    path = os.path.join(tmp, "probe.pth")

    def run(variant):
        model.load_state_dict(start)          # every run from the same weights
        optim.exp_avg.zero_(), optim.exp_avg_sq.zero_(), optim.state.zero_()
        step = steps["plain" if variant == "a" else "logged"]
        state = s2f.TrainState(model, optim, async_write=variant == "c") if variant in "cd" else None
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(args.iters):
            step()
            if state is not None and (it + 1) % args.every == 0:
                state.snapshot()
                state.write(path, meta=dict(iter=it + 1))
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.iters * 1e3
        if state is not None:
            state.close()          # (a write still running is not part of the iterations' time: the loop would run on)
        step.check()
        return ms

    ms = {v: [] for v in "abcd"}
    for _ in range(args.runs):
        for v in "abcd":
            ms[v].append(run(v))
    read = log.read()
    assert read.first_nonfinite is None, read
    rows = {v: dict(median_ms=round(statistics.median(x), 4), spread_ms=round(max(x) - min(x), 4), runs_ms=[round(t, 4) for t in x])
            for v, x in ms.items()}
    a = rows["a"]
    out = dict(workload=args.workload, batch=B, iters=args.iters, every=args.every,
               a_plain=rows["a"], b_logged=rows["b"], c_snapshot_async=rows["c"], d_snapshot_sync=rows["d"],
               b_minus_a_ms=round(rows["b"]["median_ms"] - a["median_ms"], 4), c_minus_a_ms=round(rows["c"]["median_ms"] - a["median_ms"], 4),
               d_minus_a_ms=round(rows["d"]["median_ms"] - a["median_ms"], 4),
               b_within_spread_of_a=bool(abs(rows["b"]["median_ms"] - a["median_ms"]) <= a["spread_ms"]),
               c_within_spread_of_a=bool(abs(rows["c"]["median_ms"] - a["median_ms"]) <= a["spread_ms"]),
               file_bytes=os.path.getsize(path), log_terms=len(read.names))
    print(json.dumps(dict(step=out)), flush=True)

    # the kernel alone
    state = s2f.TrainState(model, optim)
    words = int(state.slots[:, 2].sum())
    e0, e1 = lib.s2f_event_create(), lib.s2f_event_create()
    us = []
    for direction in (False, True):
        got = []
        for i in range(args.reps + 5):
            lib.s2f_time_next_call(e0, e1)
            ops.state_copy(state.tensors, state.slots, state.chunks, state.flat, to_params=direction)
            torch.cuda.synchronize()
            t = ctypes.c_double()
            lib.s2f_event_elapsed_us(e0, e1, ctypes.byref(t))
            if i >= 5:
                got.append(t.value)
        us.append(statistics.median(got))
    lib.s2f_event_destroy(e0), lib.s2f_event_destroy(e1)
    rows = dict(tensors=len(state.tensors), chunks=int(state.chunks.shape[0]), words=words, moved_bytes=8 * words,
                unaligned_tensors=sum(1 for t in state.tensors if t.data_ptr() % 16),
                to_flat_us=round(us[0], 2), to_params_us=round(us[1], 2),
                to_flat_GBps=round(8 * words / us[0] * 1e-3, 1), to_params_GBps=round(8 * words / us[1] * 1e-3, 1),
                to_flat_share_of_hbm_peak=round(8 * words / us[0] * 1e-3 / HBM_PEAK_GBPS, 4), hbm_peak_GBps=HBM_PEAK_GBPS)
    print(json.dumps(dict(kernel=rows)), flush=True)
    os.remove(path)
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
