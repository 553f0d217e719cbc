"""Measurement of `s2f_seg_confusion` on one MI355X (docs/EXPERIMENTS.md "IoUMetric"), with `s2f_seg_hist` on the same inputs as
the yardstick.  Maps with large regions, not noise: the recorded blocky cases of tests/golden/metric_iou.npz enlarged (nearest
neighbour) and cropped to 512 x 683 at K = 150 and to 1024 x 2048 at K = 19; int64 prediction, uint8 label.  Per map the three
variants -- seg_hist, seg_confusion on its automatic route (the LDS table at these K), seg_confusion with route="global" -- alternate
inside every run, --runs times:

  kernel_us   the dispatch packet's own begin / end timestamps (s2f_time_next_call): median, min and 90th percentile of --reps
              launches after --warmup, per run
  replay_us   device events around --replays replays of a captured graph of --chain back-to-back launches, / (replays x chain):
              what one more launch costs in a stream that is kept full, per run

The results of the variants are compared first (both routes give one matrix; its diagonal is the histogram's first row).

    python tools/probe_seg_confusion.py [--reps 200] [--warmup 20] [--runs 5] [--out FILE.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spike2former_amd import ops                                  # noqa: E402
from spike2former_amd._lib import check, lib                      # noqa: E402

MAPS = (("k150_blocky", 150, 512, 683), ("k19_blocky", 19, 1024, 2048))


def enlarged(a, H, W):
    f = max(-(-H // a.shape[0]), -(-W // a.shape[1]))
    return np.ascontiguousarray(np.repeat(np.repeat(a, f, axis=0), f, axis=1)[:H, :W])


def kernel_us(fn, reps, warmup):
    e0, e1, us, out = lib.s2f_event_create(), lib.s2f_event_create(), ctypes.c_double(), []
    for i in range(warmup + reps):
        lib.s2f_time_next_call(e0, e1)
        fn()
        torch.cuda.synchronize()
        check(lib.s2f_event_elapsed_us(e0, e1, ctypes.byref(us)), "s2f_event_elapsed_us")
        if i >= warmup:
            out.append(us.value)
    lib.s2f_event_destroy(e0)
    lib.s2f_event_destroy(e1)
    out.sort()
    return statistics.median(out), out[0], out[int(0.9 * (len(out) - 1))]


def replay_us(fn, chain, replays, warmup):
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):          # one stream, a single chain
        for _ in range(chain):
            fn()
    for _ in range(warmup):
        graph.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (replays * chain)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--chain", type=int, default=50)
    ap.add_argument("--replays", type=int, default=40)
    ap.add_argument("--out", default=None, help="also write the lines to this text file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    ops.STRICT = True
    g = np.load(os.path.join(ROOT, "tests", "golden", "metric_iou.npz"), allow_pickle=False)
    lines = [f"s2f_seg_confusion vs s2f_seg_hist, {torch.cuda.get_device_name(0)}; reps {a.reps}, warmup {a.warmup}, runs {a.runs}, "
             f"graph of {a.chain} launches x {a.replays} replays; microseconds per launch",
             f"{'map':>12} {'K':>4} {'variant':>16} {'run':>3} {'kernel med':>10} {'min':>8} {'p90':>8} {'replay':>8}"]
    print("\n".join(lines), flush=True)
    for name, K, H, W in MAPS:
        pred = torch.from_numpy(enlarged(g[f"{name}.pred"], H, W).astype(np.int64)).cuda()
        label = torch.from_numpy(enlarged(g[f"{name}.label"], H, W)).cuda()
        totals = torch.zeros(3, K, dtype=torch.int64, device="cuda")
        mats = {r: torch.zeros(K, K, dtype=torch.int64, device="cuda") for r in (None, "global")}
        variants = (("seg_hist", lambda: ops.seg_hist(pred, label, totals)),
                    ("confusion auto", lambda: ops.seg_confusion(pred, label, mats[None])),
                    ("confusion global", lambda: ops.seg_confusion(pred, label, mats["global"], route="global")))
        for _, fn in variants:
            fn()
        m = mats[None]
        # (the recorded maps hold labels outside the classes, which count in the histogram's prediction row alone: the diagonal)
        assert torch.equal(m, mats["global"]) and torch.equal(m.diagonal(), totals[0]) and int(m.sum()) > 0, name
        pairs = int((m != 0).sum())
        rows = {v: [] for v, _ in variants}
        for run in range(a.runs):
            for v, fn in variants:
                med, best, p90 = kernel_us(fn, a.reps, a.warmup)
                rep = replay_us(fn, a.chain, a.replays, 3)
                rows[v].append((med, rep))
                lines.append(f"{H}x{W:>5} {K:>6} {v:>16} {run:>3} {med:>10.2f} {best:>8.2f} {p90:>8.2f} {rep:>8.2f}")
                print(lines[-1], flush=True)
        for v, r in rows.items():
            meds, reps = [x[0] for x in r], [x[1] for x in r]
            lines.append(f"{H}x{W:>5} {K:>6} {v:>16} all  kernel median of runs {statistics.median(meds):.2f} (spread {min(meds):.2f} .. "
                         f"{max(meds):.2f}), replay {statistics.median(reps):.2f} (spread {min(reps):.2f} .. {max(reps):.2f}); "
                         f"{pairs} non-zero pairs, {H * W * 9 / statistics.median(meds) * 1e-6:.2f} TB/s of 9 B per pixel")
            print(lines[-1], flush=True)
    assert not ops.FALLBACKS, ops.FALLBACKS
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
