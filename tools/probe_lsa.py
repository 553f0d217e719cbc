"""Measurement of the device-side Hungarian assignment on one MI355X (docs/EXPERIMENTS.md "Device-side assignment"):

  kernel   s2f_lsa_tables alone at C2's sizes (L = 7, B = 2, Q = 100, K = 150) for n_present in {1, 10, 40, 100, 150}, on uniform costs
           and on the "every query nearly alike" family (n (n + 1) / 2 column scans at n >= Q), with the fp64 cost tile in LDS and
           re-read as fp32 from L2 (ops.lsa_tables(tile_l2=True)): the dispatch packets' own timestamps (s2f_time_next_call: begin of the first
           launch to end of the second), median of --reps launches after --warmup.  The tables are compared with the host route's first.
  step     graph.GraphedHungarianStep at --workload (C2), batch 2, assign="host" against assign="device", no optimizer, on (a) the bench's
           synthetic maps with 10 classes per image and (b) noise maps with every class present: windows of at least --seconds of
           replays each, closed by a synchronise, alternating host / device / host / device ...; the host route's window-to-window
           spread is the A/A figure of the run.

    python tools/probe_lsa.py [--workload C2] [--seconds 1.0] [--windows 4] [--out FILE.json] [--skip-step]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spike2former_amd as s2f                                    # noqa: E402
from spike2former_amd import ops                                  # noqa: E402
from spike2former_amd._lib import check, lib                      # noqa: E402


def kernel_rows(reps, warmup):
    from spike2former_amd.loss import MaskFormerLoss
    L, B, Q, K = 7, 2, 100, 150
    crit = MaskFormerLoss(K, Q)
    e0, e1, us = lib.s2f_event_create(), lib.s2f_event_create(), ctypes.c_double()
    rows = []
    for n in (1, 10, 40, 100, 150):
        for family in ("uniform", "queries_alike"):
            rng = np.random.default_rng(n)
            count = np.zeros((B, 256), np.float32)
            cost = rng.random((L, B, Q, K), np.float32) * 22 - 1
            for b in range(B):
                present = np.sort(rng.choice(K, n, replace=False))
                count[b, present] = 100
                if family == "queries_alike":
                    for l in range(L):
                        cost[l, b][:, present] = (5 * rng.random(n)[None, :] + 1e-4 * rng.random((Q, n))).astype(np.float32)
            want = crit.match_tables(cost, count)
            t0 = time.perf_counter()
            for _ in range(3):
                crit.match_tables(cost, count)
            host_us = (time.perf_counter() - t0) / 3 * 1e6
            dc, dn = torch.from_numpy(cost).cuda(), torch.from_numpy(count).cuda()
            row = dict(n_present=n, family=family, host_scipy_us=round(host_us, 1))
            for tile in ("lds", "l2"):
                out = ops.lsa_tables(dc, dn, K, tile_l2=tile == "l2")
                torch.cuda.synchronize()
                same = all(np.array_equal(g.cpu().numpy(), w_) for g, w_ in zip(out[:3], want))
                ts = []
                for i in range(warmup + reps):
                    lib.s2f_time_next_call(e0, e1)
                    ops.lsa_tables(dc, dn, K, out=out, tile_l2=tile == "l2")
                    torch.cuda.synchronize()
                    check(lib.s2f_event_elapsed_us(e0, e1, ctypes.byref(us)), "s2f_event_elapsed_us")
                    if i >= warmup:
                        ts.append(us.value)
                row[f"{tile}_us"], row[f"{tile}_us_min"], row[f"{tile}_tables_are_scipys"] = round(statistics.median(ts), 2), round(min(ts), 2), same
            rows.append(row)
            print(json.dumps(row), flush=True)
    lib.s2f_event_destroy(e0)
    lib.s2f_event_destroy(e1)
    return rows


def bench_maps(w, B, kind, classes=10):
    """the label maps of bench.py --loss hungarian (--gt noise / the synthetic regions), same seeds"""
    gen = torch.Generator().manual_seed(1)
    if kind == "noise":
        return torch.randint(0, w["K"], (B, 1, w["H"], w["W"]), generator=gen)
    seg = torch.empty(B, 1, w["H"], w["W"], dtype=torch.int64)
    for i in range(B):
        cl = torch.randperm(w["K"], generator=gen)[:classes]
        ys = torch.sort(torch.randint(1, w["H"], (3,), generator=gen)).values.tolist()
        plane = torch.empty(w["H"], w["W"], dtype=torch.int64)
        k = 0
        for y0, y1 in zip([0] + ys, ys + [w["H"]]):
            xs = torch.sort(torch.randint(1, w["W"], (max(classes // 4, 1),), generator=gen)).values.tolist()
            for x0, x1 in zip([0] + xs, xs + [w["W"]]):
                plane[y0:y1, x0:x1] = cl[k % classes]
                k += 1
        seg[i, 0] = plane
    return seg


def window_ms(step, seconds):
    """replays for at least `seconds`, closed by a synchronise -> ms per step"""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(8):
            step()
        n += 8
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e3


def step_rows(workload, seconds, windows):
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.graph import GraphedHungarianStep
    from spike2former_amd.init_utils import seeded_init
    w = s2f.WORKLOADS[workload]
    B = 2
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg(workload))).cuda().train()
    s2f.set_keep_membrane(model, False)
    red = FlatGradAllReduce(model.parameters(), 1)
    red.install_sinks()
    img = torch.randn(B, 3, w["H"], w["W"], generator=torch.Generator().manual_seed(1000)).cuda()
    segs = {"synthetic_10_classes": bench_maps(w, B, "synthetic").cuda(), "noise_all_classes": bench_maps(w, B, "noise").cuda()}
    first = segs["synthetic_10_classes"]
    s2f.reset_net(model); red.zero()                       # one eager step: which gradients arrive through a sink (as bench.py)
    sum(model(img, [first[i] for i in range(B)], mode="loss").values()).backward()
    ops.wgrad_join(); red.gather(); red.compact()
    for p in model.parameters():
        p.grad = None
    import gc
    gc.collect()
    steps = {}
    for a in ("host", "device"):
        steps[a] = GraphedHungarianStep(model, img, first, red, warmup=2, assign=a)
        # a replay needs the static tensors, not the autograd graph recorded at capture: drop it, so that no graph of an earlier step
        # is alive while the next one is captured (see graph.GraphedSplitStep)
        steps[a].outs = tuple(o.detach() for o in steps[a].outs)
        gc.collect()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    rows = []
    for name, seg in segs.items():
        got = {}
        for a, st in steps.items():
            for _ in range(3):                             # every shape warmed up on both routes
                model.load_state_dict(state)               # (BatchNorm running statistics feed the padded convolutions' border value)
                out = st(img, seg)
            steps["device"].check()
            torch.cuda.synchronize()
            got[a] = {k: float(v) for k, v in out.items()}
        gap = max(abs(got["device"][k] - got["host"][k]) / max(abs(got["host"][k]), 1e-3) for k in got["host"])
        ms = {"host": [], "device": []}
        for _ in range(windows):
            for a in ("host", "device"):
                ms[a].append(window_ms(steps[a], seconds))
        steps["device"].check()
        h, d = statistics.median(ms["host"]), statistics.median(ms["device"])
        row = dict(maps=name, workload=workload, batch=B, host_ms=round(h, 4), device_ms=round(d, 4), device_minus_host_ms=round(d - h, 4),
                   host_windows_ms=[round(v, 4) for v in ms["host"]], device_windows_ms=[round(v, 4) for v in ms["device"]],
                   host_aa_spread_ms=round(max(ms["host"]) - min(ms["host"]), 4), loss_rel_gap_device_vs_host=gap)
        row["device_not_slower_beyond_spread"] = bool(d <= h + row["host_aa_spread_ms"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None, help="also write the rows to this JSON file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    ops.STRICT = True
    res = dict(kernel=kernel_rows(a.reps, a.warmup))
    if not a.skip_step:
        res["step"] = step_rows(a.workload, a.seconds, a.windows)
        res["condition_synthetic_device_not_slower"] = res["step"][0]["device_not_slower_beyond_spread"]
    res["fallbacks"] = dict(ops.FALLBACKS)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
