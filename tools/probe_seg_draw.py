"""Measurement of `s2f_seg_draw` on one MI355X: two panels (ground truth | prediction) at 512 x 683 and 1024 x 2048, K = 150 with
about 20 classes present (32 x 32 blocks), next to the host route a user had before it --

  kernel_us   s2f_seg_draw alone: the dispatch packet's own begin / end timestamps (s2f_time_next_call); median, min and 90th
              percentile of --reps launches after --warmup, --runs times; the bytes it moves (3 B picture + 1 B uint8 annotation + 8 B
              int64 prediction read, 6 B written per pixel) over the median
  host_ms     the device-to-host copy of the prediction the host route needs, then tests/draw_ref.py (the reference's np.unique, the
              masked write per class present, the float64 blend, the truncation, the concatenation) on the host arrays: wall clock,
              median of --host-reps after one warm-up.  The picture and the annotation are taken to be on the host already.

The two panels are compared byte for byte before anything is timed.  Writes the table to --out.

    python tools/probe_seg_draw.py [--reps 200] [--warmup 20] [--runs 3] [--host-reps 5] [--out profiles/seg_draw_timing.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import draw_ref as D                                              # noqa: E402
from spike2former_amd import ops                                  # noqa: E402
from spike2former_amd._lib import check, lib                      # noqa: E402

K, PRESENT, BLOCK = 150, 20, 32


def scene(H, W, rng):
    """a noise picture, a raw annotation of 32 x 32 blocks of 20 of the 150 classes with an ignored border, and a prediction that
    has a fifth of the blocks wrong"""
    classes = rng.permutation(K)[:PRESENT]
    grid = classes[rng.integers(0, PRESENT, (H // BLOCK + 1, W // BLOCK + 1))]
    wrong = classes[rng.integers(0, PRESENT, grid.shape)]
    pgrid = np.where(rng.random(grid.shape) < 0.2, wrong, grid)
    up = lambda t: np.ascontiguousarray(np.repeat(np.repeat(t, BLOCK, 0), BLOCK, 1)[:H, :W])  # noqa: E731
    gt = (up(grid) + 1).astype(np.uint8)          # raw: the data set's indices start at 1
    gt[:8] = 0
    gt[:, -8:] = 255
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), gt, up(pgrid).astype(np.int64)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_draw_timing.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    ops.STRICT = True
    rng = np.random.default_rng(1)
    pal = rng.integers(0, 256, (K, 3), dtype=np.uint8)
    lines = [f"`python tools/probe_seg_draw.py` on one MI355X ({torch.cuda.get_device_name(0)}), one process; s2f_seg_draw, two panels, "
             f"K = {K}, {PRESENT} classes present in {BLOCK} x {BLOCK} blocks, BGR picture, uint8 raw annotation (reduce_zero_label), "
             f"int64 prediction; reps {a.reps}, warmup {a.warmup}, runs {a.runs}, host reps {a.host_reps}",
             "kernel: the dispatch packet's timestamps, microseconds; host: device-to-host copy of the prediction + tests/draw_ref.py, "
             "wall clock, milliseconds", ""]
    for H, W in ((512, 683), (1024, 2048)):
        img, gt, pred = scene(H, W, rng)
        img_d, gt_d, pred_d, pal_d = (torch.from_numpy(t).cuda() for t in (img, gt, pred, pal))
        out = torch.empty(H, 2 * W, 3, dtype=torch.uint8, device="cuda")
        draw = lambda: ops.seg_draw(img_d, pal_d, gt_d, pred_d, bgr=True, reduce_zero_label=True, out=out)  # noqa: E731
        want = D.panel(img, pal, gt, pred, bgr=True, rzl=True)
        assert np.array_equal(draw().cpu().numpy(), want), (H, W)
        nbytes = H * W * (3 + 1 + 8 + 6)
        meds = []
        for run in range(a.runs):
            med, best, p90 = kernel_us(draw, a.reps, a.warmup)
            meds.append(med)
            lines.append(f"{H:5d}x{W:5d}  run {run}  kernel med {med:8.2f}  min {best:8.2f}  p90 {p90:8.2f}")

        def host():
            return D.panel(img, pal, gt, pred_d.cpu().numpy(), bgr=True, rzl=True)
        host()
        ms = []
        for _ in range(a.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host()
            ms.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(meds)
        lines.append(f"{H:5d}x{W:5d}  all    kernel median of runs {med:.2f} us (spread {min(meds):.2f} .. {max(meds):.2f}); {nbytes} bytes "
                     f"moved (18 per pixel): {nbytes / med * 1e-6:.2f} TB/s; host route median {statistics.median(ms):.1f} ms "
                     f"(spread {min(ms):.1f} .. {max(ms):.1f}), {statistics.median(ms) * 1e3 / med:.0f} x the kernel")
        print("\n".join(lines[-a.runs - 1:]), flush=True)
    assert not ops.FALLBACKS, ops.FALLBACKS
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
