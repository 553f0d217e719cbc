"""Measurement of the evaluation hot path on one MI355X (docs/EXPERIMENTS.md "IoUMetric"): for 512 x 683 and 1024 x 2048 maps at K = 150
on (a) a blocky map, (b) a one-class map, (c) uniform noise --

  kernel_us       s2f_seg_hist alone: the dispatch packet's own begin / end timestamps (s2f_time_next_call), median of --reps launches
                  after --warmup; bytes moved (8 B int64 prediction + 1 B uint8 label per pixel) / time against the 8 TB/s HBM figure
  process_us      IoUMetric.process per image on the kernel path: wall clock over 10 x --reps images, ended by ONE synchronise; median of three windows
  aten_us         the same per-image work written in ATen on the GPU the way the reference scores an image (two boolean-mask gathers, the
                  equality gather, three torch.histc on float copies, three device -> host copies, float32 sums on the host), same window
  ratio           process_us / aten_us  (the condition of the record: <= 1.0 on (a))

    python tools/probe_seg_hist.py [--reps 200] [--warmup 20] [--out FILE.json]
"""
import argparse
import ctypes
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
from spike2former_amd.data_preprocessor import PixelData, SegDataSample      # noqa: E402

K, HBM = 150, 8.0e12


def make(kind, H, W, gen):
    if kind == "one_class":
        return torch.full((H, W), 7, dtype=torch.int64), torch.full((H, W), 7, dtype=torch.uint8)
    if kind == "noise":
        label = torch.randint(0, K, (H, W), generator=gen)
        label[torch.rand(H, W, generator=gen) < 0.05] = 255
        return torch.randint(0, K, (H, W), generator=gen), label.to(torch.uint8)
    bs = 32          # blocky: 32 x 32 blocks of a dozen classes, a fifth of the prediction's blocks wrong, an ignored border
    classes = torch.randperm(K, generator=gen)[:12]
    grid = classes[torch.randint(0, 12, (H // bs + 1, W // bs + 1), generator=gen)]
    wrong = classes[torch.randint(0, 12, grid.shape, generator=gen)]
    pgrid = torch.where(torch.rand(grid.shape, generator=gen) < 0.2, wrong, grid)
    up = lambda t: t.repeat_interleave(bs, 0).repeat_interleave(bs, 1)[:H, :W].contiguous()
    label = up(grid)
    label[:8] = 255
    label[:, -8:] = 255
    return up(pgrid), label.to(torch.uint8)


def aten_image(pred, label, sums):
    """one image the way the reference scores it, on the GPU"""
    mask = label != 255
    p, l = pred[mask], label[mask].to(pred)
    inter = p[p == l]
    a_i = torch.histc(inter.float(), bins=K, min=0, max=K - 1).cpu()
    a_p = torch.histc(p.float(), bins=K, min=0, max=K - 1).cpu()
    a_l = torch.histc(l.float(), bins=K, min=0, max=K - 1).cpu()
    sums[0] += a_i
    sums[1] += a_p
    sums[2] += a_l


def kernel_us(pred, label, totals, reps, warmup):
    e0, e1, us, out = lib.s2f_event_create(), lib.s2f_event_create(), ctypes.c_double(), []
    for i in range(warmup + reps):
        lib.s2f_time_next_call(e0, e1)
        ops.seg_hist(pred, label, totals)
        torch.cuda.synchronize()
        check(lib.s2f_event_elapsed_us(e0, e1, ctypes.byref(us)), "s2f_event_elapsed_us")
        if i >= warmup:
            out.append(us.value)
    lib.s2f_event_destroy(e0)
    lib.s2f_event_destroy(e1)
    return statistics.median(out), min(out)


def wall_us(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the rows to this JSON file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    ops.STRICT = True
    gen = torch.Generator().manual_seed(1)
    rows = []
    for H, W in ((512, 683), (1024, 2048)):
        for kind in ("blocky", "one_class", "noise"):
            pred, label = (t.cuda() for t in make(kind, H, W, gen))
            metric = s2f.IoUMetric()
            metric.dataset_meta = dict(classes=[str(i) for i in range(K)])
            sample = SegDataSample(gt_sem_seg=label[None])
            sample.pred_sem_seg = PixelData(pred[None])
            # same answer first (the ATen form's float32 counts are exact at these sizes)
            sums = torch.zeros(3, K)
            aten_image(pred, label, sums)
            metric.process({}, [sample])
            assert torch.equal(metric._totals.cpu(), sums.to(torch.int64)), (H, W, kind)
            med, best = kernel_us(pred, label, metric._totals, a.reps, a.warmup)
            # the two per-image forms alternate, three windows each
            proc, aten = [], []
            for _ in range(3):
                proc.append(wall_us(lambda: metric.process({}, [sample]), 10 * a.reps, a.warmup))
                aten.append(wall_us(lambda: aten_image(pred, label, sums), 10 * a.reps, a.warmup))
            nbytes = H * W * 9
            row = dict(map=f"{H}x{W}", kind=kind, kernel_us=round(med, 2), kernel_us_min=round(best, 2),
                       kernel_tb_s=round(nbytes / med * 1e-6, 3), kernel_share_of_hbm=round(nbytes / (med * 1e-6) / HBM, 3),
                       process_us=round(statistics.median(proc), 2), aten_us=round(statistics.median(aten), 2),
                       process_us_windows=[round(v, 2) for v in proc], aten_us_windows=[round(v, 2) for v in aten])
            row["ratio"] = round(row["process_us"] / row["aten_us"], 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
    ok = all(r["ratio"] <= 1.0 for r in rows if r["kind"] == "blocky")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(reps=a.reps, warmup=a.warmup, rows=rows, condition_blocky_ratio_le_1=ok, fallbacks=dict(ops.FALLBACKS)), f, indent=1)
    print(json.dumps(dict(condition_blocky_ratio_le_1=ok)))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
