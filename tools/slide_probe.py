"""Measurement of sliding-window inference on one MI355X: the C3 model in eval mode on a seeded [1, 3, 1024, 2048] input, crop
(512, 1024), stride (341, 683) -- the Cityscapes protocol, 3 x 3 windows -- through the routes of EncoderDecoder.slide_inference:

  torch      the reference's loop (route="torch"): per window F.pad, preds +=, count_mat += 1, then preds / count_mat
  torch_2    the same arm a second time: the gap between the two medians is the noise floor of this run
  device     the device route without window_batch: one window per encode_decode call, one s2f_slide_accumulate launch per window
  batch3/9   test_cfg['window_batch'] = 3 and 9: s2f_slide_windows cuts a group, one encode_decode call at batch 3 / 9, one
             s2f_slide_accumulate launch per group, the membranes reset per group

The arms alternate iteration by iteration in ONE process (a drift of the clocks hits all of them alike); an iteration is reset_net
+ slide_inference between two device synchronisations, wall clock.  Every arm is warmed first; the peak of
torch.cuda.max_memory_allocated is taken over one warm iteration per arm, above what is allocated before it (weights, input).
Before anything is timed the device route is compared bit for bit with the torch loop.  After the arms, the two kernels on their
own at the same geometry, from the dispatch packets' timestamps (s2f_time_next_call).  Writes the table to --out.

    python tools/slide_probe.py [--iters 20] [--warmup 3] [--kernel-reps 50] [--out profiles/slide_inference_ab.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spike2former_amd as s2f                                     # noqa: E402
from spike2former_amd import ops                                   # noqa: E402
from spike2former_amd._lib import check, lib                       # noqa: E402
from spike2former_amd.init_utils import seeded_init                # noqa: E402

H, W, CROP, STRIDE = 1024, 2048, (512, 1024), (341, 683)
ARMS = (("torch", None, "torch"), ("device", None, None), ("batch3", 3, None), ("batch9", 9, None), ("torch_2", None, "torch"))


def kernel_us(fn, reps, warmup=5):
    """the durations of `reps` calls of fn (ONE C-ABI call each) from the dispatch packets' timestamps, sorted"""
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
    return sorted(out)


def kernel_lines(K, reps):
    """s2f_slide_accumulate (all nine windows in one launch; one window per launch, summed over the nine) and s2f_slide_windows
    (nine windows in one launch) on their own, with the bytes the algorithm needs over the median"""
    ny, nx, eh, ew = ops.slide_grid(H, W, CROP, STRIDE)
    nw, win, full = ny * nx, 4 * K * eh * ew, 4 * K * H * W
    logits = torch.randn(nw, 1, K, eh, ew, device="cuda")
    preds = torch.empty(1, K, H, W, device="cuda")
    img = torch.randn(1, 3, H, W, device="cuda")
    out = []
    t = kernel_us(lambda: ops.slide_accumulate(preds, logits, CROP, STRIDE, 0), reps)
    med = statistics.median(t)
    out.append(f"slide_accumulate, 9 windows in one launch  {med:9.1f} [{t[0]:.1f} - {t[-1]:.1f}]  {nw} x {win / 1e6:.1f} MB read + "
               f"{full / 1e6:.1f} MB written = {(nw * win + full) / 1e6:.1f} MB: {(nw * win + full) / med * 1e-6:.2f} TB/s")
    per = []
    for w0 in range(nw):          # in increasing w0, as the protocol asks: every launch sees the stored values it would see in use
        for v in range(w0):
            ops.slide_accumulate(preds, logits[v:v + 1], CROP, STRIDE, v)
        per.append(kernel_us(lambda: ops.slide_accumulate(preds, logits[w0:w0 + 1], CROP, STRIDE, w0), reps))
    meds = [statistics.median(p) for p in per]
    out.append(f"slide_accumulate, one window per launch    {sum(meds):9.1f} summed over the 9 launches (each {min(meds):.1f} .. {max(meds):.1f}); "
               f"a launch reads {win / 1e6:.1f} MB and reads and writes up to {win / 1e6:.1f} MB of preds")
    t = kernel_us(lambda: ops.slide_windows(img, CROP, STRIDE, 0, nw), reps)
    med = statistics.median(t)
    cut = 4 * 3 * eh * ew * nw
    out.append(f"slide_windows, 9 windows in one launch     {med:9.1f} [{t[0]:.1f} - {t[-1]:.1f}]  {cut / 1e6:.1f} MB read + {cut / 1e6:.1f} MB "
               f"written: {2 * cut / med * 1e-6:.2f} TB/s")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--workload", default="C3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slide_inference_ab.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    assert a.iters >= 20, "at least 20 timed iterations per arm"
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg(a.workload))).cuda().eval()
    K = s2f.WORKLOADS[a.workload]["K"]
    img = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(11)).cuda()

    def run(group, route):
        model.test_cfg = dict(mode="slide", crop_size=CROP, stride=STRIDE, **({} if group is None else dict(window_batch=group)))
        s2f.reset_net(model)
        return model.slide_inference(img, [dict(img_shape=(H, W), ori_shape=(H, W))], route=route)

    times, peaks, outs = {n: [] for n, _, _ in ARMS}, {}, {}
    with torch.no_grad():
        for name, group, route in ARMS:
            for _ in range(a.warmup):
                run(group, route)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            outs[name] = run(group, route).clone()
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated() - base
        same = torch.equal(outs["torch"].view(torch.int32), outs["device"].view(torch.int32))
        assert same, "the device route is not the torch loop bit for bit"
        ref = outs["device"]
        diffs = {n: ((outs[n] - ref).abs().max().item(), (outs[n].argmax(1) != ref.argmax(1)).float().mean().item()) for n in outs}
        scale = ref.abs().max().item()
        del outs, ref
        for _ in range(a.iters):
            for name, group, route in ARMS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(group, route)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)

    ny, nx, eh, ew = ops.slide_grid(H, W, CROP, STRIDE)
    full, win = 4 * K * H * W, 4 * K * eh * ew
    med = {n: statistics.median(t) for n, t in times.items()}
    floor = abs(med["torch"] - med["torch_2"])
    lines = [f"`python tools/slide_probe.py` on one MI355X ({torch.cuda.get_device_name(0)}), one process; {a.workload} model, eval, seeded "
             f"input [1, 3, {H}, {W}], crop {CROP}, stride {STRIDE}: {ny} x {nx} windows of {eh} x {ew}, K = {K}; {a.iters} timed "
             f"iterations per arm after {a.warmup} warm ones, arms alternated per iteration; wall clock between device synchronisations, ms",
             f"bytes (computed, not measured): a full map {full / 1e6:.1f} MB, a window's logits {win / 1e6:.1f} MB; the merge reads "
             f"{ny * nx} x {win / 1e6:.1f} MB and writes the map once; the loop's glue moves about 4 x {full / 1e6:.1f} MB x {ny * nx} = "
             f"{4 * full * ny * nx / 1e9:.2f} GB",
             f"device route == torch loop bit for bit: {same}", ""]
    for name, _, _ in ARMS:
        t = sorted(times[name])
        lines.append(f"{name:8s} median {med[name]:8.2f}  min {t[0]:8.2f}  p90 {t[int(0.9 * (len(t) - 1))]:8.2f}  max {t[-1]:8.2f}  "
                     f"peak memory above the model and input {peaks[name] / 1e6:9.1f} MB  "
                     f"max |logit - device| {diffs[name][0]:.3e} (scale {scale:.3e})  arg-max differs on {diffs[name][1]:.2e} of the pixels")
    lines += ["", f"noise floor |torch - torch_2| = {floor:.2f} ms",
              f"device - torch = {med['device'] - med['torch']:+.2f} ms ({'within' if med['device'] - med['torch'] <= floor else 'BEYOND'} "
              f"the noise floor as a slow-down)",
              f"batch3 - device = {med['batch3'] - med['device']:+.2f} ms, batch9 - device = {med['batch9'] - med['device']:+.2f} ms"]
    lines += ["", f"kernels alone (the dispatch packets' own timestamps, s2f_time_next_call; median [min - max] of {a.kernel_reps} "
              f"launches after 5, us), B = 1, K = {K}, random logits:"] + kernel_lines(K, a.kernel_reps)
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
