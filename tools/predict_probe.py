"""Measurement of captured inference (graph.GraphedPredict behind test_cfg['graph']) and of the fused label kernel (s2f_seg_label) on
one MI355X.  Per workload three arms alternate iteration by iteration in ONE process (a drift of the clocks hits all of them alike):

  eager      test_cfg without `graph`: every launch issued from Python, as before the option existed
  graph      test_cfg['graph'] = dict(capture_after=1): the pass is a hipGraph replay per key (captured during the warm iterations)
  eager_2    the eager arm a second time: the gap between the two medians is the noise floor of this run

An iteration is reset_net + EncoderDecoder.inference between two device synchronisations, wall clock.  Workloads:

  whole B=1, B=2   the C2 model, eval, whole-image inference on a seeded [B, 3, 512, 512] input
  slide            the C3 model, eval, on the seeded [1, 3, 1024, 2048] picture of tools/slide_probe.py: crop (512, 1024), stride
                   (341, 683), window_batch = 3 -- three groups of three windows, one key

Before anything is timed the graph arm is compared bit for bit with the eager arm.  Per captured key the capture time (warm-up passes
included) and the growth of torch.cuda.memory_reserved are listed: what `max_graphs` and `capture_after` are sized by.  Then the tail
of postprocess_result on its own at K = 150, 512 x 683 -> 512 x 683 and -> 256 x 341: s2f_resize_fwd + s2f_seg_argmax against
s2f_seg_label, from the dispatch packets' timestamps (s2f_time_next_call).  Writes the table to --out.

    python tools/predict_probe.py [--iters 20] [--warmup 3] [--kernel-reps 50] [--out profiles/graphed_predict_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import spike2former_amd as s2f                                     # noqa: E402
from spike2former_amd import ops                                   # noqa: E402
from spike2former_amd.init_utils import seeded_init                # noqa: E402
from slide_probe import CROP, STRIDE, kernel_us                    # noqa: E402

ARMS = ("eager", "graph", "eager_2")
SLIDE = dict(mode="slide", crop_size=CROP, stride=STRIDE, window_batch=3)


def measure(model, img, base_cfg, iters, warmup):
    """-> (times per arm, bit equality of the graph arm with the eager arm, the graph arm's GraphedPredict)"""
    H, W = img.shape[-2:]
    cfgs = {"eager": dict(base_cfg), "graph": dict(base_cfg, graph=dict(capture_after=1)), "eager_2": dict(base_cfg)}

    def run(arm):
        model.test_cfg = cfgs[arm]
        s2f.reset_net(model)
        return model.inference(img, [dict(img_shape=(H, W), ori_shape=(H, W)) for _ in range(img.shape[0])])

    model.__dict__.pop("_graphed_predict", None)
    times, outs = {a: [] for a in ARMS}, {}
    with torch.no_grad():
        for arm in ARMS:
            for _ in range(max(warmup, 2)):          # (the graph arm captures in its first warm iteration)
                outs[arm] = run(arm)
            outs[arm] = outs[arm].clone()
        torch.cuda.synchronize()
        same = torch.equal(outs["eager"].view(torch.int32), outs["graph"].view(torch.int32))
        del outs
        for _ in range(iters):
            for arm in ARMS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(arm)
                torch.cuda.synchronize()
                times[arm].append((time.perf_counter() - t0) * 1e3)
    gp = model.__dict__.pop("_graphed_predict")
    model.test_cfg = dict(base_cfg)
    return times, same, gp


def report(title, times, same, gp):
    med = {a: statistics.median(t) for a, t in times.items()}
    floor = abs(med["eager"] - med["eager_2"])
    gain = med["eager"] - med["graph"]
    lines = [title, f"  graph arm == eager arm bit for bit: {same}"]
    for a in ARMS:
        t = sorted(times[a])
        lines.append(f"  {a:8s} median {med[a]:8.2f} [{t[0]:.2f} - {t[-1]:.2f}] ms")
    lines.append(f"  noise floor |eager - eager_2| = {floor:.2f} ms; eager / graph = {med['eager'] / med['graph']:.2f} "
                 f"(eager - graph = {gain:+.2f} ms: " + ("the graph arm is faster" if gain > floor else
                                                         "within the noise floor" if gain >= -floor else "the graph arm is SLOWER") + ")")
    c = gp.census
    lines.append(f"  census of the graph arm: {c['captures']} captures, {c['replays']} replays, {c['evictions']} evictions, eager {c['eager']}")
    for e in gp.capture_log:
        lines.append(f"  captured key input {list(e['key'][0])}, img_shape {e['key'][1]}: {e['seconds'] * 1e3:8.1f} ms to capture (warm-up "
                     f"passes included), torch.cuda.memory_reserved grew by {e['reserved_bytes'] / 1e6:8.1f} MB")
    return lines + [""]


def tail_lines(K, reps):
    """the tail of postprocess_result at K classes on a 512 x 683 map: two launches against one"""
    x = torch.randn(K, 512, 683, generator=torch.Generator().manual_seed(3)).cuda()
    out = []
    for size in ((512, 683), (256, 341)):
        planes = ops.resize_window(x, size)
        assert torch.equal(ops.seg_argmax(planes), ops.seg_label(x, size)), "s2f_seg_label is not the two-pass route"
        a = kernel_us(lambda: ops.resize_window(x, size), reps)
        b = kernel_us(lambda: ops.seg_argmax(planes), reps)
        f = kernel_us(lambda: ops.seg_label(x, size), reps)
        two = statistics.median(a) + statistics.median(b)
        a2 = kernel_us(lambda: ops.resize_window(x, size), reps)          # the first arm again: the noise floor
        b2 = kernel_us(lambda: ops.seg_argmax(planes), reps)
        two2 = statistics.median(a2) + statistics.median(b2)
        fused, floor = statistics.median(f), abs(two - two2)
        full = 4 * K * size[0] * size[1]
        out.append(f"  512 x 683 -> {size[0]} x {size[1]}: s2f_resize_fwd {statistics.median(a):8.1f} [{a[0]:.1f} - {a[-1]:.1f}] + s2f_seg_argmax "
                   f"{statistics.median(b):8.1f} [{b[0]:.1f} - {b[-1]:.1f}] = {two:8.1f} us (again: {two2:.1f}, floor {floor:.1f}); s2f_seg_label "
                   f"{fused:8.1f} [{f[0]:.1f} - {f[-1]:.1f}] us: two-pass / fused = {two / fused:.2f} "
                   f"({'faster' if two - fused > floor else 'within the noise floor' if two - fused >= -floor else 'SLOWER'}); the planes "
                   f"between the two launches are {full / 1e6:.1f} MB written and read once, and as large a temporary")
        del planes
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graphed_predict_ab.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    assert a.iters >= 20, "at least 20 timed iterations per arm"
    lines = [f"`python tools/predict_probe.py` on one MI355X ({torch.cuda.get_device_name(0)}), one process; models seeded, eval, "
             f"no_grad; {a.iters} timed iterations per arm after {max(a.warmup, 2)} warm ones, arms alternated per iteration; median "
             f"[min - max] of the wall clock between device synchronisations", ""]
    w = s2f.WORKLOADS["C2"]
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C2"))).cuda().eval()
    for B in (1, 2):
        img = torch.randn(B, 3, w["H"], w["W"], generator=torch.Generator().manual_seed(1000 + B)).cuda()
        lines += report(f"whole-image inference, C2, input [{B}, 3, {w['H']}, {w['W']}], K = {w['K']}:",
                        *measure(model, img, dict(mode="whole"), a.iters, a.warmup))
    del model
    torch.cuda.empty_cache()
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C3"))).cuda().eval()
    img = torch.randn(1, 3, 1024, 2048, generator=torch.Generator().manual_seed(11)).cuda()
    lines += report(f"slide inference, C3, input [1, 3, 1024, 2048], crop {CROP}, stride {STRIDE}, window_batch 3 (3 replays per picture), "
                    f"K = {s2f.WORKLOADS['C3']['K']}:", *measure(model, img, SLIDE, a.iters, a.warmup))
    del model
    torch.cuda.empty_cache()
    lines += [f"the tail of postprocess_result alone, K = 150 (the dispatch packets' own timestamps, s2f_time_next_call; median [min - max] "
              f"of {a.kernel_reps} launches after 5, us), random logits:"] + tail_lines(150, a.kernel_reps)
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
