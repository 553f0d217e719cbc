"""Measurement of the operand census on one MI355X (prints its lines; --out also writes them to a file.  profiles/op_census.txt
holds a run of it beside hand-written sections: do not point --out at it):

  kernel   s2f_operand_census on 2^25 fp32 and on 2^25 bf16 elements beside a device-to-device copy of the same bytes in the same
           process -- the copy is the yardstick: it reads AND writes the bytes, the census only reads them.  Both are timed the same
           way, device events around `--reps` back-to-back calls, rounds of the two alternating; the census also from its dispatch
           packet's own timestamps (s2f_time_next_call).  Achieved GB/s = bytes read / time.
  pass     one eval pass of the C2 model (reset_net + model(img, mode='logits'), batch 1, wall clock between two device
           synchronisations) plain and under a live OpCensus, alternating; the census arm's launches and table rows.

    python tools/op_census_probe.py [--reps 50] [--rounds 7] [--passes 7] [--out FILE]
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
from slide_probe import kernel_us                                  # noqa: E402

N = 1 << 25


def events_us(fn, reps):
    """microseconds per call of `reps` back-to-back calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def kernel_lines(reps, rounds):
    out = []
    for dtype, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        x = (torch.randint(0, 9, (N,), device="cuda").float() / 8).to(dtype)
        dst = torch.empty_like(x)
        row = torch.zeros(8, dtype=torch.int64, device="cuda")
        nbytes = x.numel() * x.element_size()
        census = lambda: ops.operand_census(x, row, 8)          # noqa: E731
        copy = lambda: dst.copy_(x)                               # noqa: E731
        for fn in (census, copy):
            events_us(fn, 5)
        t_census, t_copy = [], []
        for _ in range(rounds):
            t_census.append(events_us(census, reps))
            t_copy.append(events_us(copy, reps))
        packet = statistics.median(kernel_us(census, reps))
        mc, mp = statistics.median(t_census), statistics.median(t_copy)
        out.append(f"  {name}  2^25 elements, {nbytes >> 20} MiB")
        out.append(f"    s2f_operand_census   {mc:8.2f} us/call [{min(t_census):.2f} - {max(t_census):.2f}]   {nbytes / mc / 1e3:7.1f} GB/s read"
                   f"   (dispatch packet: {packet:.2f} us, {nbytes / packet / 1e3:.1f} GB/s)")
        out.append(f"    device-to-device copy {mp:8.2f} us/call [{min(t_copy):.2f} - {max(t_copy):.2f}]   {nbytes / mp / 1e3:7.1f} GB/s read + as much written")
        out.append(f"    census / copy        {mc / mp:8.3f}")
    return out


def pass_lines(passes):
    w = s2f.WORKLOADS["C2"]
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C2"))).cuda().eval()
    img = torch.randn(1, 3, w["H"], w["W"], generator=torch.Generator().manual_seed(0)).cuda()

    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s2f.reset_net(model)
        model(img, mode="logits")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    plain, census_ms, rep = [], [], None
    with torch.no_grad():
        for _ in range(3):
            run()
        for _ in range(passes):
            plain.append(run())
            with s2f.OpCensus(model) as census:
                census_ms.append(run())
                rep = census.report()
    launches = sum(sum(1 for _ in r["operands"]) * r["calls"] for r in rep.rows)
    mp, mc = statistics.median(plain), statistics.median(census_ms)
    return [f"  C2 (512 x 512, T = 4), batch 1, eval, name-seeded weights, {passes} passes each, alternating",
            f"    plain eval pass      {mp:8.2f} ms [{min(plain):.2f} - {max(plain):.2f}]",
            f"    pass under a census  {mc:8.2f} ms [{min(census_ms):.2f} - {max(census_ms):.2f}]   ({mc / mp:.2f} x; {len(rep.rows)} rows, "
            f"{launches} s2f_operand_census launches, unfused routes, one table read-back)",
            "    " + rep.totals_line()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the lines to this file (nothing is written by default)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "op_census_probe needs the MI355X"
    lines = [f"python tools/op_census_probe.py --reps {args.reps} --rounds {args.rounds} --passes {args.passes}",
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}", "", "kernel (median of the rounds [min - max])"]
    lines += kernel_lines(args.reps, args.rounds)
    lines += ["", "census pass against a plain eval pass (median [min - max])"]
    lines += pass_lines(args.passes)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
