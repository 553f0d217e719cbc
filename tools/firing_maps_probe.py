"""Measurement of the firing maps on one MI355X (prints its lines; --out also writes them to a file.  profiles/firing_maps_ab.txt holds
a run of it: records, not gates):

  kernel   s2f_firing_map on the largest and on the smallest neuron map of the C2 model (the shapes are taken from one pass under
           FiringMaps, batch 1) beside a device-to-device copy of the same bytes in the same process, rounds of the two alternating:
           device events around `--reps` back-to-back calls, and the dispatch packet's own timestamps (s2f_time_next_call).
           Achieved GB/s = bytes of the neuron output / time (the planes written, 16 bytes per pixel, are not counted).
  draw     one s2f_firing_draw of a 128 x 128 plane over a 512 x 512 picture, the same two ways.
  pass     one eval pass of the C2 model (reset_net + model(img, mode='logits'), batch 1, wall clock between two device
           synchronisations) plain and under a live FiringMaps of every neuron, alternating in one process; the launches of the
           live arm; one read().

    python tools/firing_maps_probe.py [--reps 50] [--rounds 7] [--passes 7] [--out FILE]
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
from op_census_probe import events_us                              # noqa: E402


def med(v):
    return f"{statistics.median(v):8.2f} [{min(v):.2f} - {max(v):.2f}]"


def map_lines(shapes, reps, rounds):
    out = []
    for what, name, (T, B, C, h, w) in shapes:
        x = (torch.randint(0, 9, (T * B, C, h, w), device="cuda").float() / 8)
        x[torch.rand_like(x) < 0.7] = 0
        dst = torch.empty_like(x)
        stats = torch.empty(B, 4, h, w, dtype=torch.int32, device="cuda")
        nbytes = x.numel() * x.element_size()
        fmap = lambda: ops.firing_map(x, B, 8, stats, assign=True)          # noqa: E731
        copy = lambda: dst.copy_(x)                                         # noqa: E731
        for fn in (fmap, copy):
            events_us(fn, 5)
        t_map, t_copy = [], []
        for _ in range(rounds):
            t_map.append(events_us(fmap, reps))
            t_copy.append(events_us(copy, reps))
        packet = statistics.median(kernel_us(fmap, reps))
        mm = statistics.median(t_map)
        out.append(f"  {what}: {name}  [T B, C, h, w] = [{T * B}, {C}, {h}, {w}] fp32, {nbytes / 2 ** 20:.2f} MiB")
        out.append(f"    s2f_firing_map        {med(t_map)} us/call   {nbytes / mm / 1e3:7.1f} GB/s read   (dispatch packet: {packet:.2f} us, "
                   f"{nbytes / packet / 1e3:.1f} GB/s)")
        out.append(f"    device-to-device copy {med(t_copy)} us/call   {nbytes / statistics.median(t_copy) / 1e3:7.1f} GB/s read + as much written")
    return out


def draw_lines(reps, rounds):
    H = W = 512
    img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda")
    plane = torch.randint(0, 1000, (128, 128), dtype=torch.int32, device="cuda")
    lut = torch.from_numpy(s2f.SegLocalVisualizer.default_firing_lut()).cuda()
    out_t = torch.empty(H, W, 3, dtype=torch.uint8, device="cuda")
    draw = lambda: ops.firing_draw(img, plane, 999, lut, 0.5, out=out_t)          # noqa: E731
    events_us(draw, 5)
    t = [events_us(draw, reps) for _ in range(rounds)]
    packet = statistics.median(kernel_us(draw, reps))
    nbytes = 2 * 3 * H * W
    return [f"  128 x 128 plane over a 512 x 512 picture ({nbytes / 2 ** 20:.2f} MiB of picture read + written)",
            f"    s2f_firing_draw       {med(t)} us/call   {nbytes / statistics.median(t) / 1e3:7.1f} GB/s   (dispatch packet: {packet:.2f} us)"]


def pass_lines(model, img, passes):
    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s2f.reset_net(model)
        model(img, mode="logits")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    plain, live = [], []
    maps = s2f.FiringMaps(model)
    with torch.no_grad():
        for _ in range(3):
            run()
        for _ in range(passes):
            plain.append(run())
            with maps:
                maps.clear()
                live.append(run())
                read = maps.read()
    launches = sum(read.meta[n][3] for n in read.names)
    mp, ml = statistics.median(plain), statistics.median(live)
    return [f"  C2 ({img.shape[2]} x {img.shape[3]}, T = {maps.T}), batch 1, eval, name-seeded weights, {passes} passes each, alternating",
            f"    plain eval pass          {med(plain)} ms",
            f"    pass under FiringMaps    {med(live)} ms   ({ml / mp:.2f} x; {len(maps.nodes)} neurons hooked, {len(read.names)} maps, "
            f"{len(maps.skipped)} skipped, {launches} s2f_firing_map launches, the hooked routes)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the lines to this file (nothing is written by default)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "firing_maps_probe needs the MI355X"
    w = s2f.WORKLOADS["C2"]
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C2"))).cuda().eval()
    img = torch.randn(1, 3, w["H"], w["W"], generator=torch.Generator().manual_seed(0)).cuda()
    with torch.no_grad(), s2f.FiringMaps(model) as maps:
        s2f.reset_net(model)
        model(img, mode="logits")
        sizes = {n: (maps.T, 1) + maps._geometry[n][:3] for n in maps.passes}
    elems = lambda n: sizes[n][0] * sizes[n][2] * sizes[n][3] * sizes[n][4]          # noqa: E731
    largest, smallest = max(sizes, key=elems), min(sizes, key=elems)
    lines = [f"python tools/firing_maps_probe.py --reps {args.reps} --rounds {args.rounds} --passes {args.passes}",
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}", "", "kernel (median of the rounds [min - max])"]
    lines += map_lines([("largest map of C2", largest, sizes[largest]), ("smallest map of C2", smallest, sizes[smallest])], args.reps,
                       args.rounds)
    lines += ["", "drawing (median of the rounds [min - max])"] + draw_lines(args.reps, args.rounds)
    lines += ["", "a pass under FiringMaps against a plain eval pass (median [min - max])"] + pass_lines(model, img, args.passes)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
