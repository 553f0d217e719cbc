"""Per-layer MACs, synaptic operations and the energy estimate of one workload (spike2former_amd/energy.py: OpCensus) on one MI355X:
build a workload of WORKLOADS with name-seeded weights or a checkpoint, run N synthetic or given pictures through `test_step` under a
census, print the table -- one line per synaptic op, the totals line with params, MACs, real MACs, SOPs and mJ.

    python tools/energy_report.py [C2] [--images 2] [--checkpoint state.pth] [--inputs pictures.pt] [--amplitude 1.0]
                                  [--e-mac 4.6e-12] [--e-ac 0.9e-12] [--csv out.csv] [--json out.json] [--by-stage]

--inputs: a torch file holding one float tensor [N, 3, H, W] (already normalised); without it seeded standard-normal pictures times
--amplitude.  --checkpoint: a state_dict (or a dict with one under 'state_dict'), loaded strictly.  Seeded weights say what the
network COSTS per spike, not how often a trained one fires: the rates of a report without a checkpoint are those of random weights."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spike2former_amd as s2f                                     # noqa: E402
from spike2former_amd.init_utils import seeded_init                # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("workload", nargs="?", default="C2", choices=sorted(s2f.WORKLOADS))
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--checkpoint")
    ap.add_argument("--inputs")
    ap.add_argument("--amplitude", type=float, default=1.0)
    ap.add_argument("--e-mac", type=float, default=s2f.energy.E_MAC)
    ap.add_argument("--e-ac", type=float, default=s2f.energy.E_AC)
    ap.add_argument("--csv")
    ap.add_argument("--json")
    ap.add_argument("--by-stage", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("energy_report: needs the MI355X (the model's kernels have no host path)")
    w = s2f.WORKLOADS[args.workload]
    model = s2f.MODELS.build(s2f.model_cfg(args.workload))
    if args.checkpoint:
        state = torch.load(args.checkpoint, map_location="cpu")
        model.load_state_dict(state.get("state_dict", state), strict=True)
    else:
        seeded_init(model)
    model.cuda().eval()
    if args.inputs:
        pictures = torch.load(args.inputs, map_location="cpu").float()
    else:
        g = torch.Generator().manual_seed(0)
        pictures = args.amplitude * torch.randn(args.images, 3, w["H"], w["W"], generator=g)
    with s2f.OpCensus(model, max_passes=len(pictures)) as census:
        for img in pictures:
            s2f.reset_net(model)
            model.test_step(dict(inputs=[img]))
        rep = census.report(e_mac=args.e_mac, e_ac=args.e_ac)
    print(f"{args.workload}: {len(pictures)} pictures of {tuple(pictures.shape[1:])}, "
          f"{'checkpoint ' + args.checkpoint if args.checkpoint else 'name-seeded weights'}")
    print(rep)
    if args.by_stage:
        print()
        for stage, s in rep.by_stage().items():
            print(f"{stage:<44} rows {s['rows']:>4}  MACs {s['macs'] / 1e9:>9.4f} G  real {s['real_macs'] / 1e9:>9.4f} G  "
                  f"SOPs {s['sops'] / 1e9:>9.4f} G  {1e3 * s['energy_J']:>9.4f} mJ")
    bad = rep.spikes_off_grid()
    if bad:
        print(f"\nWARNING: {len(bad)} ops were handed a spike map with elements off the 1 / {rep.D} grid: " + ", ".join(r["key"] for r in bad[:5]))
    if args.csv:
        rep.to_csv(args.csv)
    if args.json:
        with open(args.json, "w") as f:
            f.write(rep.to_json())


if __name__ == "__main__":
    main()
