"""Eager eval-mode predict of a workload's model at an arbitrary image size: which C-ABI entry points (kernel families) ran, how
often, and which ops.fallback sites were taken -- the odd-size audit of the predict path (docs/EXPERIMENTS.md).
    python tools/any_size_census.py [workload H W [B]] > any_size_census.txt
Runs with ops.STRICT off so that every site that leaves the package's kernels is listed instead of raising at the first one;
`--strict` runs under STRICT (exit status 1 on the first fall-back).  Also prints the eager predict time (ms, median of 5)."""
import collections
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import spike2former_amd as s2f
from spike2former_amd import _lib, ops
from spike2former_amd._lib import lib
from spike2former_amd.init_utils import seeded_init

args = [a for a in sys.argv[1:] if not a.startswith("--")]
workload = args[0] if args else "C2"
H, W = (int(args[1]), int(args[2])) if len(args) >= 3 else (512, 683)
B = int(args[3]) if len(args) >= 4 else 1
ops.STRICT = "--strict" in sys.argv
calls = collections.Counter()
ON = [False]


def wrap(name):
    orig = getattr(lib, name)

    def w(*a):
        if ON[0]:
            calls[name] += 1
        return orig(*a)
    setattr(lib, name, w)


for name, (res, argt) in _lib.SIGNATURES.items():
    if len(argt) >= 3 and name not in ("s2f_time_next_call", "s2f_event_elapsed_us"):
        wrap(name)

dev = torch.device("cuda", 0)
model = seeded_init(s2f.MODELS.build(s2f.model_cfg(workload))).to(dev).eval()
s2f.set_keep_membrane(model, False)
img = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(1000)).to(dev)


def step():
    s2f.reset_net(model)
    with torch.no_grad():
        return model(img, mode="predict")


import warnings
warnings.simplefilter("ignore", RuntimeWarning)          # (the sites are counted in ops.FALLBACKS)
step()
torch.cuda.synchronize()
before = dict(ops.FALLBACKS)
ON[0] = True
out = step()
torch.cuda.synchronize()
ON[0] = False
ts = []
for _ in range(5):
    t0 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) * 1e3)
fb = {k: v - before.get(k, 0) for k, v in ops.FALLBACKS.items() if v != before.get(k, 0)}
print(f"# {workload} eval predict at B={B} {H}x{W}: {sum(calls.values())} C-ABI calls in {len(calls)} entry points; "
      f"eager predict {sorted(ts)[2]:.2f} ms (median of 5)")
print(f"# pred_sem_seg {tuple(out[0].pred_sem_seg.data.shape)} {out[0].pred_sem_seg.data.dtype}; "
      f"seg_logits {tuple(out[0].seg_logits.data.shape)}")
print(f"# fall-backs taken per predict: {fb if fb else 'none'}")
for name, n in sorted(calls.items(), key=lambda kv: (-kv[1], kv[0])):
    print(f"{n:5d}x  {name}")
