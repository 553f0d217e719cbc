"""Worker of tests/test_gpu_grad_accum.py::test_two_ranks_reduce_once_per_group: one rank of a world-size-2 job whose ranks SHARE
GPU 0 (gloo carries the collectives, as in tests/_train_loop_worker.py).  FlatAdamW(accumulative_counts=2) is handed to the step,
which at world size > 1 stops behind `accum.add()`; TrainLoop all-reduces, updates, finishes and appends -- the first three only on
the iterations that close a group.  Four iterations: `red.reduce` ran twice, the optimizer stepped twice, both ranks hold bit-equal
parameters.  argv[1]: a directory; rank r works in argv[1]/rank{r}.  Prints `RANK r OK` or raises."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spike2former_amd as s2f                                               # noqa: E402
from spike2former_amd.augment import TrainAugment                            # noqa: E402
from spike2former_amd.dist import FlatGradAllReduce, broadcast_params, init_process_group      # noqa: E402
from spike2former_amd.graph import GraphedHungarianStep                     # noqa: E402
from spike2former_amd.init_utils import seeded_init                         # noqa: E402
from spike2former_amd.train import FlatAdamW, LinearThenPoly                # noqa: E402
from step_rig import CLIP, NORM, examples, make_batches                     # noqa: E402

rank, world, local = init_process_group()
assert world == 2 and dist.get_backend() == "gloo"
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
w = s2f.WORKLOADS["C1_64"]
crop = (w["H"], w["W"])
model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C1_64"))).to(dev).train()
broadcast_params(model)
s2f.set_keep_membrane(model, False)
red = FlatGradAllReduce(model.parameters(), world)
opt = FlatAdamW(model, red, lr=0.001, weight_decay=0.005, clip_grad=CLIP, accumulative_counts=2)
sched = LinearThenPoly(opt, warmup=4, total=20, start_factor=0.1)
aug = TrainAugment(crop_size=crop, scale=(2 * crop[1], crop[0]), ratio_range=(0.5, 2.0), cat_max_ratio=0.75, photometric=True,
                   batch_size=2, max_source_pixels=70 * 90, seed=11, rank=rank, **NORM)
log = s2f.TrainLog(window=8)
example_in, example_seg = (t.to(dev) for t in examples(crop))
step = GraphedHungarianStep(model, example_in, example_seg, red, warmup=1, optimizer=opt, log=log)
assert step.two_graphs and step.optimizer is opt and step.log_captured is False
batches = make_batches(w["K"])[rank:] + make_batches(w["K"])[:rank]          # each rank its own pictures
work = os.path.join(sys.argv[1], f"rank{rank}")

reduces, reduce = [], red.reduce


def counted(*args, **kw):
    reduces.append(opt.accum.count)          # the iterations done when the all-reduce is issued
    return reduce(*args, **kw)


red.reduce = counted
start = torch.cat([p.detach().flatten() for p in red.params]).clone()
assert float(opt.state[4]) == 0.0          # the warm-up passes and the capture updated nothing
loop = s2f.TrainLoop(step, opt, sched, aug, batches, max_iters=4, hooks=[dict(type="LoggerHook", interval=2, window_size=2)],
                     work_dir=work)
assert loop.eager_update and loop.eager_append
loop.run()
torch.cuda.synchronize()
assert reduces == [2, 4], reduces          # ONE all-reduce per group, behind its last iteration
assert float(opt.state[4]) == 2.0 and sched.t == 4 and opt.accum.count == 4 and log.read().count == 4
chk = torch.cat([p.detach().flatten() for p in red.params])
both = [torch.zeros_like(chk) for _ in range(world)]
dist.all_gather(both, chk)
assert torch.equal(both[0], both[1]), "parameters differ between the ranks"
assert bool(torch.isfinite(chk).all()) and not torch.equal(chk, start)
if rank == 0:
    with open(os.path.join(work, "vis_data", "scalars.json")) as f:
        lines = [json.loads(line) for line in f]
    assert [r["iter"] for r in lines] == [2, 4] and all(r["grad/accum"] == 2 and np.isfinite(r["loss"]) and r["grad_norm"] > 0 for r in lines)
print(f"RANK {rank} OK reduces {reduces}", flush=True)
dist.barrier()
dist.destroy_process_group()
