"""Worker of tests/test_gpu_train_loop.py::test_two_ranks_train_checkpoint_and_resume: one rank of a world-size-2 job whose ranks
SHARE GPU 0 (gloo carries the collectives, as in tests/_dist_worker.py).  TrainLoop at world size > 1: the step holds no optimizer
(two graphs around the host assignment, the route tests/_dist_worker.py runs under gloo), the loop all-reduces the flat gradient
buffer, updates eagerly and appends the log's row behind the update.  Four iterations with a checkpoint every second one, then
both ranks, put somewhere else first, resume from rank 0's file and run two more.  argv[1]: a directory; rank r works in
argv[1]/rank{r}.  Prints `RANK r OK` or raises."""
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
with torch.no_grad():                                        # rank 1 starts from different weights: the broadcast fixes it
    if rank == 1:
        for p in model.parameters():
            p.mul_(1.25)
broadcast_params(model)
s2f.set_keep_membrane(model, False)
red = FlatGradAllReduce(model.parameters(), world)
opt = FlatAdamW(model, red, lr=0.001, weight_decay=0.005, clip_grad=CLIP)
sched = LinearThenPoly(opt, warmup=4, total=20, start_factor=0.1)
aug = TrainAugment(crop_size=crop, scale=(2 * crop[1], crop[0]), ratio_range=(0.5, 2.0), cat_max_ratio=0.75, photometric=True,
                   batch_size=2, max_source_pixels=70 * 90, seed=11, rank=rank, **NORM)
log = s2f.TrainLog(window=8)
example_in, example_seg = (t.to(dev) for t in examples(crop))
step = GraphedHungarianStep(model, example_in, example_seg, red, warmup=1, log=log)
assert step.two_graphs and step.optimizer is None and step.log_captured is False
batches = make_batches(w["K"])[rank:] + make_batches(w["K"])[:rank]          # each rank its own pictures
work = os.path.join(sys.argv[1], f"rank{rank}")
hooks = [dict(type="LoggerHook", interval=2, window_size=2), dict(type="CheckpointHook", interval=2)]


def parameters_agree(what):
    chk = torch.cat([p.detach().flatten() for p in red.params])
    both = [torch.zeros_like(chk) for _ in range(world)]
    dist.all_gather(both, chk)
    assert torch.equal(both[0], both[1]), f"parameters differ between the ranks {what}"
    assert bool(torch.isfinite(chk).all())
    return chk


start = torch.cat([p.detach().flatten() for p in red.params]).clone()
s2f.TrainLoop(step, opt, sched, aug, batches, max_iters=4, hooks=hooks, work_dir=work).run()
after4 = parameters_agree("after four iterations").clone()
assert not torch.equal(after4, start) and float(opt.state[4]) == 4.0 and sched.t == 4
files = sorted(os.listdir(work)) if os.path.isdir(work) else []
if rank == 0:          # rank 0 alone has written
    assert files == ["iter_2.pth", "iter_4.pth", "last_checkpoint", "vis_data"], files
    with open(os.path.join(work, "vis_data", "scalars.json")) as f:
        lines = [json.loads(line) for line in f]
    assert [r["iter"] for r in lines] == [2, 4] and all(np.isfinite(r["loss"]) and r["grad_norm"] > 0 for r in lines)
else:
    assert files == [], files
rng4 = aug.rng.bit_generator.state
dist.barrier()
# somewhere else, then back from rank 0's file -- on both ranks
with torch.no_grad():
    for p in model.parameters():
        p.mul_(1.5 + rank)
opt.exp_avg.fill_(0.5), opt.exp_avg_sq.fill_(0.25), opt.state.fill_(9.0)
sched.t = 11
aug.rng.random(7)
path = os.path.join(sys.argv[1], "rank0", "iter_4.pth")
loop = s2f.TrainLoop(step, opt, sched, aug, batches, max_iters=6, hooks=hooks, work_dir=work + "_resumed", load_from=path, resume=True)
assert len(torch.load(path, weights_only=True)["augment"]) == 2
loop.state.load(path, resume=True)
assert torch.equal(parameters_agree("after loading"), after4) and aug.rng.bit_generator.state == rng4          # each rank ITS generator
loop.run()
after6 = parameters_agree("after the resumed iterations")
assert not torch.equal(after6, after4) and float(opt.state[4]) == 6.0 and sched.t == 6 and loop.log.read().count == 6
print(f"RANK {rank} OK files {files}", flush=True)
dist.barrier()
dist.destroy_process_group()
