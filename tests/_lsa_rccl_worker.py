"""Worker of tests/test_gpu_lsa_step.py::test_two_graph_form_under_a_process_group_is_the_single_graph: the real training step with
the assignment on the device in ONE process -- with S2F_FORCE_DIST=1 under a live RCCL communicator (backend nccl, world 1: the
step is graph A | graph B), without it under no process group (one graph).  Writes [(loss dictionary, flat gradients)] of three
replays to argv[1]."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spike2former_amd as s2f                                               # noqa: E402
from spike2former_amd.dist import FlatGradAllReduce, broadcast_params, init_process_group      # noqa: E402
from spike2former_amd.graph import GraphedHungarianStep                     # noqa: E402
from spike2former_amd.init_utils import seeded_init                         # noqa: E402
from test_gpu_lsa_step import N_CLASSES, region_maps                  # noqa: E402

rank, world, local = init_process_group()
backend = dist.get_backend() if dist.is_initialized() else "none"
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
w = s2f.WORKLOADS["C1_64"]
model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C1_64"))).to(dev).train()
broadcast_params(model)
s2f.set_keep_membrane(model, False)
red = FlatGradAllReduce(model.parameters(), world)
imgs = [torch.randn(2, 3, w["H"], w["W"], generator=torch.Generator().manual_seed(5 + i)).to(dev) for i in range(3)]
segs = [region_maps(2, w["H"], w["W"], w["K"], N_CLASSES[i], 6 + i).to(dev) for i in range(3)]
state = {k: v.clone() for k, v in model.state_dict().items()}

step = GraphedHungarianStep(model, imgs[0], segs[0], red, warmup=1, assign="device")
steps = []
for i in (0, 1, 2, 0):
    model.load_state_dict(state)
    got = step(imgs[i], segs[i])
    step.check()
    torch.cuda.synchronize()
    steps.append(({k: float(v) for k, v in got.items()}, red.flat.detach().cpu().clone()))
torch.save({"steps": steps}, sys.argv[1])
print(f"backend {backend} two_graphs {step.two_graphs} loss {sum(steps[-1][0].values()):.9e}", flush=True)
if dist.is_initialized():
    dist.destroy_process_group()
