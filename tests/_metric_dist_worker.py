"""Worker of tests/test_metric.py: one rank of a world-size-2 gloo job on CPU.  Each rank scores its share of the recorded K = 150
cases through spike2former_amd.evaluate(..., rank, world_size); the int64 totals are all-reduced inside IoUMetric.evaluate, so both
ranks must return the summary of the WHOLE set."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def batches_of(g, seq):
    """the recorded cases of a sequence as single-image batches of mmengine-style dict samples; the model below hands the
    recorded prediction back as its output"""
    out = []
    for n in (str(n) for n in g[f"{seq}.cases"]):
        pred = torch.from_numpy(g[f"{n}.pred"]).to(torch.float32 if bool(g[f"{n}.float_pred"]) else torch.int64)
        out.append(dict(inputs=[torch.zeros(3, 4, 4)],
                        data_samples=[dict(recorded_pred=pred[None], gt_sem_seg=dict(data=torch.from_numpy(g[f"{n}.label"])[None]))]))
    return out


class RecordedModel(torch.nn.Module):
    def test_step(self, batch):
        for d in batch["data_samples"]:
            d["pred_sem_seg"] = dict(data=d.pop("recorded_pred"))
        return batch["data_samples"]


def worker(rank, world, port, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    import spike2former_amd as s2f
    from spike2former_amd.dist import init_process_group
    r, w, _ = init_process_group("gloo")
    g = np.load(os.path.join(ROOT, "tests", "golden", "metric_iou.npz"), allow_pickle=False)
    metric = s2f.METRICS.build(dict(type="IoUMetric", iou_metrics=["mIoU", "mDice", "mFscore"], beta=2))
    metric.dataset_meta = dict(classes=[str(i) for i in range(150)])
    batches = batches_of(g, "k150")
    got = s2f.evaluate(RecordedModel(), batches, metric, rank=r, world_size=w)
    mine = len(batches[r::w])
    assert 0 < mine < len(batches)                       # disjoint, non-empty shares (5 cases: 3 + 2, no padding)
    out[rank] = dict(got)
    dist.barrier()
    dist.destroy_process_group()
