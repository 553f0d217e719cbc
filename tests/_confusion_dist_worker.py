"""Worker of tests/test_confusion.py: one rank of a world-size-2 gloo job on CPU.  Each rank scores its share of the hand-counted
images through spike2former_amd.evaluate(..., rank, world_size); the int64 matrices are all-reduced inside
ConfusionMatrix.evaluate, so both ranks must end with the matrix of the WHOLE set."""
import os


def worker(rank, world, port, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    import spike2former_amd as s2f
    from spike2former_amd.dist import init_process_group
    from test_confusion import NAMES, HandModel, hand_batches
    r, w, _ = init_process_group("gloo")
    metric = s2f.METRICS.build(dict(type="ConfusionMatrix"))
    metric.dataset_meta = dict(classes=NAMES)
    batches = hand_batches()
    assert 0 < len(batches[r::w]) < len(batches)          # disjoint, non-empty shares (3 images: 2 + 1)
    own = s2f.ConfusionMatrix()                            # this rank's share alone, never all-reduced: evaluated before the group's
    own.dataset_meta = dict(classes=NAMES)
    for b in hand_batches()[r::w]:
        own.process(b, b["data_samples"])
    own_matrix = own._acc.tolist()
    summary = s2f.evaluate(HandModel(), batches, metric, rank=r, world_size=w)
    out[rank] = dict(matrix=metric.matrix.tolist(), summary=dict(summary), own=own_matrix)
    dist.barrier()
    dist.destroy_process_group()
