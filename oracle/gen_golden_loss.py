"""TEST INFRASTRUCTURE -- golden vectors for the Hungarian-matched MaskFormer loss.

Runs the REFERENCE's own loss path on CPU (mmdet MaskFormerHead.loss_by_feat with HungarianAssigner / MaskPseudoSampler /
CrossEntropyLoss / FocalLoss / DiceLoss and mmseg's _seg_data_to_instance_data, imported through oracle/ref_loss_shells.py)
on seeded inputs and stores inputs + outputs in tests/golden/loss_f1.npz (`cases`) and tests/golden/loss_f1_edges.npz
(`cases_edges`: maps that leave one tile / one chunk of the loss kernels).  Usable only where /root/reference is mounted:

    python -m oracle.gen_golden_loss [f1 | edges]         (default: both files)
"""
import os

import numpy as np
import torch

from . import ref_loss_shells as rl

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
OUT = os.path.join(GOLDEN, "loss_f1.npz")
OUT_EDGES = os.path.join(GOLDEN, "loss_f1_edges.npz")


def cases():
    """name -> (cls [L,B,Q,K+1], mask_preds [L,B,Q,h,w], gt_sem_seg [B,1,H,W], K)"""
    out = {}
    g = torch.Generator().manual_seed(11)
    K, Q = 5, 10                                           # fewer classes than queries
    seg = torch.randint(0, K, (2, 1, 32, 32), generator=g)
    seg[0, :, :8] = 255                                    # an ignored band
    out["a"] = (torch.randn(3, 2, Q, K + 1, generator=g), torch.randn(3, 2, Q, 16, 16, generator=g) * 2, seg, K)
    K, Q = 20, 6                                           # more ground-truth masks than queries (rectangular assignment)
    seg = torch.randint(0, K, (2, 1, 24, 40), generator=g)
    out["b"] = (torch.randn(2, 2, Q, K + 1, generator=g), torch.randn(2, 2, Q, 12, 20, generator=g) * 3, seg, K)
    K, Q = 4, 5                                            # one image without ground truth
    seg = torch.randint(0, K, (2, 1, 16, 16), generator=g)
    seg[1] = 255
    out["c"] = (torch.randn(2, 2, Q, K + 1, generator=g), torch.randn(2, 2, Q, 8, 8, generator=g), seg, K)
    seg = torch.full((1, 1, 16, 16), 255)                  # no ground truth at all (zero-match branch)
    out["d"] = (torch.randn(2, 1, Q, K + 1, generator=g), torch.randn(2, 1, Q, 8, 8, generator=g), seg, K)
    return out


def _region_seg(B, H, W, K, g):
    """[B, 1, H, W] piecewise-constant label maps: a 3 x 4 grid of blocks with unequal borders, a random class each, and a band of
    the ignored label that cuts through the blocks"""
    seg = torch.empty(B, 1, H, W, dtype=torch.int64)
    ys, xs = [0, H // 3 + 1, (2 * H) // 3 - 1, H], [0, W // 4 + 3, W // 2 + 1, (3 * W) // 4 - 2, W]
    for b in range(B):
        pick = torch.randint(0, K, (12,), generator=g)
        for i in range(3):
            for j in range(4):
                seg[b, 0, ys[i]:ys[i + 1], xs[j]:xs[j + 1]] = pick[i * 4 + j]
        seg[b, 0, H // 2 - 1:H // 2 + 2, W // 5:(4 * W) // 5 + b] = 255
    return seg


def cases_edges():
    """Maps past one 8 x 64 tile of the label-map backward kernel, region label maps with a band of 255.  Logits within +/-12: the
    reference's float32 costs and the fp64-following cost kernel agree on the assignment there (see costs_all_classes)."""
    out = {}
    g = torch.Generator().manual_seed(23)
    K, Q = 6, 8                                            # 9 x 66: one row and two columns into the next tiles
    seg = _region_seg(2, 18, 132, K, g)
    out["e"] = (torch.randn(2, 2, Q, K + 1, generator=g), (torch.randn(2, 2, Q, 9, 66, generator=g) * 3).clamp(-12, 12), seg, K)
    K, Q = 12, 5                                           # 17 x 130: three tiles each way with remainders; more classes than queries
    seg = _region_seg(2, 34, 260, K, g)
    out["f"] = (torch.randn(2, 2, Q, K + 1, generator=g), (torch.randn(2, 2, Q, 17, 130, generator=g) * 3).clamp(-12, 12), seg, K)
    return out


def write(case_set, path):
    L = rl.load()
    blob = {}
    for name, (cls, mp, seg, K) in case_set.items():
        Q = cls.shape[2]
        head = rl.reference_loss_head(K, Q)
        cls, mp = cls.clone().requires_grad_(True), mp.clone().requires_grad_(True)
        samples = [rl.SegSample(seg[i], *seg.shape[-2:]) for i in range(seg.shape[0])]
        fake = type("F", (), {"ignore_index": 255})()
        inst, metas = L.seg_head.MaskFormerHead._seg_data_to_instance_data(fake, samples)
        losses = head.loss_by_feat(cls, mp, inst, metas)
        sum(losses.values()).backward()
        # cross-check with this repository's restatement before writing anything
        from spike2former_amd.loss import MaskFormerLoss, seg_to_instances
        c2, m2 = cls.detach().clone().requires_grad_(True), mp.detach().clone().requires_grad_(True)
        mine = MaskFormerLoss(K, Q).loss_by_feat(c2, m2, [seg_to_instances(seg[i]) for i in range(seg.shape[0])])
        sum(mine.values()).backward()
        assert list(mine) == list(losses)
        for k in losses:
            assert abs(float(mine[k]) - float(losses[k])) <= 1e-5 * max(1.0, abs(float(losses[k]))), (name, k)
        assert torch.allclose(c2.grad, cls.grad, atol=1e-6) and torch.allclose(m2.grad, mp.grad, atol=1e-7)
        blob[f"{name}_cls"], blob[f"{name}_masks"], blob[f"{name}_seg"] = cls.detach().numpy(), mp.detach().numpy(), seg.numpy()
        blob[f"{name}_K"] = np.int64(K)
        blob[f"{name}_keys"] = np.array(list(losses.keys()))
        blob[f"{name}_losses"] = np.array([float(v) for v in losses.values()], np.float64)
        blob[f"{name}_gcls"], blob[f"{name}_gmasks"] = cls.grad.numpy(), mp.grad.numpy()
        blob[f"{name}_labels"] = np.concatenate([i.labels.numpy() for i in inst]) if inst else np.zeros(0, np.int64)
        print(name, {k: round(float(v), 5) for k, v in losses.items()})
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path), "bytes")


def main(which=("f1", "edges")):
    if "f1" in which:
        write(cases(), OUT)
    if "edges" in which:
        write(cases_edges(), OUT_EDGES)


if __name__ == "__main__":
    import sys
    main(tuple(sys.argv[1:]) or ("f1", "edges"))
