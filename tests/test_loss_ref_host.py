"""tests/loss_ref.py, the fp64 reference the GPU tests of the loss kernels compare with (tests/test_gpu_loss_kernels.py), checked on
the CPU so that it cannot be wrong unnoticed: against the golden vectors of the reference's own loss code, against
MaskFormerLoss.match_costs in double precision -- and the one place where the kernels deliberately do NOT follow the reference's
float32 arithmetic (saturated logits in the matching costs) pinned with figures."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref  # noqa: E402
from spike2former_amd.loss import _EPS32, MaskFormerLoss, seg_to_instances  # noqa: E402


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_mask_sums_reproduce_the_golden_mask_and_dice_losses(golden, name):
    """loss_mask / loss_dice of every decoder layer from loss_ref.mask_sums, the matches of MaskFormerLoss.assign and the formulas of
    loss_by_feat's fused branch == the values the reference's loss code stored, 1e-6 relative."""
    g = golden("loss_f1.npz")
    K = int(g[f"{name}_K"])
    cls, masks, seg = (torch.from_numpy(g[f"{name}_{k}"]) for k in ("cls", "masks", "seg"))
    L, B, Q, h, w = masks.shape
    H, W = seg.shape[-2:]
    assert (H, W) == (2 * h, 2 * w)
    crit = MaskFormerLoss(K, Q)
    gts = [seg_to_instances(seg[b]) for b in range(B)]
    matches = crit.assign(cls, masks, gts)
    offsets = np.cumsum([0] + [int(lab.numel()) for lab, _ in gts])
    tgt_u8 = torch.cat([m for _, m in gts]).to(torch.uint8)
    stored = dict(zip(g[f"{name}_keys"].tolist(), g[f"{name}_losses"].tolist()))
    for l in range(L):
        rows = np.concatenate([b * Q + matches[b][0][l] for b in range(B)])
        gt_index = torch.from_numpy(np.concatenate([offsets[b] + matches[b][1][l] for b in range(B)]))
        num_masks = max(float(sum(max(len(matches[b][0][l]), 1) for b in range(B))), 1.0)
        assert len(rows) > 0
        a, bsum, csum, fsum = loss_ref.mask_sums(masks[l].flatten(0, 1)[rows], tgt_u8, gt_index, crit.mask.alpha,
                                                 crit.mask.gamma).unbind(1)
        d = (2 * a + crit.dice.eps) / (bsum + csum + crit.dice.eps)
        loss_dice = float(crit.dice.loss_weight * (1 - d).sum() / (num_masks + _EPS32))
        loss_mask = float(crit.mask.loss_weight * fsum.sum() / (num_masks * (H * W) + _EPS32))
        prefix = "" if l == L - 1 else f"d{l}."
        assert abs(loss_dice - stored[prefix + "loss_dice"]) <= 1e-6 * abs(stored[prefix + "loss_dice"]), (l, loss_dice)
        assert abs(loss_mask - stored[prefix + "loss_mask"]) <= 1e-6 * abs(stored[prefix + "loss_mask"]), (l, loss_mask)


def test_seg_sums_are_mask_sums_of_the_compared_label_map():
    """seg_sums == mask_sums on `seg == class`; rows without a match: zeros, and no gradient reaches them."""
    g = torch.Generator().manual_seed(2)
    B, R, h, w = 2, 4, 3, 6
    pred = (torch.randn(B, R, h, w, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    seg = torch.randint(0, 4, (B, 2 * h, 2 * w), generator=g).to(torch.uint8)
    rc = torch.tensor([[0, -1, 3, 2], [1, 1, -1, 7]], dtype=torch.int32)
    got = loss_ref.seg_sums(pred, seg, rc, 0.25, 1.5)
    valid = (rc.reshape(-1) >= 0).nonzero().flatten()
    tgt = torch.stack([seg[int(i) // R] == int(rc.reshape(-1)[i]) for i in valid]).to(torch.uint8)
    want = loss_ref.mask_sums(pred.detach().reshape(B * R, h, w)[valid], tgt, torch.arange(len(valid)), 0.25, 1.5)
    assert torch.equal(got[valid], want)
    assert got[1].abs().max() == 0 and got[6].abs().max() == 0 and got[7, 2].item() == 0.0      # class 7 is absent: sum t = 0
    got.sum().backward()
    assert pred.grad[0, 1].abs().max() == 0 and pred.grad[1, 2].abs().max() == 0 and pred.grad[0, 0].abs().max() > 0


def _cost_inputs(seed, B, R, hw, K, saturated):
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(B, R, hw, generator=g) * 3
    if saturated:                                       # half of the logits beyond +/-20
        big = torch.tensor([20., -20., 50., -50., 90., -90., 120., -120.])[torch.randint(0, 8, (B, R, hw), generator=g)]
        u = torch.where(torch.rand(B, R, hw, generator=g) < 0.5, big + torch.randn(B, R, hw, generator=g), u)
    else:
        u = u.clamp(-10, 10)
    seg = torch.randint(0, K, (B, hw), generator=g).to(torch.uint8)
    seg[:, :hw // 8] = 255
    return u, seg


def test_cost_bins_with_the_normalisation_are_match_costs_in_double():
    """cost_bins + costs_all_classes' normalisation == MaskFormerLoss.match_costs run in double on the columns of the classes
    present, to 1e-12 (the two differ only in `1 - s` against sigmoid(-u), 1e-16 absolute at these logits)."""
    L, Q, K, h, w = 2, 5, 6, 6, 8
    g = torch.Generator().manual_seed(4)
    cls = torch.randn(L, Q, K + 1, generator=g, dtype=torch.float64)
    masks = torch.randn(L, Q, h, w, generator=g, dtype=torch.float64) * 3
    seg = torch.randint(0, K - 1, (2 * h, 2 * w), generator=g)              # class K - 1 is absent
    seg[:2] = 255
    crit = MaskFormerLoss(K, Q)
    labels, gm = seg_to_instances(seg)
    small_masks = torch.nn.functional.interpolate(gm.unsqueeze(1).float(), (h, w), mode="nearest").squeeze(1)
    want = crit.match_costs(cls, masks, labels, small_masks.double())
    small = seg[::2, ::2].reshape(1, h * w)
    cfg = crit.cost_focal_cfg
    bins, _ = loss_ref.cost_bins(masks.reshape(1, L * Q, h * w), small, K, cfg["alpha"], cfg["gamma"], cfg["eps"])
    count = torch.stack([(small == c).sum(1) for c in range(K)], 1)
    mask_cost = loss_ref.costs_from_bins(bins, count, K, h * w, crit.cost_focal, crit.cost_dice, crit.cost_dice_eps)
    got = (-cls.softmax(-1)[..., :K] * crit.cost_cls + mask_cost.view(L, Q, K))[:, :, labels]
    assert labels.tolist() == list(range(K - 1)) and want.abs().max() > 1
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


def test_the_fp32_reference_form_leaves_fp64_at_saturated_logits_only():
    """Why the cost kernel follows fp64 and not the reference's float32 expression: in float32 `1 - s` is exactly 0 once u > ~17, and
    -(1 - s + eps).log() then jumps to -log(1e-12) = 27.6 where the true value is ~u.  With half of the logits beyond +/-20 the
    float32 form misses the fp64 bins by more than 1e-2 of a bin's absolute-term sum (measured on these inputs: 0.098); with |u| <= 10 by
    less than 1e-4 (measured: 3.0e-6).  ops.mask_cost_bins forms 1 - s as sigmoid(-u), without the subtraction, and stays within 2e-5
    of fp64 in both regimes (tests/test_gpu_loss_kernels.py) -- so at saturated logits loss_semantic may assign differently from
    the reference's float32 costs.  That is deliberate."""
    B, R, hw, K = 2, 3, 1024, 7
    worst = {}
    for saturated in (True, False):
        u, seg = _cost_inputs(7, B, R, hw, K, saturated)
        want, absum = loss_ref.cost_bins(u, seg, K, 0.25, 2.0, 1e-12)
        got = loss_ref.cost_bins_fp32_reference_form(u, seg, K, 0.25, 2.0, 1e-12)
        worst[saturated] = ((got.double() - want).abs() / absum.clamp(min=1e-30)).max().item()
    print("fp32 reference form against fp64, worst bin / absolute-term sum:", worst)
    assert worst[True] > 1e-2
    assert worst[False] < 1e-4
