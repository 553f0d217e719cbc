"""Plain fp64 restatement of the mask-loss and matching-cost kernels (spike2former_amd/csrc/upsample.hip s2f_mask_loss_fwd/bwd,
spike2former_amd/csrc/maskloss.hip s2f_mask_loss_seg_fwd/bwd and s2f_mask_cost_bins) -- a test helper, no conftest, nothing of the
package imported: torch only.  Written from the formulas the kernels' headers quote (F.interpolate(scale 2, bilinear,
align_corners=False); losses/focal_loss.py:36-44; match_cost.py:289-297, :361-371), not from the kernels: every function is the
textbook expression on float64 tensors (or on `dtype`, for measuring what ATen's fp32 evaluation of the same expression gives),
gradients come from autograd on that graph.  tests/test_loss_ref_host.py checks this file on the CPU against the golden vectors of
the reference's own loss code and against MaskFormerLoss.match_costs in double precision."""
import torch
import torch.nn.functional as F


def _sums(pred, tgt, alpha, gamma):
    """pred [N, h, w] logits, tgt [N, 2h, 2w] 0/1 of pred's dtype -> [N, 4] = {sum s t, sum s, sum t, sum focal}"""
    u = F.interpolate(pred.unsqueeze(1), scale_factor=2, mode="bilinear", align_corners=False).squeeze(1)
    s = u.sigmoid()
    pt = (1 - s) * tgt + s * (1 - tgt)
    focal = F.binary_cross_entropy_with_logits(u, tgt, reduction="none") * (alpha * tgt + (1 - alpha) * (1 - tgt)) * pt.pow(gamma)
    return torch.stack([(s * tgt).flatten(1).sum(1), s.flatten(1).sum(1), tgt.flatten(1).sum(1), focal.flatten(1).sum(1)], 1)


def mask_sums(pred, tgt_u8, gt_index, alpha, gamma, dtype=torch.float64):
    """pred [P, h, w] (a leaf that requires grad receives the gradient), tgt_u8 [G, 2h, 2w] 0/1, gt_index [P] -> [P, 4] in `dtype`"""
    return _sums(pred.to(dtype), (tgt_u8[gt_index.long()] != 0).to(dtype), alpha, gamma)


def seg_sums(pred, seg_u8, row_class, alpha, gamma, dtype=torch.float64):
    """pred [B, R, h, w], seg_u8 [B, 2h, 2w] label map, row_class [B, R] (or [B * R]) -> [B * R, 4] in `dtype`: the target of row
    (b, r) is  seg[b] == row_class[b, r];  rows with row_class < 0 give zeros (and no gradient)."""
    B, R, h, w = pred.shape
    rc = row_class.reshape(B, R).long()
    tgt = (seg_u8.long()[:, None] == rc[:, :, None, None]).to(dtype).reshape(B * R, 2 * h, 2 * w)
    sums = _sums(pred.to(dtype).reshape(B * R, h, w), tgt, alpha, gamma)
    return sums * (rc.reshape(-1, 1) >= 0).to(dtype)


def _bins(pos, neg, s, seg_small, K):
    B, R, hw = s.shape
    out = s.new_zeros(B, R, 2 * K + 2)
    absum = s.new_zeros(B, R, 2 * K + 2)
    lab = seg_small.long()
    for c in range(K):
        m = (lab == c).to(s.dtype)[:, None, :]                                               # [B, 1, hw]
        out[..., c] = ((pos - neg) * m).sum(-1)
        out[..., K + c] = absum[..., K + c] = (s * m).sum(-1)
        absum[..., c] = ((pos.abs() + neg.abs()) * m).sum(-1)
    out[..., 2 * K] = absum[..., 2 * K] = neg.sum(-1)
    out[..., 2 * K + 1] = absum[..., 2 * K + 1] = s.sum(-1)
    return out, absum


def cost_bins(pred, seg_small, K, alpha, gamma, eps, dtype=torch.float64):
    """pred [B, R, hw] logits, seg_small [B, hw] labels -> (bins, absum), each [B, R, 2K + 2] in `dtype`:
      bins[..., c] = sum over the pixels of class c < K of (pos - neg),  bins[..., K + c] = sum of s over them,
      bins[..., 2K] = sum of neg over all pixels,  bins[..., 2K + 1] = sum of s over all pixels
    with  s = sigmoid(u), c = sigmoid(-u) = 1 - s WITHOUT the subtraction,  pos = -log(s + eps) alpha c^gamma,
    neg = -log(c + eps) (1 - alpha) s^gamma.  `absum` is the sum of |pos| + |neg| behind every bins entry (the s entries: sum s; the
    neg total: sum neg), the scale a tolerance on a bin refers to."""
    u = pred.to(dtype)
    s, c = u.sigmoid(), (-u).sigmoid()
    pos = -(s + eps).log() * alpha * c.pow(gamma)
    neg = -(c + eps).log() * (1 - alpha) * s.pow(gamma)
    return _bins(pos, neg, s, seg_small, K)


def cost_bins_fp32_reference_form(pred, seg_small, K, alpha, gamma, eps):
    """The same bins from the reference's own expression evaluated in float32 (match_cost.py:289-297 as
    MaskFormerLoss.match_costs restates it): `1 - s` is a float32 subtraction, which is exactly 0 once u > ~17, so
    -(1 - s + eps).log() jumps to -log(eps) = 27.6 there, where the true value is ~u.  Kept to DOCUMENT how far that expression is
    from its own double-precision value at saturated logits; nothing in the package follows it.  Returns bins only (float32)."""
    u = pred.float()
    s = u.sigmoid()
    neg = -(1 - s + eps).log() * (1 - alpha) * s.pow(gamma)
    pos = -(s + eps).log() * alpha * (1 - s).pow(gamma)
    return _bins(pos, neg, s, seg_small, K)[0]


def costs_from_bins(bins, count_small, K, hw, w_focal=20.0, w_dice=1.0, dice_eps=1.0):
    """The mask part of MaskFormerLoss.costs_all_classes' normalisation: bins [B, R, 2K + 2], count_small [B, K] (pixels of every
    class in the small label map) -> focal * w_focal + dice * w_dice, [B, R, K]"""
    D, S, neg, stot = bins[..., :K], bins[..., K:2 * K], bins[..., 2 * K:2 * K + 1], bins[..., 2 * K + 1:]
    focal = (D + neg) / hw
    dice = 1 - (2 * S + dice_eps) / (stot + count_small[:, None, :].to(bins.dtype) + dice_eps)
    return focal * w_focal + dice * w_dice
