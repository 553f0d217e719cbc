"""The mask losses of the Hungarian-matched loss (csrc/maskloss.hip) and the device-side assignment (csrc/lsa.hip)."""
import torch

from .core import *          # noqa: F401,F403  (the shared plumbing: _ptr, _stream, check, lib, Spikes, ...)


# ------------------------------------------------------------------------------------------------ mask losses (row f1)
class _MaskLossSums(torch.autograd.Function):
    """sums[p] = {sum s t, sum s, sum t, sum focal} over the 2x up-sampled logits of matched prediction p against its binary
    target (s2f.h s2f_mask_loss_fwd/bwd); nothing of size [P, 2h, 2w] exists forward, one such buffer backward."""

    @staticmethod
    def forward(ctx, pred, tgt, gt_index, alpha, gamma):
        _need_cuda(pred)
        pred = pred.contiguous()
        tgt = tgt.contiguous()
        P, h, w = pred.shape
        assert tgt.dtype == torch.uint8 and tgt.shape[1:] == (2 * h, 2 * w) and gt_index.dtype == torch.int64
        sums = torch.empty(P, 4, dtype=torch.float32, device=pred.device)
        check(lib.s2f_mask_loss_fwd(_ptr(pred), _ptr(tgt), _ptr(gt_index), _ptr(sums), P, h, w, alpha, gamma, _stream()),
              "s2f_mask_loss_fwd")
        ctx.save_for_backward(pred, tgt, gt_index)
        ctx.cfg = (alpha, gamma)
        return sums

    @staticmethod
    def backward(ctx, g):
        pred, tgt, gt_index = ctx.saved_tensors
        P, h, w = pred.shape
        g = g.contiguous()
        gup = torch.empty(P, 2 * h, 2 * w, dtype=torch.float32, device=pred.device)
        check(lib.s2f_mask_loss_bwd(_ptr(pred), _ptr(tgt), _ptr(gt_index), _ptr(g), _ptr(gup), P, h, w, *ctx.cfg, _stream()),
              "s2f_mask_loss_bwd")
        gp = torch.empty_like(pred)
        check(lib.s2f_upsample2x_bwd(_ptr(gup), _ptr(gp), P, h, w, _stream()), "s2f_upsample2x_bwd")
        return gp, None, None, None, None


def mask_loss_sums(pred, tgt_u8, gt_index, alpha, gamma):
    """pred [P, h, w] fp32 logits, tgt_u8 [G, 2h, 2w] uint8 0/1, gt_index [P] int64 -> [P, 4]"""
    return _MaskLossSums.apply(pred, tgt_u8, gt_index, float(alpha), float(gamma))


def mask_cost_bins(pred, seg_small, K, alpha, gamma, eps):
    """pred [B, R, hw] fp32 logits, seg_small [B, hw] uint8 label map -> [B, R, 2K + 2]: per class id the segmented sums of
    (pos - neg) and of s, then sum neg and sum s over all pixels (s2f.h s2f_mask_cost_bins; match_cost.py:289-297, :361-371)."""
    _need_cuda(pred)
    pred, seg_small = pred.contiguous(), seg_small.contiguous()
    B, R, hw = pred.shape
    assert seg_small.dtype == torch.uint8 and seg_small.shape == (B, hw) and pred.dtype == torch.float32
    out = torch.empty(B, R, 2 * K + 2, dtype=torch.float32, device=pred.device)
    check(lib.s2f_mask_cost_bins(_ptr(pred), _ptr(seg_small), _ptr(out), B, R, hw, K, alpha, gamma, eps, _stream()),
          "s2f_mask_cost_bins")
    return out


LSA_MAX_QUERIES, LSA_MAX_CLASSES = 256, 254          # include/s2f.h S2F_LSA_MAX_QUERIES / S2F_LSA_MAX_CLASSES
LSA_TILE_L2 = 1                                      # include/s2f.h S2F_LSA_TILE_L2 (the flags word of s2f_lsa_tables_ex)


def lsa_tables(cost, count_full, K, out=None, tile_l2=False):
    """The Hungarian assignment of the semantic-map loss on the device (s2f.h s2f_lsa_tables): cost [L, B, Q, K] fp32 and
    count_full [B, 256] fp32 as MaskFormerLoss.costs_all_classes returns them -> (tgt_labels [L, B, Q] int64, row_class [B, L*Q]
    int32, num_masks [L] fp32, status [1] int32) -- the three tables of MaskFormerLoss.match_tables plus a status word (bit 0: a
    label in K..254 is present, bit 1: a non-finite cost in a present column; num_masks is NaN then).  `out`: those four tensors
    to write into (static buffers of a captured step); every element is written.  No autograd; nothing synchronises.
    `tile_l2` (measurement only, tools/probe_lsa.py): re-read the costs from L2 instead of keeping the fp64 tile in LDS."""
    if not (cost.is_cuda and count_full.is_cuda):
        raise RuntimeError("ops.lsa_tables runs on the GPU only (HIP kernel, no host fall-back); got a CPU tensor -- "
                           "the host route is MaskFormerLoss.match_tables (assign='host')")
    if cost.dtype != torch.float32 or count_full.dtype != torch.float32:
        raise RuntimeError(f"ops.lsa_tables takes fp32 costs and counts; got {cost.dtype}, {count_full.dtype}")
    if cost.dim() != 4 or cost.shape[3] != K:
        raise ValueError(f"cost [L, B, Q, K = {K}], got {tuple(cost.shape)}")
    L, B, Q = cost.shape[:3]
    if tuple(count_full.shape) != (B, 256) or count_full.device != cost.device:
        raise ValueError(f"count_full [B = {B}, 256] on {cost.device}, got {tuple(count_full.shape)} on {count_full.device}")
    cost, count_full = cost.detach().contiguous(), count_full.detach().contiguous()
    dev = cost.device
    if out is None:
        out = (torch.empty(L, B, Q, dtype=torch.int64, device=dev), torch.empty(B, L * Q, dtype=torch.int32, device=dev),
               torch.empty(L, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    tgt, rows, num_masks, status = out
    for t, shape, dtype in ((tgt, (L, B, Q), torch.int64), (rows, (B, L * Q), torch.int32), (num_masks, (L,), torch.float32),
                            (status, (1,), torch.int32)):
        if not (t.device == dev and tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()):
            raise ValueError(f"out: a contiguous {dtype} tensor of shape {shape} on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    args = (_ptr(cost), _ptr(count_full), _ptr(tgt), _ptr(rows), _ptr(num_masks), _ptr(status), L, B, Q, int(K))
    if tile_l2:
        check(lib.s2f_lsa_tables_ex(*args, LSA_TILE_L2, _stream()), "s2f_lsa_tables_ex")
    else:
        check(lib.s2f_lsa_tables(*args, _stream()), "s2f_lsa_tables")
    return tgt, rows, num_masks, status


class _MaskLossSeg(torch.autograd.Function):
    """sums[(b, r)] = {sum s t, sum s, sum t, sum focal} of the 2x up-sampled logits pred[b, r] against  seg[b] == row_class[b, r]
    (rows with row_class < 0: zeros, zero gradient); s2f.h s2f_mask_loss_seg_fwd/bwd."""

    @staticmethod
    def forward(ctx, pred, seg, row_class, alpha, gamma):
        _need_cuda(pred)
        pred = pred.contiguous()
        B, R, h, w = pred.shape
        assert seg.dtype == torch.uint8 and seg.shape == (B, 2 * h, 2 * w) and seg.is_contiguous()
        assert row_class.dtype == torch.int32 and row_class.numel() == B * R and row_class.is_contiguous()
        sums = torch.empty(B * R, 4, dtype=torch.float32, device=pred.device)
        part = torch.empty(int(lib.s2f_mask_loss_seg_partials(B, R, h, w)), dtype=torch.float32, device=pred.device)
        check(lib.s2f_mask_loss_seg_fwd(_ptr(pred), _ptr(seg), _ptr(row_class), _ptr(sums), _ptr(part), B, R, h, w, alpha, gamma,
                                        _stream()), "s2f_mask_loss_seg_fwd")
        ctx.save_for_backward(pred, seg, row_class)
        ctx.cfg = (alpha, gamma)
        return sums

    @staticmethod
    def backward(ctx, g):
        pred, seg, row_class = ctx.saved_tensors
        B, R, h, w = pred.shape
        gp = torch.empty_like(pred)
        check(lib.s2f_mask_loss_seg_bwd(_ptr(pred), _ptr(seg), _ptr(row_class), _ptr(g.contiguous()), _ptr(gp), B, R, h, w, *ctx.cfg,
                                        _stream()), "s2f_mask_loss_seg_bwd")
        return gp, None, None, None, None


def mask_loss_seg(pred, seg_u8, row_class, alpha, gamma):
    """pred [B, R, h, w] fp32 logits, seg_u8 [B, 2h, 2w] uint8 label map, row_class [B * R] int32 -> sums [B * R, 4]"""
    return _MaskLossSeg.apply(pred, seg_u8, row_class, float(alpha), float(gamma))


__all__ = [n for n in dir() if not n.startswith('__')]
