"""Plain fp64 restatement of the head's mask contraction and of the products around it (spike2former_amd/ops/gemm.py:
mask_einsum_folded, mask_einsum, class_mask_product, linear_tm) -- a test helper, no conftest, nothing of the package imported: torch
only.  Written from the formulas (maskformer_head.py:582-583 on pixel_decoder.py:467-470), not from the kernels:

  folded     out[b]   = scale sum_t E[t,b] (W S[t,b] + bias 1^T)
                      = scale ( sum_t EW[t,b] S[t,b] + rowb[b] 1^T ),   EW[t,b] = E[t,b] W,   rowb[b] = sum_t E[t,b] bias
             dS[t,b]  = scale EW[t,b]^T g[b]
             H[t,b]   = g[b] S[t,b]^T,   rs[b] = g[b] 1 (the row sums of g)
             dE[t,b]  = scale ( H[t,b] W^T + rs[b] bias^T )
             dW       = scale sum_{t,b} E[t,b]^T H[t,b]
             dbias    = scale sum_{t,b} E[t,b]^T rs[b]
  unfolded   out[b]   = scale sum_t E[t,b] MF[t,b];   dE[t,b] = scale g[b] MF[t,b]^T;   dMF[t,b] = scale E[t,b]^T g[b]
  class_mask out[b]   = cls[b]^T masks[b]                          (einsum 'bqc,bqhw->bchw')
  linear     y = x W^T + b;   gx = gy W;   gW = gy^T x;   gb = 1^T gy

Shapes: E [T,B,Q,Co], S [T,B,C,HW], W [Co,C], bias [Co] or None, g [B,Q,HW].  `dtype`: fp64 is the reference; fp32 evaluates the same
association plainly, for measuring.  tests/test_mask_ref_host.py checks the closed forms against autograd of the two-step expression
(the 1x1 convolution, then einsum('tbqc,tbchw->tbqhw') summed over t) and abs_sums against a per-element loop."""
import torch


def _cast(dtype, *ts):
    return tuple(None if t is None else t.to(dtype) for t in ts)


def forward_folded(E, S, W, bias, scale, dtype=torch.float64):
    """-> (out [B,Q,HW], EW [T,B,Q,C], rowb [B,Q] or None)"""
    E, S, W, bias = _cast(dtype, E, S, W, bias)
    EW = torch.einsum("tbqo,oc->tbqc", E, W)
    acc = torch.einsum("tbqc,tbcn->bqn", EW, S)
    rowb = None
    if bias is not None:
        rowb = torch.einsum("tbqo,o->bq", E, bias)
        acc = acc + rowb.unsqueeze(-1)
    return acc * scale, EW, rowb


def backward_folded(E, S, W, bias, g, scale, dtype=torch.float64):
    """-> dict: dS [T,B,C,HW], dE [T,B,Q,Co], dW [Co,C], dbias [Co] or None, and the intermediates EW [T,B,Q,C], H [T,B,Q,C] (both
    without the scale) and rs [B,Q]"""
    E, S, W, bias, g = _cast(dtype, E, S, W, bias, g)
    EW = torch.einsum("tbqo,oc->tbqc", E, W)
    dS = torch.einsum("tbqc,bqn->tbcn", EW, g) * scale
    H = torch.einsum("bqn,tbcn->tbqc", g, S)
    rs = g.sum(-1)
    dE = torch.einsum("tbqc,oc->tbqo", H, W)
    dbias = None
    if bias is not None:
        dE = dE + rs.unsqueeze(0).unsqueeze(-1) * bias
        dbias = torch.einsum("tbqo,bq->o", E, rs) * scale
    dW = torch.einsum("tbqo,tbqc->oc", E, H) * scale
    return {"dS": dS, "dE": dE * scale, "dW": dW, "dbias": dbias, "EW": EW, "H": H, "rs": rs}


def abs_sums(E, S, W, bias, g):
    """The sum of ABSOLUTE terms behind every entry of out, dS, dE, dW, dbias and of the intermediates the op holds in fp32 (EW, rowb,
    H, rs = rowsum(g)), scale 1: the same expressions on absolute values (the intermediates that enter a second sum are thereby replaced
    by their own sums of absolute terms: an upper bound).  While such a sum stays below 2^24 granules -- the granule: the product of the
    operands' common denominators -- every partial sum of the entry is a whole number of granules below 2^24, i.e. exact in fp32 in ANY
    order of the additions."""
    E, S, W, g = (t.double().abs() for t in (E, S, W, g))
    bias = None if bias is None else bias.double().abs()
    out, EW, rowb = forward_folded(E, S, W, bias, 1.0)
    sums = backward_folded(E, S, W, bias, g, 1.0)
    sums.update(out=out, rowb=rowb)
    return sums


def forward_unfolded(E, MF, scale, dtype=torch.float64):
    """E [T,B,Q,C], MF [T,B,C,HW] -> out [B,Q,HW]"""
    E, MF = _cast(dtype, E, MF)
    return torch.einsum("tbqc,tbcn->bqn", E, MF) * scale


def backward_unfolded(E, MF, g, scale, dtype=torch.float64):
    """-> (dE [T,B,Q,C], dMF [T,B,C,HW])"""
    E, MF, g = _cast(dtype, E, MF, g)
    return torch.einsum("bqn,tbcn->tbqc", g, MF) * scale, torch.einsum("tbqc,bqn->tbcn", E, g) * scale


def abs_sums_unfolded(E, MF, g):
    E, MF, g = (t.double().abs() for t in (E, MF, g))
    dE, dMF = backward_unfolded(E, MF, g, 1.0)
    return {"out": forward_unfolded(E, MF, 1.0), "dE": dE, "dMF": dMF}


def class_mask(cls_score, mask_probs, dtype=torch.float64):
    """cls_score [B,Q,K], mask_probs [B,Q,h,w] -> [B,K,h,w]"""
    cls_score, mask_probs = _cast(dtype, cls_score, mask_probs)
    return torch.einsum("bqc,bqhw->bchw", cls_score, mask_probs)


def linear(x, w, b, gy, dtype=torch.float64):
    """x [n,c], w [o,c], b [o] or None, gy [n,o] -> (y, gx, gw, gb or None)"""
    x, w, b, gy = _cast(dtype, x, w, b, gy)
    y = x @ w.t()
    if b is not None:
        y = y + b
    return y, gy @ w, gy.t() @ x, (gy.sum(0) if b is not None else None)
