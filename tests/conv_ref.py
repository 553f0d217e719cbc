"""Plain fp64 restatement of the dense k x k convolution and of the depthwise stencil (spike2former_amd/ops/conv.py: conv_dense,
dwconv) with their gradients -- a test helper, no conftest, nothing of the package imported: torch only.  Written from the formulas,
one shifted slice and one multiply-add per tap (i, j), not from the kernels and not through F.conv2d:

  dense      xp        = x with a ring of `pad` zeros
             X_ij      = xp[:, :, i : i + s Ho : s, j : j + s Wo : s]                      (the map the tap (i, j) reads, stride s)
             y         = sum_ij w[:, :, i, j] X_ij + bias                                   (contraction over the input channels)
             dxp_ij   += w[:, :, i, j]^T gy        (added at the positions X_ij reads);   dx = the interior of dxp
             dw[:, :, i, j] = sum_n gy[n] X_ij[n]^T;   db = sum over (n, h, w) of gy
  depthwise  xp        = x with a ring of `pad` entries that hold border[c] (BNAndPadLayer; zeros without a border)
             y[:, c]   = sum_ij w[c, i, j] xp[:, c, i : i + Ho, j : j + Wo]
             dx        = the interior of dxp,  dxp[:, c, i : i + Ho, j : j + Wo] += w[c, i, j] gy[:, c]
             dw[c, i, j] = sum over (n, h, w) of gy[:, c] xp[:, c, i : i + Ho, j : j + Wo]   (the ring's constants count; the border
                           itself is detached and receives no gradient)

Shapes: x [N, C, H, W], dense w [M, C, k, k], bias [M] or None, depthwise w [C, 1, K, K], border [C] or None, gy the output's shape.
`dtype`: fp64 is the reference; fp32 evaluates the same association plainly, for measuring.  tests/test_conv_ref_host.py checks the
closed forms against autograd of F.conv2d in fp64 and abs_sums against the same operations on absolute values."""
import torch


def _cast(dtype, *ts):
    return tuple(None if t is None else t.to(dtype) for t in ts)


def _padded(x, pad, border=None):
    """x inside a ring of `pad` entries: zeros, or the per-channel constant border[c]"""
    N, C, H, W = x.shape
    xp = x.new_zeros(N, C, H + 2 * pad, W + 2 * pad)
    if border is not None:
        xp += border.view(1, C, 1, 1)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    return xp


def conv_dense(x, w, bias, stride, pad, gy, dtype=torch.float64):
    """nn.Conv2d(C, M, k, stride, pad) and its gradients -> {y [N, M, Ho, Wo], dx [N, C, H, W], dw [M, C, k, k], db [M] or None}
    (gy None: forward only, the gradients are None)"""
    x, w, bias, gy = _cast(dtype, x, w, bias, gy)
    N, C, H, W = x.shape
    M, _, kh, kw = w.shape
    s = stride
    Ho, Wo = (H + 2 * pad - kh) // s + 1, (W + 2 * pad - kw) // s + 1
    xp = _padded(x, pad)
    taps = [(i, j, slice(i, i + s * (Ho - 1) + 1, s), slice(j, j + s * (Wo - 1) + 1, s)) for i in range(kh) for j in range(kw)]
    y = x.new_zeros(N, M, Ho, Wo)
    for i, j, rows, cols in taps:
        y += torch.einsum("mc,nchw->nmhw", w[:, :, i, j], xp[:, :, rows, cols])
    if bias is not None:
        y += bias.view(1, M, 1, 1)
    if gy is None:
        return {"y": y, "dx": None, "dw": None, "db": None}
    dxp, dw = torch.zeros_like(xp), torch.zeros_like(w)
    for i, j, rows, cols in taps:
        dxp[:, :, rows, cols] += torch.einsum("mc,nmhw->nchw", w[:, :, i, j], gy)
        dw[:, :, i, j] = torch.einsum("nmhw,nchw->mc", gy, xp[:, :, rows, cols])
    return {"y": y, "dx": dxp[:, :, pad:pad + H, pad:pad + W].contiguous(), "dw": dw,
            "db": gy.sum((0, 2, 3)) if bias is not None else None}


def dwconv(x, w, pad, border, gy, dtype=torch.float64):
    """nn.Conv2d(C, C, K, 1, 0, groups=C) on x padded by `pad` entries of border[c] (zeros for None), and its gradients
    -> {y [N, C, Ho, Wo], dx [N, C, H, W], dw [C, 1, K, K]}  (gy None: forward only)"""
    x, w, border, gy = _cast(dtype, x, w, border, gy)
    N, C, H, W = x.shape
    K = w.shape[-1]
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    xp = _padded(x, pad, border)
    wk = w.reshape(C, K, K)
    y = x.new_zeros(N, C, Ho, Wo)
    for i in range(K):
        for j in range(K):
            y += wk[:, i, j].view(1, C, 1, 1) * xp[:, :, i:i + Ho, j:j + Wo]
    if gy is None:
        return {"y": y, "dx": None, "dw": None}
    dxp, dw = torch.zeros_like(xp), torch.zeros_like(wk)
    for i in range(K):
        for j in range(K):
            dxp[:, :, i:i + Ho, j:j + Wo] += wk[:, i, j].view(1, C, 1, 1) * gy
            dw[:, i, j] = (gy * xp[:, :, i:i + Ho, j:j + Wo]).sum((0, 2, 3))
    return {"y": y, "dx": dxp[:, :, pad:pad + H, pad:pad + W].contiguous(), "dw": dw.reshape(w.shape)}


def abs_sums(op, *args):
    """The sum of ABSOLUTE terms A behind every entry of what `op` (conv_dense or dwconv of this file) returns for `args`: the same
    expressions on |x|, |w|, |bias|, |gy| (and |border|), in fp64.  While such a sum stays below 2^24 granules -- the granule: the
    product of the operands' common denominators -- every partial sum of the entry is a whole number of granules below 2^24, i.e.
    exact in fp32 in ANY order of the additions."""
    return op(*[a.double().abs() if torch.is_tensor(a) else a for a in args])
