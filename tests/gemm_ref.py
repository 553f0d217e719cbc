"""Plain fp64 restatement of the 1x1 products (spike2former_amd/ops/gemm.py: spike_gemm, dense_gemm, spike_gemm_siblings, dx_gemm,
bmm_small) with their gradients -- a test helper, no conftest, nothing of the package imported: torch only (and tests/bn_ref.py for the
BatchNorm tile sums).  Written from the formulas, one batched matrix product per term, not from the kernels:

  product    x [B, G K, L], ws = G matrices [M, K], bias [G M] or None, gy [B, G M, L] or None; group g reads the rows g K .. (g + 1) K
             y[b, g M + m, l]  = sum_k ws[g][m, k] x[b, g K + k, l] + bias[g M + m]
             dx[b, g K + k, l] = sum_m ws[g][m, k] gy[b, g M + m, l]
             dw[g][m, k]       = sum_b sum_l gy[b, g M + m, l] x[b, g K + k, l];   db = sum over (b, l) of gy
  siblings   G maps xs[g] [B, K, L] of one shape (two may be the same map), ws[g] [M, K], gy [G, B, M, L] or None
             y[g] = ws[g] xs[g];  dx[g] = ws[g]^T gy[g] (per GROUP: a map read by two groups receives the sum of both);  dw[g] as above
  bmm        a [B, M, K] @ b [B, K, N] -> [B, M, N], or (reduce_batch) their sum over B -> [M, N]
  partials   the BatchNorm partials of a GEMM epilogue, [M, B ceil(L / 128), 2] fp32 (s2f_bn_partials_count): bn_ref.tile_partials at
             a tile of 128 columns over y padded with zero columns to a whole tile (a zero adds nothing to a sum or a sum of squares)

`dtype`: fp64 is the reference; fp32 evaluates the same association plainly, for measuring.  abs_sums: the same expressions on
absolute values.  The draw helpers of the route suite live here too, so that tests/test_gemm_ref_host.py can check them without a
GPU; that file also checks the closed forms against fp64 autograd of torch.einsum."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref  # noqa: E402

TILE = 128          # columns behind one BatchNorm partial of the GEMM epilogues (include/s2f.h)


def _cast(dtype, *ts):
    return tuple(None if t is None else t.to(dtype) for t in ts)


def product(x, ws, bias, gy, dtype=torch.float64):
    """-> {y [B, G M, L], dx [B, G K, L], dw (list of G [M, K]), db [G M] or None}  (gy None: forward only, the gradients are None)"""
    x, bias, gy = _cast(dtype, x, bias, gy)
    ws = list(_cast(dtype, *ws))
    G = len(ws)
    M, K = ws[0].shape
    B, GK, L = x.shape
    assert GK == G * K and all(tuple(w.shape) == (M, K) for w in ws)
    xg = x.view(B, G, K, L)
    y = torch.stack([torch.matmul(ws[g], xg[:, g]) for g in range(G)], 1).reshape(B, G * M, L)
    if bias is not None:
        y = y + bias.view(1, G * M, 1)
    if gy is None:
        return {"y": y, "dx": None, "dw": None, "db": None}
    gg = gy.view(B, G, M, L)
    dx = torch.stack([torch.matmul(ws[g].t(), gg[:, g]) for g in range(G)], 1).reshape(B, G * K, L)
    dw = [torch.matmul(gg[:, g], xg[:, g].transpose(1, 2)).sum(0) for g in range(G)]
    return {"y": y, "dx": dx, "dw": dw, "db": gy.sum((0, 2)) if bias is not None else None}


def siblings(xs, ws, gy, dtype=torch.float64):
    """-> {y [G, B, M, L], dx [G, B, K, L] (per group), dw (list of G [M, K])}"""
    outs = [product(x, [w], None, None if gy is None else gy[g], dtype) for g, (x, w) in enumerate(zip(xs, ws))]
    if gy is None:
        return {"y": torch.stack([o["y"] for o in outs], 0), "dx": None, "dw": None}
    return {"y": torch.stack([o["y"] for o in outs], 0), "dx": torch.stack([o["dx"] for o in outs], 0), "dw": [o["dw"][0] for o in outs]}


def bmm(a, b, reduce_batch=False, dtype=torch.float64):
    a, b = _cast(dtype, a, b)
    c = torch.matmul(a, b)
    return c.sum(0) if reduce_batch else c


def abs_sums(op, *args):
    """The sum of ABSOLUTE terms A behind every entry of what `op` (product, siblings or bmm of this file) returns for `args`: the same
    expressions on |.|, in fp64.  While such a sum stays below 2^24 granules -- the granule: the product of the operands' common
    denominators -- every partial sum of the entry is a whole number of granules below 2^24, i.e. exact in fp32 in ANY order."""
    def a(v):
        if torch.is_tensor(v):
            return v.double().abs()
        if isinstance(v, (list, tuple)):
            return [a(t) for t in v]
        return v
    return op(*[a(v) for v in args])


def partials(y):
    """y [B, M, L] -> [M, B ceil(L / 128), 2] fp32: the exact fp64 tile sums (sum, sum of squares), rounded to fp32 once"""
    B, M, L = y.shape
    Lp = -(-L // TILE) * TILE
    yp = torch.zeros(B, M, Lp, dtype=torch.float64)
    yp[:, :, :L] = y.detach().cpu().double()
    return bn_ref.tile_partials(yp, TILE)


def partials64(y):
    """the same tile sums in fp64, unrounded, and those of |y| and y^2's own absolute terms (= y^2): (sums [M, P, 2], abs [M, P, 2])"""
    B, M, L = y.shape
    Lp = -(-L // TILE) * TILE
    yp = torch.zeros(B, M, Lp, dtype=torch.float64)
    yp[:, :, :L] = y.detach().cpu().double()
    yt = yp.view(B, M, Lp // TILE, TILE)
    lay = lambda t: t.permute(1, 0, 2).reshape(M, B * (Lp // TILE))
    s1, s2, a1 = lay(yt.sum(3)), lay((yt * yt).sum(3)), lay(yt.abs().sum(3))
    return torch.stack([s1, s2], -1), torch.stack([a1, s2], -1)


# -------------------------------------------------------------------------------------------------------------- draws
def grid(g, lo, hi, *s):
    """integers lo .. hi as fp64"""
    return torch.randint(lo, hi + 1, s, generator=g).double()


def draw_spikes(g, *s):
    """sparse (25 %) multiples of 1/8 in [0, 1]"""
    return grid(g, 1, 8, *s) / 8 * (torch.rand(*s, generator=g) < 0.25)


def draw_eighths(g, *s):
    """multiples of 1/8 in [-1, 1]"""
    return grid(g, -8, 8, *s) / 8


def wide_values(g, *s):
    """20 significant bits per entry, v = +-(a / 8 + b 2^-11 + c 2^-19) with 4 <= a <= 8, 1 <= b <= 3, c odd below 8: hi = bf16(v) is
    a / 8, and the rest has set bits from 2^-11 or above down to 2^-19, more than the 8 significant bits of `mid` -- none of them is
    representable by two bf16 terms (asserted for EVERY entry)"""
    v = grid(g, 4, 8, *s) / 8 + grid(g, 1, 3, *s) * 2.0 ** -11 + (2 * grid(g, 0, 3, *s) + 1) * 2.0 ** -19
    v = v * (2 * grid(g, 0, 1, *s) - 1)
    hi = v.bfloat16().double()
    assert torch.equal(v.float().double(), v) and bool((hi + (v - hi).bfloat16().double() != v).all())
    return v


def one_hot(g, B, C, L):
    """[B, C, L] with ONE entry 1 per batch element"""
    x = torch.zeros(B, C, L, dtype=torch.float64)
    for b in range(B):
        x[b, int(torch.randint(0, C, (1,), generator=g)), int(torch.randint(0, L, (1,), generator=g))] = 1.0
    return x


def selection(g, M, K):
    """a 0/1 matrix [M, K] with at most one 1 per row AND per column (min(M, K) ones, at drawn places): a product with it picks
    single entries of the other operand, in either direction"""
    w = torch.zeros(M, K, dtype=torch.float64)
    n = min(M, K)
    w[torch.randperm(M, generator=g)[:n], torch.randperm(K, generator=g)[:n]] = 1.0
    return w
