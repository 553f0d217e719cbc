"""tests/gemm_ref.py against fp64 autograd of torch.einsum (no GPU): the closed forms of the 1x1 products and their gradients, abs_sums
against the same operations on absolute values, the BatchNorm tile sums, and the draw helpers of the route suite."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref  # noqa: E402
import gemm_ref  # noqa: E402


def _draw(B, G, M, K, L, bias, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return r(B, G * K, L), [r(M, K) for _ in range(G)], (r(G * M) if bias else None), r(B, G * M, L)


@pytest.mark.parametrize("B,G,M,K,L,bias", [(2, 1, 5, 7, 6, False), (3, 1, 4, 3, 5, True), (2, 3, 4, 5, 9, False), (1, 2, 3, 2, 4, True)])
def test_product_against_autograd_of_einsum(B, G, M, K, L, bias):
    x, ws, b, gy = _draw(B, G, M, K, L, bias, B + G + M)
    xl = x.clone().requires_grad_(True)
    wl = [w.clone().requires_grad_(True) for w in ws]
    bl = None if b is None else b.clone().requires_grad_(True)
    y = torch.einsum("gmk,bgkl->bgml", torch.stack(wl, 0), xl.view(B, G, K, L)).reshape(B, G * M, L)
    if bl is not None:
        y = y + bl.view(1, -1, 1)
    y.backward(gy)
    got = gemm_ref.product(x, ws, b, gy)
    tol = dict(rtol=0, atol=1e-12)
    torch.testing.assert_close(got["y"], y.detach(), **tol)
    torch.testing.assert_close(got["dx"], xl.grad, **tol)
    for g in range(G):
        torch.testing.assert_close(got["dw"][g], wl[g].grad, **tol)
    if b is None:
        assert got["db"] is None
    else:
        torch.testing.assert_close(got["db"], bl.grad, **tol)
    fwd = gemm_ref.product(x, ws, b, None)
    assert torch.equal(fwd["y"], got["y"]) and fwd["dx"] is None and fwd["dw"] is None and fwd["db"] is None
    f32 = gemm_ref.product(x, ws, b, gy, torch.float32)
    assert f32["y"].dtype == torch.float32 and f32["dw"][0].dtype == torch.float32
    torch.testing.assert_close(f32["y"].double(), got["y"], rtol=0, atol=1e-4)


def test_siblings_share_a_map_and_sum_its_gradient():
    B, M, K, L = 2, 4, 5, 6
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    xa, xb = r(B, K, L).requires_grad_(True), r(B, K, L).requires_grad_(True)
    ws = [r(M, K).requires_grad_(True) for _ in range(3)]
    gy = r(3, B, M, L)
    maps = [xa, xb, xb]          # k and v read the SAME map
    y = torch.stack([torch.einsum("mk,bkl->bml", w, x) for w, x in zip(ws, maps)], 0)
    y.backward(gy)
    got = gemm_ref.siblings([m.detach() for m in maps], [w.detach() for w in ws], gy)
    tol = dict(rtol=0, atol=1e-12)
    torch.testing.assert_close(got["y"], y.detach(), **tol)
    torch.testing.assert_close(got["dx"][0], xa.grad, **tol)
    torch.testing.assert_close(got["dx"][1] + got["dx"][2], xb.grad, **tol)
    for i in range(3):
        torch.testing.assert_close(got["dw"][i], ws[i].grad, **tol)


@pytest.mark.parametrize("reduce_batch", [False, True])
def test_bmm_against_einsum(reduce_batch):
    g = torch.Generator().manual_seed(4)
    a, b = torch.randn(3, 5, 7, generator=g, dtype=torch.float64), torch.randn(3, 7, 4, generator=g, dtype=torch.float64)
    want = torch.einsum("bmk,bkn->mn" if reduce_batch else "bmk,bkn->bmn", a, b)
    torch.testing.assert_close(gemm_ref.bmm(a, b, reduce_batch), want, rtol=0, atol=1e-12)
    assert gemm_ref.bmm(a, b, reduce_batch, torch.float32).dtype == torch.float32


def test_abs_sums_are_the_same_operations_on_absolute_values():
    B, G, M, K, L = 2, 2, 3, 4, 5
    x, ws, b, gy = _draw(B, G, M, K, L, True, 11)
    A = gemm_ref.abs_sums(gemm_ref.product, x, ws, b, gy)
    want = gemm_ref.product(x.abs(), [w.abs() for w in ws], b.abs(), gy.abs())
    for k in ("y", "dx", "db"):
        assert torch.equal(A[k], want[k])
    assert all(torch.equal(p, q) for p, q in zip(A["dw"], want["dw"]))
    # an explicit entry: A_y[b, m, l] = sum_k |w[m, k]| |x[b, k, l]| + |bias[m]|
    e = (ws[1][2].abs() * x[1, K:, 3].abs()).sum() + b[M + 2].abs()
    assert abs(A["y"][1, M + 2, 3].item() - e.item()) <= 1e-12
    # every entry bounds its signed value
    ref = gemm_ref.product(x, ws, b, gy)
    assert bool((ref["y"].abs() <= A["y"] + 1e-12).all()) and bool((ref["dx"].abs() <= A["dx"] + 1e-12).all())
    S = gemm_ref.abs_sums(gemm_ref.siblings, [x[:, :K], x[:, K:]], ws, gy.view(B, G, M, L).transpose(0, 1))
    assert torch.equal(S["dx"][0], A["dx"][:, :K])
    a, c = torch.randn(2, 3, 4, dtype=torch.float64), torch.randn(2, 4, 5, dtype=torch.float64)
    assert torch.equal(gemm_ref.abs_sums(gemm_ref.bmm, a, c, True), torch.matmul(a.abs(), c.abs()).sum(0))


@pytest.mark.parametrize("L", [128, 136, 36, 256])
def test_partials_are_the_tile_sums_in_the_layout_of_the_epilogue(L):
    B, M = 2, 3
    y = torch.randn(B, M, L, generator=torch.Generator().manual_seed(L))
    P = B * -(-L // 128)
    part = gemm_ref.partials(y)
    assert tuple(part.shape) == (M, P, 2) and part.dtype == torch.float32
    s64, a64 = gemm_ref.partials64(y)
    assert torch.equal(s64.float(), part)
    for b in range(B):
        for t in range(-(-L // 128)):
            tile = y[b, :, 128 * t:128 * (t + 1)].double()
            p = b * -(-L // 128) + t
            torch.testing.assert_close(s64[:, p, 0], tile.sum(1), rtol=0, atol=1e-12)
            torch.testing.assert_close(s64[:, p, 1], (tile * tile).sum(1), rtol=0, atol=1e-12)
            torch.testing.assert_close(a64[:, p, 0], tile.abs().sum(1), rtol=0, atol=1e-12)
    if L % 128 == 0:
        assert torch.equal(part, bn_ref.tile_partials(y, 128))


def test_draw_helpers():
    g = torch.Generator().manual_seed(5)
    v = gemm_ref.wide_values(g, 64, 33)
    hi = v.bfloat16().double()
    mid = (v - hi).bfloat16().double()
    lo = (v - hi - mid).bfloat16().double()
    assert bool((hi + mid != v).all())          # every entry fails the two-term representation ...
    assert torch.equal(hi + mid + lo, v)        # ... and three terms hold it
    assert torch.equal(v.float().double(), v) and bool((v.abs() >= 0.5).all()) and bool((v.abs() < 1.01).all())
    s = gemm_ref.draw_spikes(g, 4, 16, 40)
    assert torch.equal(s * 8, (s * 8).round()) and s.min().item() >= 0 and s.max().item() <= 1
    assert 0.15 < (s != 0).double().mean().item() < 0.35
    assert torch.equal(s.bfloat16().double(), s)
    e = gemm_ref.draw_eighths(g, 50, 50)
    assert torch.equal(e * 8, (e * 8).round()) and e.abs().max().item() <= 1
    h = gemm_ref.one_hot(g, 3, 5, 7)
    assert torch.equal(h.sum((1, 2)), torch.ones(3, dtype=torch.float64)) and set(h.unique().tolist()) == {0.0, 1.0}
    for M, K in ((6, 9), (9, 6), (5, 5)):
        w = gemm_ref.selection(g, M, K)
        assert w.sum().item() == min(M, K) and w.sum(0).max().item() == 1 and w.sum(1).max().item() == 1
