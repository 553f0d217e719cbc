"""CPU: the fp64 restatement of the DCNv3 sampling core that tests/test_gpu_dcn_routes.py compares the kernels with
(tests/dcn_ref.py) -- its closed-form gradients against autograd through the oracle (square geometries) and through F.grid_sample
on the padded map (a Kh != Kw window, separate strides, pads and dilations), abs_sums against the same operations on absolute
values and against a loop over single terms, and all four results against the vectors captured from the reference."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import s2f_oracle as so

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_ref  # noqa: E402


def _maps(N, H, W, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw, seed):
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = dcn_ref.out_hw(H, W, Kh, Kw, sh, sw, ph, pw, dh, dw)
    P = Kh * Kw
    x = torch.randn(N, H, W, G * Cg, generator=g, dtype=torch.float64)
    off = torch.randn(N, Ho, Wo, G * P * 2, generator=g, dtype=torch.float64) * 2
    m = torch.randn(N, Ho, Wo, G * P, generator=g, dtype=torch.float64)
    gy = torch.randn(N, Ho, Wo, G * Cg, generator=g, dtype=torch.float64)
    return x, off, m, gy


def _close(a, b, tol=1e-12):
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


# (N, H, W, G, Cg, K, stride, pad, dil, offset_scale)
SQUARE = [(2, 5, 7, 3, 4, 3, 1, 1, 1, 1.0), (1, 9, 8, 2, 3, 3, 2, 1, 1, 0.5), (1, 7, 7, 2, 2, 3, 1, 2, 2, 2.0),
          (1, 6, 9, 1, 5, 5, 1, 2, 1, 1.5), (2, 4, 4, 2, 8, 3, 1, 0, 1, 1.7), (1, 1, 1, 2, 4, 3, 1, 1, 1, 0.3)]


@pytest.mark.parametrize("N,H,W,G,Cg,K,s,p,d,osc", SQUARE)
def test_closed_forms_equal_autograd_through_the_oracle(N, H, W, G, Cg, K, s, p, d, osc):
    x, off, m, gy = _maps(N, H, W, G, Cg, K, K, s, s, p, p, d, d, seed=H * 10 + W)
    if H == 1:
        off = off * 0.2          # (a 1 x 1 map: keep some taps on it)
    a, b, c = (t.clone().requires_grad_(True) for t in (x, off, m))
    yo = so.dcnv3_core(a, b, c, G, Cg, K, s, p, d, osc)
    yo.backward(gy)
    y, dx, doff, dm = dcn_ref.dcnv3(x, off, m, gy, G, Cg, K, K, s, s, p, p, d, d, osc)
    assert y.dtype == torch.float64 and y.abs().max().item() > 0 and dx.abs().max().item() > 0
    assert _close(y, yo.detach()) and _close(dx, a.grad) and _close(doff, b.grad) and _close(dm, c.grad)


def _grid_sample_core(x, off, m, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw, osc):
    """the formula of SURVEY C.5 through F.grid_sample on the padded map, one tap at a time (align_corners=True: pixel p of a
    row of S pixels sits at the normalised coordinate 2 p / (S - 1) - 1)"""
    N, H, W, C = x.shape
    Ho, Wo = dcn_ref.out_hw(H, W, Kh, Kw, sh, sw, ph, pw, dh, dw)
    Hp, Wp = H + 2 * ph, W + 2 * pw
    xp = F.pad(x, [0, 0, pw, pw, ph, ph]).view(N, Hp, Wp, G, Cg).permute(0, 3, 4, 1, 2).reshape(N * G, Cg, Hp, Wp)
    o = off.view(N, Ho, Wo, G, Kh * Kw, 2)
    mm = m.view(N, Ho, Wo, G, Kh * Kw)
    wo = torch.arange(Wo, dtype=x.dtype).view(1, 1, Wo, 1)
    ho = torch.arange(Ho, dtype=x.dtype).view(1, Ho, 1, 1)
    y = 0
    for iw in range(Kw):
        for jh in range(Kh):
            k = iw * Kh + jh
            px = wo * sw + (dw * (Kw - 1)) // 2 + (iw - (Kw - 1) // 2) * dw * osc + o[..., k, 0] * osc          # [N, Ho, Wo, G]
            py = ho * sh + (dh * (Kh - 1)) // 2 + (jh - (Kh - 1) // 2) * dh * osc + o[..., k, 1] * osc
            grid = torch.stack((2 * px / (Wp - 1) - 1, 2 * py / (Hp - 1) - 1), dim=-1).permute(0, 3, 1, 2, 4).reshape(N * G, Ho, Wo, 2)
            v = F.grid_sample(xp, grid, mode="bilinear", padding_mode="zeros", align_corners=True)          # [N*G, Cg, Ho, Wo]
            y = y + v.view(N, G, Cg, Ho, Wo).permute(0, 3, 4, 1, 2) * mm[..., k].unsqueeze(-1)
    return y.reshape(N, Ho, Wo, C)


@pytest.mark.parametrize("geo", [(2, 6, 7, 2, 3, 3, 1, 1, 2, 1, 0, 1, 1, 1.0), (1, 7, 5, 2, 4, 1, 3, 2, 1, 0, 2, 1, 2, 1.5),
                                 (1, 8, 6, 1, 2, 2, 3, 1, 1, 1, 1, 1, 1, 0.5)])
def test_closed_forms_equal_autograd_through_grid_sample_with_a_window_that_is_not_square(geo):
    """Kh != Kw, sh != sw, ph != pw, dh != dw: a reference that exchanged the two window sides, or the roles of h and w in the
    tap order k = i_w Kh + j_h, would read other offsets and fail here.  (randn offsets: no position is an integer, where the
    normalisation of grid_sample could fall on the other side of the floor.)"""
    N, H, W, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw, osc = geo
    x, off, m, gy = _maps(N, H, W, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw, seed=7 + Kh)
    a, b, c = (t.clone().requires_grad_(True) for t in (x, off, m))
    yo = _grid_sample_core(a, b, c, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw, osc)
    yo.backward(gy)
    y, dx, doff, dm = dcn_ref.dcnv3(x, off, m, gy, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw, osc)
    assert y.abs().max().item() > 0 and dx.abs().max().item() > 0
    assert _close(y, yo.detach(), 1e-10) and _close(dx, a.grad, 1e-10) and _close(doff, b.grad, 1e-10) and _close(dm, c.grad, 1e-10)


def _term_loop(x, off, m, gy, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw, osc):
    """A and T of every entry by a loop over single terms, in Python floats"""
    N, H, W, C = x.shape
    Ho, Wo = dcn_ref.out_hw(H, W, Kh, Kw, sh, sw, ph, pw, dh, dw)
    P = Kh * Kw
    A = [torch.zeros(N, Ho, Wo, C, dtype=torch.float64), torch.zeros(N, H, W, C, dtype=torch.float64),
         torch.zeros(N, Ho, Wo, G * P * 2, dtype=torch.float64), torch.zeros(N, Ho, Wo, G * P, dtype=torch.float64)]
    T = [torch.zeros_like(a) for a in A]
    for n in range(N):
        for ho in range(Ho):
            for wo in range(Wo):
                for g in range(G):
                    for iw in range(Kw):
                        for jh in range(Kh):
                            k = iw * Kh + jh
                            ox, oy = (off[n, ho, wo, (g * P + k) * 2 + i].item() for i in (0, 1))
                            px = wo * sw + (dw * (Kw - 1)) // 2 + (iw - (Kw - 1) // 2) * dw * osc + ox * osc
                            py = ho * sh + (dh * (Kh - 1)) // 2 + (jh - (Kh - 1) // 2) * dh * osc + oy * osc
                            x0, y0 = math.floor(px), math.floor(py)
                            lx, ly = px - x0, py - y0
                            mk = abs(m[n, ho, wo, g * P + k].item())
                            for c in range(Cg):
                                ch = g * Cg + c
                                gv = abs(gy[n, ho, wo, ch].item())
                                for ey in (0, 1):
                                    for ex in (0, 1):
                                        yy, xx = y0 + ey - ph, x0 + ex - pw
                                        inside = 0 <= yy < H and 0 <= xx < W
                                        v = abs(x[n, yy, xx, ch].item()) if inside else 0.0
                                        wq = (ly if ey else 1 - ly) * (lx if ex else 1 - lx)
                                        A[0][n, ho, wo, ch] += mk * wq * v
                                        T[0][n, ho, wo, ch] += 1
                                        A[3][n, ho, wo, g * P + k] += gv * wq * v
                                        T[3][n, ho, wo, g * P + k] += 1
                                        A[2][n, ho, wo, (g * P + k) * 2] += osc * mk * gv * (ly if ey else 1 - ly) * v
                                        A[2][n, ho, wo, (g * P + k) * 2 + 1] += osc * mk * gv * (lx if ex else 1 - lx) * v
                                        T[2][n, ho, wo, (g * P + k) * 2] += 1
                                        T[2][n, ho, wo, (g * P + k) * 2 + 1] += 1
                                        if inside:
                                            A[1][n, yy, xx, ch] += gv * mk * wq
                                            T[1][n, yy, xx, ch] += 1
    return A, T


def test_abs_sums_are_the_same_operations_on_absolute_values():
    geo = (1, 3, 4, 2, 2, 3, 2, 1, 2, 1, 0, 1, 1)
    x, off, m, gy = _maps(*geo, seed=3)
    A, T = dcn_ref.abs_sums(x, off, m, gy, *geo[3:], 1.5)
    # the bilinear weights are not negative: y, dx and dmask of the absolute maps ARE their sums of absolute terms
    y, dx, _, dm = dcn_ref.dcnv3(x.abs(), off, m.abs(), gy.abs(), *geo[3:], 1.5)
    assert torch.equal(A[0], y) and torch.equal(A[1], dx) and torch.equal(A[3], dm)
    got = dcn_ref.dcnv3(x, off, m, gy, *geo[3:], 1.5)
    for a, r in zip(A, got):
        assert a.dtype == torch.float64 and a.shape == r.shape and bool((r.abs() <= a * (1 + 1e-12) + 1e-300).all())
    assert bool((A[2] > got[2].abs()).any())          # a difference of corner values counts as two terms
    wantA, wantT = _term_loop(x, off, m, gy, *geo[3:], 1.5)
    for i in range(4):
        assert _close(A[i], wantA[i]), i
        assert torch.equal(T[i], wantT[i]), i
    assert T[1].min().item() == 0 and T[1].max().item() > 4          # pixels no corner lands on, pixels many land on


def test_positions_in_fp32_round_where_fp64_does_not():
    """dtype = fp32 really evaluates in fp32: with offsets of 24 significant bits the two positions differ"""
    geo = (1, 5, 5, 1, 1, 3, 3, 1, 1, 1, 1, 1, 1)
    _, off, _, _ = _maps(*geo, seed=1)
    off = off.float().double()
    a = dcn_ref.positions(off, 5, 5, 1, 3, 3, 1, 1, 1, 1, 1, 1, 1.5, torch.float32)[0]
    b = dcn_ref.positions(off, 5, 5, 1, 3, 3, 1, 1, 1, 1, 1, 1, 1.5, torch.float64)[0]
    assert a.dtype == torch.float32 and not torch.equal(a.double(), b)
    off = torch.round(off * 1024) / 1024
    a, b = (dcn_ref.positions(off, 5, 5, 1, 3, 3, 1, 1, 1, 1, 1, 1, 1.5, t)[0] for t in (torch.float32, torch.float64))
    assert torch.equal(a.double(), b)
    y32 = dcn_ref.dcnv3(*_maps(*geo, seed=1), 1, 1, 3, 3, 1, 1, 1, 1, 1, 1, 1.0, dtype=torch.float32)[0]
    assert y32.dtype == torch.float32


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_all_four_results_against_the_reference_vectors(golden, tag):
    """tolerances of test_oracle_golden.py::test_dcnv3_core_vs_reference (the reference builds its grid in normalised fp32)"""
    g = golden("dcnv3_core.npz")
    N, H, W, G, Cg, K, s, p, d = (int(v) for v in g[f"{tag}_geom"])
    x, off, m, gy = (torch.from_numpy(np.asarray(g[f"{tag}_{k}"])) for k in ("x", "offset", "mask", "gy"))
    y, dx, doff, dm = dcn_ref.dcnv3(x, off, m, gy, G, Cg, K, K, s, s, p, p, d, d, float(g[f"{tag}_offset_scale"]))

    def close(a, b, rel):
        b = torch.from_numpy(np.asarray(b)).double()
        return (a - b).abs().max().item() <= rel * b.abs().max().item()
    assert close(y, g[f"{tag}_y"], 2e-4)
    assert close(dx, g[f"{tag}_gx"], 2e-4)
    assert close(doff, g[f"{tag}_goffset"], 2e-3)
    assert close(dm, g[f"{tag}_gmask"], 2e-4)
