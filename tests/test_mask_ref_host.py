"""tests/mask_ref.py against what it restates, on the host: the closed-form gradients against autograd of the reference's own two-step
expression (the mask_feature 1x1 convolution, then einsum('tbqc,tbchw->tbqhw') reduced over t) in fp64, and abs_sums against a
per-element loop."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ref  # noqa: E402


def _draw(T, B, Q, Co, C, HW, seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return r(T, B, Q, Co), r(T, B, C, HW), r(Co, C), (r(Co) if bias else None), r(B, Q, HW)


def _close(a, b):
    return torch.allclose(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("with_bias", [True, False])
def test_folded_closed_forms_equal_autograd_of_the_two_steps(with_bias):
    T, B, Q, Co, C, HW = 3, 2, 5, 4, 6, 7
    E, S, W, bias, g = _draw(T, B, Q, Co, C, HW, 1, with_bias)
    scale = 0.37
    leaves = [t.clone().requires_grad_(True) for t in (E, S, W)] + ([bias.clone().requires_grad_(True)] if with_bias else [])
    e, s, w = leaves[:3]
    mf = torch.nn.functional.conv2d(s.reshape(T * B, C, HW, 1), w.reshape(Co, C, 1, 1), leaves[3] if with_bias else None)
    mf = mf.reshape(T, B, Co, HW)
    out = torch.einsum("tbqc,tbcn->tbqn", e, mf).sum(0) * scale
    out.backward(g)
    got, EW, rowb = mask_ref.forward_folded(E, S, W, bias, scale)
    assert _close(got, out.detach())
    assert _close(EW, torch.einsum("tbqo,oc->tbqc", E, W)) and (rowb is None) == (not with_bias)
    r = mask_ref.backward_folded(E, S, W, bias, g, scale)
    assert _close(r["dE"], e.grad) and _close(r["dS"], s.grad) and _close(r["dW"], w.grad)
    assert _close(r["H"], torch.einsum("bqn,tbcn->tbqc", g, S)) and _close(r["rs"], g.sum(-1))
    if with_bias:
        assert _close(r["dbias"], leaves[3].grad)
        assert _close(got, scale * (torch.einsum("tbqc,tbcn->bqn", EW, S) + rowb.unsqueeze(-1)))
    else:
        assert r["dbias"] is None
    # with scale = 1 / T the sum over t is the reference's mean
    assert _close(mask_ref.forward_folded(E, S, W, bias, 1.0 / T)[0], torch.einsum("tbqc,tbcn->tbqn", E, mf.detach()).mean(0))


def test_unfolded_class_mask_and_linear_equal_autograd():
    T, B, Q, C, HW = 2, 3, 5, 4, 6
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    E, MF, go = r(T, B, Q, C), r(T, B, C, HW), r(B, Q, HW)
    e, mf = E.clone().requires_grad_(True), MF.clone().requires_grad_(True)
    out = torch.einsum("tbqc,tbcn->tbqn", e, mf).sum(0) * 0.25
    out.backward(go)
    assert _close(mask_ref.forward_unfolded(E, MF, 0.25), out.detach())
    dE, dMF = mask_ref.backward_unfolded(E, MF, go, 0.25)
    assert _close(dE, e.grad) and _close(dMF, mf.grad)
    cls, mp = r(B, Q, 7), r(B, Q, 3, 5)
    want = torch.stack([cls[b].t() @ mp[b].reshape(Q, 15) for b in range(B)]).reshape(B, 7, 3, 5)
    assert _close(mask_ref.class_mask(cls, mp), want)
    x, w, b, gy = r(9, 6), r(5, 6), r(5), r(9, 5)
    xl, wl, bl = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = torch.nn.functional.linear(xl, wl, bl)
    y.backward(gy)
    got = mask_ref.linear(x, w, b, gy)
    assert all(_close(a, c) for a, c in zip(got, (y.detach(), xl.grad, wl.grad, bl.grad)))
    assert mask_ref.linear(x, w, None, gy)[3] is None and _close(mask_ref.linear(x, w, None, gy)[0], x @ w.t())
    # the fp32 evaluation is the same association in the narrower type
    assert mask_ref.forward_unfolded(E, MF, 0.25, torch.float32).dtype == torch.float32


def test_abs_sums_equal_a_per_element_loop():
    T, B, Q, Co, C, HW = 2, 2, 3, 2, 3, 4
    E, S, W, bias, g = _draw(T, B, Q, Co, C, HW, 3)
    a = mask_ref.abs_sums(E, S, W, bias, g)
    E, S, W, bias, g = (t.abs() for t in (E, S, W, bias, g))
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    EW, H, rs, rowb = z(T, B, Q, C), z(T, B, Q, C), z(B, Q), z(B, Q)
    for t in range(T):
        for b in range(B):
            for q in range(Q):
                for c in range(C):
                    EW[t, b, q, c] = sum(E[t, b, q, o] * W[o, c] for o in range(Co))
                    H[t, b, q, c] = sum(g[b, q, n] * S[t, b, c, n] for n in range(HW))
    for b in range(B):
        for q in range(Q):
            rs[b, q] = sum(g[b, q, n] for n in range(HW))
            rowb[b, q] = sum(E[t, b, q, o] * bias[o] for t in range(T) for o in range(Co))
    out, dS, dE, dW, dbias = z(B, Q, HW), z(T, B, C, HW), z(T, B, Q, Co), z(Co, C), z(Co)
    for b in range(B):
        for q in range(Q):
            for n in range(HW):
                out[b, q, n] = sum(EW[t, b, q, c] * S[t, b, c, n] for t in range(T) for c in range(C)) + rowb[b, q]
    for t in range(T):
        for b in range(B):
            for c in range(C):
                for n in range(HW):
                    dS[t, b, c, n] = sum(EW[t, b, q, c] * g[b, q, n] for q in range(Q))
            for q in range(Q):
                for o in range(Co):
                    dE[t, b, q, o] = sum(H[t, b, q, c] * W[o, c] for c in range(C)) + rs[b, q] * bias[o]
    for o in range(Co):
        dbias[o] = sum(E[t, b, q, o] * rs[b, q] for t in range(T) for b in range(B) for q in range(Q))
        for c in range(C):
            dW[o, c] = sum(E[t, b, q, o] * H[t, b, q, c] for t in range(T) for b in range(B) for q in range(Q))
    want = {"EW": EW, "H": H, "rs": rs, "rowb": rowb, "out": out, "dS": dS, "dE": dE, "dW": dW, "dbias": dbias}
    assert set(a) == set(want)
    for k, v in want.items():
        assert _close(a[k], v), k
    # without a bias its terms vanish
    nb = mask_ref.abs_sums(E, S, W, None, g)
    assert nb["rowb"] is None and nb["dbias"] is None and _close(nb["out"], out - rowb.unsqueeze(-1))
    u = mask_ref.abs_sums_unfolded(-EW, S, g)
    assert _close(u["out"], out - rowb.unsqueeze(-1)) and _close(u["dMF"], dS) and _close(u["dE"], torch.einsum("bqn,tbcn->tbqc", g, S))
