"""tests/attn_ref.py, the fp64 reference the GPU tests of the attention core compare with (tests/test_gpu_attention.py), checked on the
CPU so that it cannot be wrong unnoticed: the closed-form gradients against torch.autograd of the reference expression written the
way the reference writes it (per-head [N, d] matrices, sdtv2.py:335-339), the fused variant against the oracle's neuron
(oracle.s2f_oracle.lif_step, whose backward is _QuantSTE), the mask packing against a per-element loop."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref  # noqa: E402
from oracle import s2f_oracle as so  # noqa: E402

SHAPES = [(2, 3, 5, 7, 11), (1, 2, 45, 12, 20), (3, 1, 1, 4, 4)]


def _draw(TB, heads, d, Nq, Nk, seed):
    g = torch.Generator().manual_seed(seed)
    C = heads * d
    q, k, v = (torch.randn(TB, C, n, generator=g, dtype=torch.float64) for n in (Nq, Nk, Nk))
    go = torch.randn(TB, C, Nq, generator=g, dtype=torch.float64)
    return q, k, v, go


def _reference_expression(q, k, v, heads, scale):
    """x = (q @ (k^T @ v)) * scale on [TB, heads, N, d] operands, back to [TB, C, N]: the reference's own lines"""
    TB, C, Nq = q.shape
    d = C // heads

    def hv(t):
        return t.view(TB, heads, d, -1).transpose(2, 3)
    kv = hv(k).transpose(-2, -1) @ hv(v)
    return ((hv(q) @ kv) * scale).transpose(2, 3).reshape(TB, C, Nq), kv


@pytest.mark.parametrize("TB,heads,d,Nq,Nk", SHAPES)
def test_closed_forms_are_autograd_of_the_reference_expression(TB, heads, d, Nq, Nk):
    q, k, v, go = _draw(TB, heads, d, Nq, Nk, 1)
    scale = 0.37
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    o_ref, kv_ref = _reference_expression(ql, kl, vl, heads, scale)
    kv_ref.retain_grad()
    o_ref.backward(go)
    o, kv = attn_ref.forward(q, k, v, heads, scale)
    gq, gk, gv, gkv = attn_ref.backward(q, k, v, go, heads, scale)
    for got, want in ((o, o_ref), (kv, kv_ref), (gq, ql.grad), (gk, kl.grad), (gv, vl.grad), (gkv, kv_ref.grad)):
        assert got.shape == want.shape and got.dtype == torch.float64
        assert (got - want.detach()).abs().max().item() <= 1e-13 * want.abs().max().item()


def test_closed_forms_are_exact_on_small_integers():
    """every sum is an integer far below 2^53: the two ways of writing the expression agree bit for bit"""
    TB, heads, d, Nq, Nk = 2, 2, 5, 8, 12
    g = torch.Generator().manual_seed(2)
    C = heads * d
    q, k, v = (torch.randint(0, 9, (TB, C, n), generator=g).double() for n in (Nq, Nk, Nk))
    go = torch.randint(-4, 5, (TB, C, Nq), generator=g).double()
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    o_ref, _ = _reference_expression(ql, kl, vl, heads, 0.25)
    o_ref.backward(go)
    o, _ = attn_ref.forward(q, k, v, heads, 0.25)
    gq, gk, gv, _ = attn_ref.backward(q, k, v, go, heads, 0.25)
    assert torch.equal(o, o_ref.detach()) and torch.equal(gq, ql.grad) and torch.equal(gk, kl.grad) and torch.equal(gv, vl.grad)
    # ... and the sums of absolute terms bound every entry
    a = attn_ref.abs_sums(q, k, v, go, heads)
    gq1, gk1, gv1, gkv1 = attn_ref.backward(q, k, v, go, heads, 1.0)
    for name, x in (("gq", gq1), ("gk", gk1), ("gv", gv1), ("gkv", gkv1)):
        assert bool((x.abs() <= a[name]).all()) and bool((x.abs() < a[name]).any()), name


@pytest.mark.parametrize("TB,heads,d,Nq,Nk", SHAPES)
def test_fused_variant_is_autograd_through_the_oracle_neuron(TB, heads, d, Nq, Nk):
    """y = lif_step(o)[0] from a reset membrane: spikes, counts and the three gradients -- with o on, below and above the edges 0 and D"""
    q, k, v, g = _draw(TB, heads, d, Nq, Nk, 3)
    scale = 8.0 / max(1.0, attn_ref.forward(q, k, v, heads, 1.0)[0].abs().max().item()) * 1.5
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    o_ref, _ = _reference_expression(ql, kl, vl, heads, scale)
    y_ref, _, s_ref = so.lif_step(o_ref, None, D=8, vth=1.0)
    y_ref.backward(g)
    o, _ = attn_ref.forward(q, k, v, heads, scale)
    inr = attn_ref.in_range(o)
    assert bool((o < 0).any()) and bool((o > 8).any()) and bool(inr.any())
    y, counts = attn_ref.neuron(o)
    assert torch.equal(y, y_ref.detach()) and torch.equal(counts, s_ref.detach())
    assert attn_ref.firing(counts) == (int(s_ref.sum().item()), int((s_ref != 0).sum().item()))
    gq, gk, gv, _ = attn_ref.backward(q, k, v, attn_ref.fused_grad(o, g), heads, scale)
    for got, want in ((gq, ql.grad), (gk, kl.grad), (gv, vl.grad)):
        assert (got - want).abs().max().item() <= 1e-13 * want.abs().max().item()


def test_in_range_includes_both_ends_as_the_oracle_does():
    o = torch.tensor([-1e-300, -0.0, 0.0, 0.5, 2.5, 3.5, 8.0, 8.0 + 2e-15, 9.0], dtype=torch.float64, requires_grad=True)
    y, _, s = so.lif_step(o, None, D=8, vth=1.0)
    y.backward(torch.full_like(o, 3.0))
    assert attn_ref.in_range(o.detach()).tolist() == [False, True, True, True, True, True, True, False, False]
    assert torch.equal(attn_ref.fused_grad(o.detach(), torch.full_like(o, 3.0)), o.grad)
    assert attn_ref.neuron(o.detach())[1].tolist() == s.tolist() == [0, 0, 0, 0, 2, 4, 8, 8, 8]          # halves go to even


@pytest.mark.parametrize("n", [1, 4, 255, 256, 257, 1027])
def test_mask_packing_against_a_per_element_loop(n):
    g = torch.Generator().manual_seed(n)
    bits = torch.rand(n, generator=g) < 0.5
    if n >= 256:
        bits[252:256] = True              # bit 63 of all four words of tile 0: the sign bit of an int64 word
    words = attn_ref.pack_mask(bits)
    assert words.dtype == torch.int64 and words.numel() == ((n + 255) >> 8) * 4
    want = [0] * words.numel()
    for e in range(n):
        if bool(bits[e]):
            want[(e >> 8) * 4 + (e & 3)] |= 1 << ((e & 255) >> 2)
    assert [int(w) & (2 ** 64 - 1) for w in words.tolist()] == want
    # the shape of the tensor does not matter: element e is the index in the contiguous tensor
    if n % 4 == 0:
        assert torch.equal(attn_ref.pack_mask(bits.reshape(2, -1, 2)), words)
