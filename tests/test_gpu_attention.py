"""Every route of the attention core's forward and backward (spike2former_amd/csrc/sdsa.hip) against the fp64 restatement of
tests/attn_ref.py, at the smallest shapes that reach it.  Each case is one row whose id names the route; the test asserts from
the shape the inequality that puts the row there (nothing else of the dispatcher is restated) and builds its inputs as the product
does: fp32 tensors for _SDSA, bf16 Spikes with autograd handles for the bf16 entry points.

  exact rows      q, k, v sparse multiples of 1/8, output gradient integers in [-4, 4], scale a power of two; each row first asserts on
                  its own draw (fp64) that every sum of ABSOLUTE terms behind kv, o, gq, gkv, gk, gv is below 2^24 granules, so the
                  order of the fp32 additions (four waves, split-N atomics, matrix-core steps) cannot matter; o, gq, gk, gv must then
                  EQUAL the fp64 values.  The fused rows (neuron in the epilogue, straight-through mask in the backward's loaders)
                  compare with the fp64 in-range mask of attn_ref and also pin spikes, firing counters and the mask words.
  three terms     integer gradients are exact in the `hi` term of the spike x general matrix-core kernel alone; this draw (three
                  non-zero tokens per row of q, go on multiples of 2^-20) needs hi + mid + lo and is still exact: gkv bit for bit.
  general rows    randn gradients (and randn q, k, v on the fp32 route): e(X) = max|X - X64| / max|X64| of the kernel against the
                  same figure of a plain fp32 CPU evaluation of the same association, e_kernel <= 8 e_cpu + 2^-22 (both add the same
                  addends in fp32; 8 for the order -- four waves, split-N atomics, contracted multiply-adds; the floor for outputs the
                  CPU happens to get exactly).

Measured on the MI355X, e_kernel / e_cpu (every e between 4.8e-08 and 3.4e-07, i.e. far above the floor):
  fp32 VALU            (2, 2, 45, 100, 300)    o 0.90   gq 0.95   gk 1.00   gv 1.00
  bf16 mfma<2> + sg<2> (1, 2, 45, 264, 520)    o 1.00   gq 1.00   gk 0.89   gv 0.63
  bf16 VALU            (1, 2, 45, 100, 1028)   o 1.00   gq 1.00   gk 1.00   gv 1.00
  bf16 fused, sg<2>    (1, 2, 64, 512, =)      (spikes, counters, mask equal)   gq 1.00   gk 1.08   gv 1.04

Not reached here: the VALU spike x general kernel WITH the straight-through mask, which only the process-wide switch
S2F_SDSA_OUTER_SG_VALU selects (the masked backward needs N % 256 == 0, where the matrix-core form is always taken).  Nor is
apply_kernel's `loaded at use` branch for bf16 rows: no entry point hands it a masked or ragged bf16 operand; the masked operand of
the fused backward is the fp32 gradient."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("o", "gq", "gk", "gv")


@pytest.fixture(scope="module")
def ops():
    from spike2former_amd import ops
    return ops


def cdiv(a, b):
    return -(-a // b)


def four_wave(TB, heads, N):
    return TB * heads * cdiv(N, 256) > 1024


# -------------------------------------------------------------------------------------------------------------- draws and runners
def draw_spikes(g, TB, C, N):
    """sparse multiples of 1/8 in [0, 1], fp64; every channel and every token fires at a rate of its own (as in real spike maps), so
    the pre-activations behind a fused neuron spread over more than a factor of two along both axes"""
    vals = torch.randint(0, 9, (TB, C, N), generator=g).double() / 8
    rate = torch.rand(TB, C, 1, generator=g).sqrt() * torch.rand(TB, 1, N, generator=g).sqrt()
    return vals * (torch.rand(TB, C, N, generator=g) < rate)


def draw_exact(TB, heads, d, Nq, Nk, seed):
    g = torch.Generator().manual_seed(seed)
    C = heads * d
    q, k, v = draw_spikes(g, TB, C, Nq), draw_spikes(g, TB, C, Nk), draw_spikes(g, TB, C, Nk)
    go = torch.randint(-4, 5, (TB, C, Nq), generator=g).double()
    return q, k, v, go


def assert_sums_exact(q, k, v, go, heads, go_den=1):
    """q, k, v on multiples of 1/8, go on multiples of 1/go_den: granules 1/64 (kv), 1/512 (o), 1/(64 go_den) (gq, gk, gv),
    1/(8 go_den) (gkv); a power-of-two scale moves exponents only"""
    sums = attn_ref.abs_sums(q, k, v, go, heads)
    per_unit = {"kv": 64, "o": 512, "gq": 64 * go_den, "gkv": 8 * go_den, "gk": 64 * go_den, "gv": 64 * go_den}
    for name, x in sums.items():
        assert x.max().item() * per_unit[name] < 2 ** 24, name


def to_spikes(ops, t):
    """fp64 map of multiples of 1/8 -> (fp32 leaf, bf16 Spikes with its autograd handle): Q_IFNode(8 (k / 8)) = k / 8, and
    d Q_IFNode(8 src) / d src = 8 (1 / 8) = 1 on [0, 1], so src.grad is the gradient of the spike map, bit for bit"""
    src = t.float().cuda().requires_grad_(True)
    s, _ = ops.lif(src * 8.0, None, keep_v=False, spikes=True)
    assert isinstance(s, ops.Spikes) and s.tok is not None and s.data.dtype == torch.bfloat16
    assert torch.equal(s.data.float(), src.detach())
    return src, s


def run_fp32(ops, q, k, v, go, heads, scale):
    qc, kc, vc = (t.float().cuda().requires_grad_(True) for t in (q, k, v))
    o = ops.sdsa(qc, kc, vc, heads, scale)
    o.backward(go.float().cuda())
    return o.detach(), qc.grad, kc.grad, vc.grad


def run_bf16(ops, q, k, v, go, heads, scale, packed, lif=None):
    """-> (o or the neuron's Spikes, gq, gk, gv, the mask words the fused forward saved for its backward or None)"""
    C = q.shape[1]
    if packed:
        src, s = to_spikes(ops, torch.cat([q, k, v], 1))
        out = ops.sdsa_packed(s, heads, scale, lif=lif)
    else:
        (sq, q_), (sk, k_), (sv, v_) = (to_spikes(ops, t) for t in (q, k, v))
        out = ops.sdsa(q_, k_, v_, heads, scale, lif=lif)
    handle = out.tok if lif is not None else out
    node = handle.grad_fn
    assert type(node).__name__.startswith("_SDSASpikes"), type(node).__name__            # the bf16 entry points, not _SDSA
    saved_mask = node.saved_tensors[4] if lif is not None else None                      # (q, k, v, kv, mask): gone after backward
    (out.float() if lif is not None else out).backward(go.float().cuda())
    if packed:
        assert src.grad.shape == (q.shape[0], 3 * C, q.shape[2])
        grads = (src.grad[:, :C], src.grad[:, C:2 * C], src.grad[:, 2 * C:])
    else:
        grads = (sq.grad, sk.grad, sv.grad)
    return (out,) + grads + (saved_mask,)


def assert_equal64(got, want, names=NAMES):
    for name, a, b in zip(names, got, want):
        assert a.dtype == torch.float32 and a.shape == b.shape, name
        assert torch.equal(a.detach().cpu().double(), b), name


def reference(q, k, v, go, heads, scale, dtype=torch.float64):
    o, _ = attn_ref.forward(q, k, v, heads, scale, dtype)
    gq, gk, gv, _ = attn_ref.backward(q, k, v, go, heads, scale, dtype)
    return o, gq, gk, gv


# -------------------------------------------------------------------------------------------------------------- exact rows: fp32
def _apply_rows(d):
    return {8: 4, 24: 8, 45: 12, 64: 16}[d]


FP32_ROWS = [
    pytest.param((1, 2, 45, 7, 13), lambda TB, h, d, Nq, Nk: Nq % 4 != 0 and Nk % 4 != 0 and d % 2 == 1 and Nq // 2 < 64 and Nk // 2 < 64,
                 id="valu-scalar-loaders-odd-d-no-split"),
    pytest.param((1, 2, 64, 132, 260), lambda TB, h, d, Nq, Nk: Nq % 4 == 0 and Nk % 4 == 0 and Nq // 2 >= 64 and Nk // 2 >= 64
                 and TB * h < 2048 and ((d + 1) // 2) ** 2 > 3 * 256, id="valu-split-atomics-d64-four-microtiles"),
    *[pytest.param((65, 16, d, 12, 20), lambda TB, h, d, Nq, Nk: four_wave(TB, h, Nq) and four_wave(TB, h, Nk)
                   and 4 * (_apply_rows(d) - 4) < d <= 4 * _apply_rows(d), id=f"apply-four-waves-jc{_apply_rows(d)}") for d in (8, 24, 45, 64)],
    pytest.param((1, 2, 45, 300, 100), lambda TB, h, d, Nq, Nk: not four_wave(TB, h, Nq) and not four_wave(TB, h, Nk) and d > 32,
                 id="apply-eight-waves-jc8"),
]


@pytest.mark.parametrize("shape,on_route", FP32_ROWS)
def test_fp32_route_equals_fp64(ops, shape, on_route):
    TB, heads, d, Nq, Nk = shape
    assert on_route(*shape)
    q, k, v, go = draw_exact(*shape, seed=d * 1000 + Nq)
    assert_sums_exact(q, k, v, go, heads)
    scale = 0.125
    assert_equal64(run_fp32(ops, q, k, v, go, heads, scale), reference(q, k, v, go, heads, scale))


# -------------------------------------------------------------------------------------------------------------- exact rows: bf16
def _mfma(N):
    return N % 8 == 0


def _ragged(N):
    return N % 16 == 8          # the last 16-column step of the matrix-core kernels is half filled


BF16_ROWS = [
    pytest.param((2, 8, 32, 100, 36), False, lambda TB, h, d, Nq, Nk: Nq % 8 == 4 and Nk % 8 == 4, id="valu-spike-spike-and-spike-general"),
    pytest.param((1, 2, 45, 100, 1028), False, lambda TB, h, d, Nq, Nk: Nq % 8 == 4 and Nk % 8 == 4 and Nk // 2 >= 64,
                 id="valu-spike-general-and-split-spike-spike"),
    pytest.param((2, 2, 32, 136, 264), False, lambda TB, h, d, Nq, Nk: _mfma(Nq) and _mfma(Nk) and d <= 32 and _ragged(Nq) and _ragged(Nk)
                 and Nq != Nk and Nq // 128 < 2 and Nk // 256 < 2, id="mfma1-and-sg1-ragged-last-step"),
    *[pytest.param((1, h, d, 264, 520), False, lambda TB, h, d, Nq, Nk: _mfma(Nq) and _mfma(Nk) and d > 32 and Nq // 128 >= 2
                   and Nk // 256 >= 2 and _ragged(Nq) and _ragged(Nk), id=f"mfma2-and-sg2-split-ragged-second-chunk-d{d}")
      for h, d in ((2, 45), (1, 64))],
    pytest.param((2, 2, 45, 264, 264), True, lambda TB, h, d, Nq, Nk: _mfma(Nq) and _ragged(Nq) and d > 32 and (3 * h * d * Nq) % 8 == 0,
                 id="packed-one-gradient-ragged"),
    pytest.param((65, 16, 45, 8, 8), False, lambda TB, h, d, Nq, Nk: four_wave(TB, h, Nq) and d > 32 and _mfma(Nq),
                 id="apply-four-waves-bf16-rows-d45"),
]


@pytest.mark.parametrize("shape,packed,on_route", BF16_ROWS)
def test_bf16_route_equals_fp64(ops, shape, packed, on_route):
    TB, heads, d, Nq, Nk = shape
    assert on_route(*shape)
    q, k, v, go = draw_exact(*shape, seed=d * 1000 + Nk)
    assert_sums_exact(q, k, v, go, heads)
    scale = 0.125
    got = run_bf16(ops, q, k, v, go, heads, scale, packed)
    assert_equal64(got[:4], reference(q, k, v, go, heads, scale))


FUSED_ROWS = [
    pytest.param((1, 2, 45, 256), False, lambda TB, h, d, N: d > 32 and N % 256 == 0 and N // 128 == 2, id="unpacked-dt2-sg-split2"),
    pytest.param((1, 2, 64, 512), False, lambda TB, h, d, N: d > 32 and N % 256 == 0 and N // 128 == 4, id="unpacked-dt2-sg-split4"),
    pytest.param((2, 4, 9, 256), True, lambda TB, h, d, N: 8 < d <= 32 and N % 256 == 0, id="packed-d9"),
    pytest.param((1, 2, 33, 256), True, lambda TB, h, d, N: d > 32 and N % 256 == 0, id="packed-d33"),
    pytest.param((65, 16, 45, 256), False, lambda TB, h, d, N: four_wave(TB, h, N) and d > 32 and N % 256 == 0,
                 id="apply-four-waves-bf16-rows-masked-gradient-d45"),
]


def fused_scale(q, k, v, heads):
    """a power of two that puts about half of the non-zero pre-activations above D = 8"""
    o1, _ = attn_ref.forward(q, k, v, heads, 1.0)
    med = o1[o1 > 0].median().item()
    return 2.0 ** round(torch.log2(torch.tensor(8.0 / med)).item())


def run_fused(ops, q, k, v, g, heads, scale, packed):
    """-> (spike map fp32, (sum of counts, non-zero counts), mask words, gq, gk, gv) of the product path"""
    from spike2former_amd.neuron import Q_IFNode
    lif = Q_IFNode()
    lif.keep_membrane = False
    lif.stats = ops.new_stats("cuda")
    y, gq, gk, gv, mask = run_bf16(ops, q, k, v, g, heads, scale, packed, lif=lif)
    assert isinstance(y, ops.Spikes) and y.data.dtype == torch.bfloat16
    assert mask is not None          # the fused kernel ran (core + neuron keeps no mask here)
    return y.data.float(), tuple(ops.read_stats(lif.stats).tolist()), mask, gq, gk, gv


@pytest.mark.parametrize("shape,packed,on_route", FUSED_ROWS)
def test_fused_route_equals_fp64(ops, shape, packed, on_route):
    TB, heads, d, N = shape
    assert on_route(*shape)
    q, k, v, g = draw_exact(TB, heads, d, N, N, seed=d * 1000 + N)
    scale = fused_scale(q, k, v, heads)
    o64, _ = attn_ref.forward(q, k, v, heads, scale)
    inr = attn_ref.in_range(o64)
    for tile in (inr.reshape(-1)[:256], inr.reshape(-1)[-256:]):            # a condition on the draw, not a measurement
        assert bool(tile.any()) and not bool(tile.all())
    go = attn_ref.fused_grad(o64, g)
    assert_sums_exact(q, k, v, go, heads, go_den=8)
    y64, counts = attn_ref.neuron(o64)
    y, stats, mask, gq, gk, gv = run_fused(ops, q, k, v, g, heads, scale, packed)
    assert torch.equal(y.cpu().double(), y64)
    assert stats == attn_ref.firing(counts)
    assert torch.equal(mask.cpu(), attn_ref.pack_mask(inr))
    assert_equal64((gq, gk, gv), attn_ref.backward(q, k, v, go, heads, scale)[:3], NAMES[1:])


# -------------------------------------------------------------------------------------------------------------- hi + mid + lo
def _bf16_terms(x):
    """fp64 values that are exact in fp32 -> their three bf16 terms (round to nearest even, exact residuals), fp64"""
    x = x.float()
    hi = x.bfloat16().float()
    mid = (x - hi).bfloat16().float()
    lo = (x - hi - mid).bfloat16().float()
    return hi.double(), mid.double(), lo.double()


@pytest.mark.parametrize("TB,heads,d,N,on_route", [
    pytest.param(2, 2, 45, 264, lambda d, N: d > 32 and N % 8 == 0 and N // 128 >= 2 and N % 16 == 8, id="sg2-split-ragged"),
    pytest.param(2, 2, 32, 136, lambda d, N: d <= 32 and N % 8 == 0 and N // 128 < 2 and N % 16 == 8, id="sg1-ragged"),
])
def test_general_operand_needs_all_three_bf16_terms(TB, heads, d, N, on_route):
    """s2f_sdsa_bwd_bf16 without a mask, gkv_ws = scale q go^T bit for bit: three non-zero tokens k / 8 per row of q anywhere in the
    row, go uniform on the multiples of 2^-20 in (-0.5, 0.5).  Every term q hi, q mid, q lo is a multiple of 2^-23, every sum of
    absolute terms is below 2^24 of them."""
    from spike2former_amd._lib import check, lib
    from spike2former_amd.ops.core import _ptr, _stream
    assert on_route(d, N)
    g = torch.Generator().manual_seed(d + N)
    C = heads * d
    where = torch.rand(TB, C, N, generator=g).argsort(-1)[..., :3]
    q = torch.zeros(TB, C, N, dtype=torch.float64).scatter_(-1, where, torch.randint(1, 9, (TB, C, 3), generator=g).double() / 8)
    assert bool(((q != 0).sum(-1) == 3).all())
    assert bool((q[..., :64] != 0).any()) and bool((q[..., N - 8:] != 0).any()) and bool((q[..., N // 2:N // 2 + 64] != 0).any())
    go = torch.randint(-(2 ** 19) + 1, 2 ** 19, (TB, C, N), generator=g).double() / 2 ** 20
    hi, mid, lo = _bf16_terms(go)
    assert torch.equal(hi + mid + lo, go) and bool((lo != 0).any())
    terms = attn_ref.heads_view(q, heads) @ attn_ref.heads_view(hi.abs() + mid.abs() + lo.abs(), heads).transpose(-1, -2)
    assert terms.max().item() * 2 ** 23 < 2 ** 24
    scale = 0.25
    want = attn_ref.backward(q, q, q, go, heads, scale)[3]
    qd = q.to(torch.bfloat16).cuda()
    assert torch.equal(qd.double().cpu(), q)
    kv = torch.zeros(TB, heads, d, d, device="cuda")
    gof = go.float().cuda()
    gq, gk, gv = (torch.empty(TB, C, N, device="cuda") for _ in range(3))
    ws = torch.empty(TB, heads, d, d, device="cuda")
    bs = C * N
    check(lib.s2f_sdsa_bwd_bf16(_ptr(qd), _ptr(qd), _ptr(qd), bs, bs, bs, _ptr(kv), _ptr(gof), 0, 8, _ptr(gq), _ptr(gk), _ptr(gv), bs, bs, bs,
                                _ptr(ws), TB, heads, d, N, N, scale, _stream()), "s2f_sdsa_bwd_bf16")
    assert torch.equal(ws.cpu().double(), want)


# -------------------------------------------------------------------------------------------------------------- general operands
def _rel(x, x64):
    return (x.detach().cpu().double() - x64).abs().max().item() / x64.abs().max().item()


def _assert_within_cpu_error(route, names, got, cpu32, ref64):
    line = []
    for name, a, c, r in zip(names, got, cpu32, ref64):
        e_kernel, e_cpu = _rel(a, r), _rel(c, r)
        line.append(f"{name} {e_kernel:.3g}/{e_cpu:.3g}=" + (f"{e_kernel / e_cpu:.2f}" if e_cpu > 0 else "-"))
    print(f"{route}: e_kernel/e_cpu  " + "  ".join(line))
    for name, a, c, r in zip(names, got, cpu32, ref64):
        assert _rel(a, r) <= 8 * _rel(c, r) + 2.0 ** -22, name


def test_general_fp32_route_within_cpu_error(ops):
    TB, heads, d, Nq, Nk = 2, 2, 45, 100, 300
    g = torch.Generator().manual_seed(11)
    C = heads * d
    q, k, v = (torch.randn(TB, C, n, generator=g).double() for n in (Nq, Nk, Nk))            # fp32 values, held in fp64
    go = torch.randn(TB, C, Nq, generator=g).double()
    scale = d ** -0.5
    got = run_fp32(ops, q, k, v, go, heads, scale)
    _assert_within_cpu_error("fp32 valu", NAMES, got, reference(q, k, v, go, heads, scale, torch.float32), reference(q, k, v, go, heads, scale))


@pytest.mark.parametrize("shape,on_route", [
    pytest.param((1, 2, 45, 264, 520), lambda d, Nq, Nk: Nq % 8 == 0 and Nk % 8 == 0 and d > 32, id="mfma2-and-sg2"),
    pytest.param((1, 2, 45, 100, 1028), lambda d, Nq, Nk: Nq % 8 == 4 and Nk % 8 == 4, id="valu-spike-general"),
])
def test_general_gradient_bf16_route_within_cpu_error(ops, shape, on_route, request):
    TB, heads, d, Nq, Nk = shape
    assert on_route(d, Nq, Nk)
    q, k, v, _ = draw_exact(*shape, seed=Nq + Nk)
    go = torch.randn(TB, heads * d, Nq, generator=torch.Generator().manual_seed(12)).double()
    scale = d ** -0.5
    got = run_bf16(ops, q, k, v, go, heads, scale, False)[:4]
    _assert_within_cpu_error("bf16 " + request.node.callspec.id, NAMES, got, reference(q, k, v, go, heads, scale, torch.float32),
                             reference(q, k, v, go, heads, scale))


def test_general_gradient_fused_route_within_cpu_error(ops):
    """the pre-activation never leaves the kernel: spike operands and a power-of-two scale make it exact, so the spikes and the mask
    are compared for equality and the three gradients take the place of the four outputs"""
    TB, heads, d, N = 1, 2, 64, 512
    assert d > 32 and N % 256 == 0
    q, k, v, _ = draw_exact(TB, heads, d, N, N, seed=13)
    g = torch.randn(TB, heads * d, N, generator=torch.Generator().manual_seed(14)).double()
    scale = fused_scale(q, k, v, heads)
    o64, _ = attn_ref.forward(q, k, v, heads, scale)
    inr = attn_ref.in_range(o64)
    assert bool(inr.any()) and not bool(inr.all())
    y, stats, mask, gq, gk, gv = run_fused(ops, q, k, v, g, heads, scale, False)
    y64, counts = attn_ref.neuron(o64)
    assert torch.equal(y.cpu().double(), y64) and stats == attn_ref.firing(counts) and torch.equal(mask.cpu(), attn_ref.pack_mask(inr))
    o32, _ = attn_ref.forward(q, k, v, heads, scale, torch.float32)
    cpu32 = attn_ref.backward(q, k, v, attn_ref.fused_grad(o32, g.float()), heads, scale, torch.float32)[:3]
    ref64 = attn_ref.backward(q, k, v, attn_ref.fused_grad(o64, g), heads, scale)[:3]
    _assert_within_cpu_error("bf16 fused mfma2-and-sg2", NAMES[1:], (gq, gk, gv), cpu32, ref64)
