"""Every route of the head's mask contraction (spike2former_amd/ops/gemm.py: mask_einsum_folded, mask_einsum, class_mask_product,
linear_tm and the token-major helpers under them) against the fp64 restatement of tests/mask_ref.py, at the smallest shapes that reach
it.  Each case is one row whose id names the route; the test first asserts from the shape the inequality that puts the row there
(through the library's own predicate where one decides) and builds its operands as the head does: fp32 E / W / bias leaves, a bf16
Spikes with its autograd handle for the spike map, the gradient read from the fp32 leaf behind the neuron.

  exact rows      E sparse multiples of 1/2 in [0, 4], spikes sparse multiples of 1/8, W / bias multiples of 1/8 in [-1, 1], g integers
                  in [-2, 2], T a power of two (scale = 1 / T moves exponents only).  Each row first asserts on its own draw (fp64,
                  mask_ref.abs_sums) that every sum of ABSOLUTE terms stays below 2^24 granules -- 1/16 for EW, dS, dW, dbias, 1/128
                  for out, 1/8 for H, 1/64 for dE -- so every fp32 intermediate and every partial sum is exact in any order (split-K
                  groups, atomics, matrix-core steps), and out, dS, dE, dW, dbias must EQUAL the fp64 values.
  three terms     the draws above fit the `hi` term of the bf16 x 3 operand split; this forward-only row gives W 20 significant bits
                  (a / 8 + b 2^-11 + c 2^-19), E one entry 1 per query row and the spike map one entry 1 per pixel and batch element,
                  so every output is ONE product W[o, c] 1 1, exact only with hi + mid + lo.
  general rows    randn E, W, bias, g (spikes stay spikes), one row per kernel family: per entry |got - ref64| <= c A + 1e-30 with A
                  the entry's sum of absolute terms (mask_ref.abs_sums) and c added up over the stages the entry passes through from
                  the constants of test_mask_einsum_matrix_core_path_vs_fp64: 2e-6 for a product (or fp32 sum) with one operand exact
                  in bf16, 4e-6 for a product of two general operands:
                    out    6e-6 = E W (4e-6) + the spike contraction (2e-6)
                    dS     8e-6 = E W (4e-6) + (scale EW)^T g, both general (4e-6)
                    dE     6e-6 = H = g S^T on spikes (2e-6) + H W^T (4e-6); the bias term rowsum(g) bias^T is one rounded sum
                    dW     6e-6 = H (2e-6) + E^T H (4e-6)
                    dbias  6e-6 = rowsum(g) (2e-6) + E^T rowsum(g) (4e-6)
                  mask_einsum: 2e-6 for out and dMF (E exact in bf16), 4e-6 for dE and for every product of the not-exact route;
                  class_mask_product 4e-6; linear_tm 4e-6 for y, gx, gw and 2e-6 for the bias gradient.
                  The same ratio max |err| / A of a plain fp32 CPU evaluation of mask_ref is printed next to the kernel's.

Measured on the MI355X, worst |err| / A over the entries, kernel | fp32 CPU (see docs/EXPERIMENTS.md for every row):
  folded (2,2,37,40,32,264)    nn-ex, pipelined H   out 3.8e-8 | 3.9e-8   dS 6.1e-8 | 6.2e-8   dE 3.0e-8 | 4.2e-8   dW 2.0e-8 | 2.8e-8   dbias 2.9e-9 | 2.9e-9
  folded (4,2,300,32,128,260)  fwd-ex, four groups  out 2.7e-8 | 3.4e-8   dS 6.0e-8 | 4.4e-8   dE 3.3e-8 | 2.9e-8   dW 5.6e-9 | 4.8e-9   dbias 1.0e-9 | 7.2e-10
  folded (2,2,37,20,32,24)     round-2 grouped H    out 6.9e-8 | 5.2e-8   dS 7.5e-8 | 5.0e-8   dE 7.7e-8 | 6.7e-8   dW 5.2e-8 | 7.9e-8   dbias 8.1e-9 | 7.0e-9
  folded (2,29,12,8,32,40)     H per (t, b)         out 8.4e-8 | 7.3e-8   dS 1.8e-7 | 1.2e-7   dE 6.3e-8 | 6.3e-8   dW 2.6e-8 | 2.2e-8   dbias 1.7e-9 | 4.8e-9
  folded (2,2,37,6,32,40)      E W on bmm_small     out 6.6e-8 | 5.2e-8   dS 1.9e-7 | 1.3e-7   dE 3.6e-8 | 4.1e-8   dW 5.2e-8 | 5.9e-8   dbias 1.1e-8 | 3.3e-9
  mask_einsum (2,2,37,40,260)  matrix cores         out 1.4e-7 | 2.4e-7   dE 7.0e-8 | 1.3e-7   dMF 1.6e-7 | 2.3e-7
  mask_einsum (2,2,37,40,35)   exact E, bmm_small   out 2.1e-7 | 1.5e-7   dE 2.5e-7 | 2.5e-7   dMF 2.1e-7 | 2.1e-7
  mask_einsum (2,2,37,40,260)  general, bmm_small   out 2.0e-7 | 2.2e-7   dE 2.0e-7 | 1.3e-7   dMF 2.2e-7 | 2.2e-7
  class_mask_product           K 19 / 150 / ragged  1.4e-7 | 1.3e-7,  2.3e-7 | 2.5e-7,  1.5e-7 | 1.5e-7
  linear_tm (111, c, 10)       c 6 / 6 no bias / 40 y 8.9e-8 | 1.0e-7, 1.3e-7 | 1.2e-7, 1.5e-7 | 7.3e-8; gx <= 2.4e-7 | 1.7e-7; gw <= 1.0e-7 | 1.0e-7
  i.e. every route is a factor of 8 to 200 inside its bound and within 2x of the plain fp32 evaluation (dbias of the Co = 6 row: 3x).

Not reached here: the `wm` = 2 / 4 tiles of s2f_spike_gemm_fwd_bf16_ex with a BACKWARD pass behind them (the two forward-only rows
reach the tiles: they need >= 512 workgroups, i.e. an 8 000-pixel map, and the backward of such a map is the same route as the small
rows); a spike map handed over in fp32 (mask_einsum_folded asserts bf16 Spikes); the packed-operand product with a gradient sink from
mask_einsum_folded itself (its dW leaves through autograd, not through a sink)."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ref  # noqa: E402

pytestmark = pytest.mark.gpu

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spike2former_amd", "csrc")
_SRC = open(os.path.join(_CSRC, "gemm_bf16.hip")).read()
BK = int(re.search(r"constexpr int BK = (\d+);", _SRC).group(1))          # contraction step of s2f_spike_gemm_fwd_bf16_ex
BN = int(re.search(r"constexpr int BN = (\d+);", _SRC).group(1))          # its column tile
MAX_JOBS = int(re.search(r"constexpr int kMaxJobs = (\d+);", _SRC).group(1))          # jobs of one grouped weight-gradient launch
THIN = 512          # fewer workgroups than this: the thin launch with its intra-workgroup contraction split

NAMES = ("out", "dS", "dE", "dW", "dbias")
GRANULES = {"EW": 16, "rowb": 16, "out": 128, "H": 8, "rs": 1, "dS": 16, "dE": 64, "dW": 16, "dbias": 16}          # per unit
C_FOLDED = {"out": 6e-6, "dS": 8e-6, "dE": 6e-6, "dW": 6e-6, "dbias": 6e-6}


@pytest.fixture(scope="module")
def ops():
    from spike2former_amd import ops
    return ops


def cdiv(a, b):
    return -(-a // b)


# -------------------------------------------------------------------------------------------------------------- routes, from the shape
def fwd_nn(T, B, Q, Co, C, HW):
    return HW % 8 == 0 and C % 32 == 0


def fwd_ex(T, B, Q, Co, C, HW):
    return HW % 8 == 4 and C % 32 == 0


def ex_mpad(Q):
    return cdiv(Q, 256) * 256 if Q > 256 else cdiv(Q, 64) * 64


def ex_blocks(B, Q, HW, rows):
    """workgroups of s2f_spike_gemm_fwd_bf16_ex on `rows`-row tiles, or 0 when the padded height is no multiple of them"""
    return cdiv(HW, BN) * (ex_mpad(Q) // rows) * B if ex_mpad(Q) % rows == 0 else 0


def ex_thin(T, B, Q, Co, C, HW):
    return fwd_ex(T, B, Q, Co, C, HW) and ex_blocks(B, Q, HW, 256) < THIN and ex_blocks(B, Q, HW, 128) < THIN and ex_blocks(B, Q, HW, 64) < THIN


def h_grouped(ops, T, B, Q, Co, C, HW):
    return T * B <= MAX_JOBS


def h_pipe(ops, T, B, Q, Co, C, HW):
    return (h_grouped(ops, T, B, Q, Co, C, HW) and bool(ops.DW_PIPE) and bool(ops.lib.s2f_spike_gemm_dw_pipe_ok(1, Q, C, HW))
            and (Q * HW) % 4 == 0 and (C * HW) % 8 == 0)


# -------------------------------------------------------------------------------------------------------------- draws and runners
def draw_exact(shape, seed, bias=True, g_rate=1.0):
    T, B, Q, Co, C, HW = shape
    g = torch.Generator().manual_seed(seed)
    E = torch.randint(0, 9, (T, B, Q, Co), generator=g).double() / 2 * (torch.rand(T, B, Q, Co, generator=g) < 0.3)
    S = torch.randint(1, 9, (T, B, C, HW), generator=g).double() / 8 * (torch.rand(T, B, C, HW, generator=g) < 0.25)
    W = torch.randint(-8, 9, (Co, C), generator=g).double() / 8
    b = torch.randint(-8, 9, (Co,), generator=g).double() / 8
    go = torch.randint(-2, 3, (B, Q, HW), generator=g).double() * (torch.rand(B, Q, HW, generator=g) < g_rate)
    return E, S, W, (b if bias else None), go


def draw_general(shape, seed, bias=True):
    T, B, Q, Co, C, HW = shape
    g = torch.Generator().manual_seed(seed)
    S = torch.randint(1, 9, (T, B, C, HW), generator=g).double() / 8 * (torch.rand(T, B, C, HW, generator=g) < 0.25)
    r = lambda *s: torch.randn(*s, generator=g).double()          # fp32 values: what the op receives is what the reference reads
    return r(T, B, Q, Co), S, (r(Co, C) * C ** -0.5).float().double(), (r(Co) if bias else None), r(B, Q, HW)


def assert_sums_exact(sums, granules=GRANULES, only=None):
    for name, x in sums.items():
        if x is not None and (only is None or name in only):
            assert x.max().item() * granules[name] < 2 ** 24, name


def to_spikes(ops, t):
    """fp64 map of multiples of 1/8 in [0, 1] -> (fp32 leaf, bf16 Spikes with its autograd handle): Q_IFNode(8 (k / 8)) = k / 8, and
    d Q_IFNode(8 src) / d src = 8 (1 / 8) = 1 on [0, 1], so src.grad is the gradient of the spike map, bit for bit"""
    src = t.float().cuda().requires_grad_(True)
    s, _ = ops.lif(src * 8.0, None, keep_v=False, spikes=True)
    assert isinstance(s, ops.Spikes) and s.tok is not None and s.data.dtype == torch.bfloat16
    assert torch.equal(s.data.float(), src.detach())
    return src, s


def plain_spikes(ops, t):
    """the same map as a Spikes whose handle asks for no gradient"""
    data = t.to(torch.bfloat16).cuda()
    assert torch.equal(data.double().cpu(), t)
    return ops.Spikes(data, ops._new_tok(data))


def run_folded(ops, E, S, W, bias, go, scale, want=("e", "s", "w"), backward=True):
    """-> {out, dS, dE, dW, dbias} (None: no gradient arrived)"""
    T, B, Q, Co = E.shape
    C, HW = S.shape[2:]
    e = E.float().cuda().requires_grad_("e" in want)
    src, sp = to_spikes(ops, S.reshape(T * B, C, HW)) if "s" in want else (None, plain_spikes(ops, S.reshape(T * B, C, HW)))
    w = W.float().cuda().requires_grad_("w" in want)
    b = None if bias is None else bias.float().cuda().requires_grad_("w" in want)
    out = ops.mask_einsum_folded(e, sp, w, b, scale, T, B, e_exact=True)
    assert out.shape == (B, Q, HW) and out.dtype == torch.float32
    if backward:
        assert type(out.grad_fn).__name__.startswith("_MaskEinsumFolded"), type(out.grad_fn).__name__
        out.backward(go.float().cuda())
    dS = None if src is None or src.grad is None else src.grad.view(T, B, C, HW)
    return {"out": out.detach(), "dS": dS, "dE": e.grad, "dW": w.grad, "dbias": None if b is None else b.grad}


def reference_folded(E, S, W, bias, go, scale, dtype=torch.float64):
    r = mask_ref.backward_folded(E, S, W, bias, go, scale, dtype)
    r["out"] = mask_ref.forward_folded(E, S, W, bias, scale, dtype)[0]
    return r


def assert_equal64(got, want, names):
    for name in names:
        a, b = got[name], want[name]
        if b is None:
            assert a is None, name
            continue
        assert a is not None and a.dtype == torch.float32 and a.shape == b.shape, name
        assert torch.equal(a.detach().cpu().double(), b), name


def assert_within(label, got, ref64, ref32, sums, c, names):
    """per entry |got - ref64| <= c A + 1e-30; prints the worst |err| / A of the kernel and of the plain fp32 evaluation"""
    worst = {}
    for name in names:
        if ref64[name] is None:
            continue
        A = sums[name]
        err = (got[name].detach().cpu().double() - ref64[name]).abs()
        err32 = (ref32[name].double() - ref64[name]).abs()
        worst[name] = (err - c[name] * A).max().item()
        print(f"ratio {label} {name}: kernel {(err / (A + 1e-300)).max().item():.2e}  fp32-cpu {(err32 / (A + 1e-300)).max().item():.2e}  bound {c[name]:.0e}")
    for name, over in worst.items():
        assert over <= 1e-30, (name, over)


# -------------------------------------------------------------------------------------------------------------- mask_einsum_folded
#   (T, B, Q, Co, C, HW), bias, switches, the inequality of the route
FOLDED_ROWS = [
    pytest.param((2, 2, 37, 40, 32, 264), True, {}, lambda o, *s: fwd_nn(*s) and s[2] % 64 != 0 and s[5] % BN == 8 and h_pipe(o, *s) and s[5] % 32 != 0,
                 id="fwd-nn-ex-ragged-q-last-column-tile-of-8+h-pipe-grouped-ragged-schedule"),
    pytest.param((2, 2, 300, 32, 32, 136), True, {}, lambda o, *s: fwd_nn(*s) and s[2] > 256 and s[1] > 1, id="fwd-nn-ex-q-above-one-row-tile"),
    pytest.param((4, 2, 37, 20, 64, 40), True, {}, lambda o, *s: fwd_nn(*s) and s[4] < s[0] * s[4] and s[4] > 32,
                 id="fwd-nn-ex-four-slabs-of-two-steps"),
    pytest.param((2, 2, 37, 40, 32, 264), False, {}, lambda o, *s: fwd_nn(*s), id="fwd-nn-ex-no-bias"),
    pytest.param((2, 2, 37, 20, 32, 260), True, {}, lambda o, *s: ex_thin(*s) and s[2] <= 256 and s[0] * s[4] < 4 * BK,
                 id="fwd-ex-64-row-padding-thin-one-group"),
    pytest.param((2, 1, 70, 20, 64, 36), True, {}, lambda o, *s: ex_thin(*s) and s[2] <= 256 and 4 * BK <= s[0] * s[4] < 16 * BK,
                 id="fwd-ex-64-row-padding-thin-two-groups"),
    pytest.param((4, 2, 300, 32, 128, 260), True, {}, lambda o, *s: ex_thin(*s) and s[2] > 256 and s[0] * s[4] >= 16 * BK,
                 id="fwd-ex-256-row-padding-thin-four-groups"),
    pytest.param((2, 2, 37, 20, 32, 260), False, {}, lambda o, *s: ex_thin(*s), id="fwd-ex-no-bias"),
    pytest.param((2, 2, 37, 20, 32, 64), True, {}, lambda o, *s: h_pipe(o, *s) and s[5] % 32 == 0, id="h-pipe-grouped-whole-steps"),
    pytest.param((2, 2, 37, 20, 32, 40), True, {}, lambda o, *s: h_pipe(o, *s) and s[5] % 32 != 0, id="h-pipe-grouped-ragged-schedule"),
    pytest.param((2, 2, 37, 20, 32, 24), True, {}, lambda o, *s: h_grouped(o, *s) and s[5] < 32 and not o.lib.s2f_spike_gemm_dw_pipe_ok(1, s[2], s[4], s[5]),
                 id="h-round2-grouped-short-rows"),
    pytest.param((2, 2, 37, 20, 32, 40), True, {"DW_PIPE": False}, lambda o, *s: h_grouped(o, *s) and not h_pipe(o, *s)
                 and o.lib.s2f_spike_gemm_dw_pipe_ok(1, s[2], s[4], s[5]), id="h-round2-grouped-pipeline-switched-off"),
    pytest.param((2, 29, 12, 8, 32, 40), True, {}, lambda o, *s: not h_grouped(o, *s), id="h-one-launch-per-slice"),
    pytest.param((2, 2, 37, 6, 32, 40), True, {}, lambda o, *s: s[3] % 4 != 0, id="ew-on-bmm-small-co6"),
]


def _switched(ops, switches):
    old = {k: getattr(ops, k) for k in switches}
    for k, v in switches.items():
        assert old[k] != v, k
        setattr(ops, k, v)
    return old


@pytest.mark.parametrize("shape,bias,switches,on_route", FOLDED_ROWS)
def test_folded_route_equals_fp64(ops, shape, bias, switches, on_route):
    T = shape[0]
    E, S, W, b, go = draw_exact(shape, seed=sum(shape) + len(switches), bias=bias)
    assert_sums_exact(mask_ref.abs_sums(E, S, W, b, go))
    old = _switched(ops, switches)
    try:
        assert on_route(ops, *shape)
        got = run_folded(ops, E, S, W, b, go, 1.0 / T)
    finally:
        for k, v in old.items():
            setattr(ops, k, v)
    assert_equal64(got, reference_folded(E, S, W, b, go, 1.0 / T), NAMES)


def _ex_wm(B, Q, HW):
    """the tile ladder of s2f_spike_gemm_fwd_bf16_ex: the widest of 256 / 128 rows that divides the padded height, is more than half
    filled by Q and gives at least THIN workgroups"""
    for rows in (256, 128):
        if ex_blocks(B, Q, HW, rows) >= THIN and Q > rows // 2:
            return rows // 64
    return 1


@pytest.mark.parametrize("shape,wm", [pytest.param((2, 4, 300, 8, 32, 4100), 2, id="fwd-ex-128-row-tiles"),
                                      pytest.param((2, 4, 300, 8, 32, 8196), 4, id="fwd-ex-256-row-tiles")])
def test_folded_forward_on_the_wide_tiles_equals_fp64(ops, shape, wm):
    """the 128- and 256-row tiles of s2f_spike_gemm_fwd_bf16_ex need 512 workgroups: forward only, on maps of 4 100 / 8 196 pixels"""
    T, B, Q, Co, C, HW = shape
    assert fwd_ex(*shape) and Q > 256 and _ex_wm(B, Q, HW) == wm
    E, S, W, b, go = draw_exact(shape, seed=HW, bias=True, g_rate=0.0)
    aE, aS, aW, ab = (t.abs() for t in (E, S, W, b))
    a_out, a_ew, a_rowb = mask_ref.forward_folded(aE, aS, aW, ab, 1.0)
    assert_sums_exact({"out": a_out, "EW": a_ew, "rowb": a_rowb})
    with torch.no_grad():
        got = run_folded(ops, E, S, W, b, go, 1.0 / T, want=(), backward=False)
    assert torch.equal(got["out"].cpu().double(), mask_ref.forward_folded(E, S, W, b, 1.0 / T)[0])


@pytest.mark.parametrize("shape,on_route", [pytest.param((2, 2, 37, 20, 32, 264), fwd_nn, id="fwd-nn-ex"),
                                            pytest.param((2, 2, 37, 20, 32, 260), fwd_ex, id="fwd-ex")])
def test_folded_forward_needs_all_three_terms_of_the_packed_operand(ops, shape, on_route):
    """W = a / 8 + b 2^-11 + c 2^-19 (20 significant bits); every query row of E holds ONE entry 1 and every pixel of a batch element
    ONE spike of 1 over all (t, c): out[b, q, n] = scale W[o(t*, q), c*] for the (t*, c*) of the pixel -- a single product, exact, that
    needs the hi, mid and lo term of (E W)"""
    T, B, Q, Co, C, HW = shape
    assert on_route(*shape)
    g = torch.Generator().manual_seed(HW)
    W = (torch.randint(-8, 9, (Co, C), generator=g).double() / 8 + torch.randint(-7, 8, (Co, C), generator=g).double() * 2.0 ** -11
         + torch.randint(1, 8, (Co, C), generator=g).double() * 2.0 ** -19)
    assert torch.equal(W.float().double(), W) and not torch.equal(W.bfloat16().double() + (W - W.bfloat16().double()).bfloat16().double(), W)
    E = torch.zeros(T, B, Q, Co, dtype=torch.float64)
    E.scatter_(3, torch.randint(0, Co, (T, B, Q, 1), generator=g), 1.0)
    S = torch.zeros(B, T * C, HW, dtype=torch.float64)
    S.scatter_(1, torch.randint(0, T * C, (B, 1, HW), generator=g), 1.0)
    S = S.view(B, T, C, HW).transpose(0, 1).contiguous()
    with torch.no_grad():
        got = run_folded(ops, E, S, W, None, None, 1.0 / T, want=(), backward=False)
    assert torch.equal(got["out"].cpu().double(), mask_ref.forward_folded(E, S, W, None, 1.0 / T)[0])


PARTIAL_SHAPE = (2, 2, 37, 20, 32, 40)


@pytest.fixture(scope="module")
def partial_case():
    E, S, W, b, go = draw_exact(PARTIAL_SHAPE, seed=77)
    assert_sums_exact(mask_ref.abs_sums(E, S, W, b, go))
    return (E, S, W, b, go), reference_folded(E, S, W, b, go, 0.5)


@pytest.mark.parametrize("want,present", [pytest.param(("e",), ("dE",), id="only-e"), pytest.param(("s",), ("dS",), id="only-the-spike-map"),
                                          pytest.param(("w",), ("dW", "dbias"), id="only-w-and-bias")])
def test_folded_partial_gradients(ops, partial_case, want, present):
    """only the inputs that ask receive a gradient -- and it is the exact one; the rest stay None"""
    draw, ref = partial_case
    got = run_folded(ops, *draw, 0.5, want=want)
    assert_equal64(got, ref, ("out",) + present)
    for name in set(NAMES) - {"out"} - set(present):
        assert got[name] is None, name


def test_folded_contract_is_checked_before_anything_is_launched(ops):
    """C % 32 == 0 and HW % 4 == 0, or a RuntimeError that names both conditions and the values it got"""
    for C, HW in ((40, 36), (32, 35)):
        E, S, W, b, go = draw_exact((2, 1, 5, 4, C, HW), seed=C)
        with pytest.raises(RuntimeError) as err:
            run_folded(ops, E, S, W, b, go, 0.5, want=())
        msg = str(err.value)
        assert "C % 32 == 0" in msg and "HW % 4 == 0" in msg and f"C={C}" in msg and f"HW={HW}" in msg, msg


GENERAL_FOLDED = [
    pytest.param((2, 2, 37, 40, 32, 264), {}, lambda o, *s: fwd_nn(*s) and h_pipe(o, *s), id="fwd-nn-ex+h-pipe-grouped"),
    pytest.param((4, 2, 300, 32, 128, 260), {}, lambda o, *s: ex_thin(*s) and s[0] * s[4] >= 16 * BK, id="fwd-ex-four-groups"),
    pytest.param((2, 2, 37, 20, 32, 24), {}, lambda o, *s: h_grouped(o, *s) and not h_pipe(o, *s), id="h-round2-grouped"),
    pytest.param((2, 29, 12, 8, 32, 40), {}, lambda o, *s: not h_grouped(o, *s), id="h-one-launch-per-slice"),
    pytest.param((2, 2, 37, 6, 32, 40), {}, lambda o, *s: s[3] % 4 != 0, id="ew-on-bmm-small-co6"),
]


@pytest.mark.parametrize("shape,switches,on_route", GENERAL_FOLDED)
def test_folded_route_general_operands_within_the_fp32_bound(ops, shape, switches, on_route):
    T = shape[0]
    assert on_route(ops, *shape)
    E, S, W, b, go = draw_general(shape, seed=sum(shape))
    got = run_folded(ops, E, S, W, b, go, 1.0 / T)
    sums = mask_ref.abs_sums(E, S, W, b, go)
    sums = {k: (None if v is None else v / T) if k in NAMES else v for k, v in sums.items()}
    assert_within("folded " + "x".join(map(str, shape)), got, reference_folded(E, S, W, b, go, 1.0 / T),
                  reference_folded(E, S, W, b, go, 1.0 / T, torch.float32), sums, C_FOLDED, NAMES)


# -------------------------------------------------------------------------------------------------------------- mask_einsum
#   (T, B, Q, C, HW), e_exact, the inequality of the route
UNFOLDED_ROWS = [
    pytest.param((2, 2, 37, 40, 260), True, lambda o, T, B, Q, C, HW: HW % 4 == 0 and o.SPIKE_GEMM_ENABLED and B > 1 and Q % 64 != 0
                 and C % 32 != 0 and (T * C) % 32 != 0, id="matrix-cores-ragged-q-c40"),
    pytest.param((2, 2, 37, 40, 35), True, lambda o, T, B, Q, C, HW: HW % 4 != 0, id="e-exact-ragged-rows-on-bmm-small"),
    pytest.param((2, 2, 37, 40, 260), False, lambda o, T, B, Q, C, HW: HW % 4 == 0, id="e-not-exact-on-bmm-small"),
]
UNFOLDED_GRANULES = {"out": 16, "dE": 8, "dMF": 2}


def run_unfolded(ops, E, MF, go, scale, e_exact):
    e, mf = E.float().cuda().requires_grad_(True), MF.float().cuda().requires_grad_(True)
    out = ops.mask_einsum(e, mf, scale, e_exact=e_exact)
    out.backward(go.float().cuda())
    return {"out": out.detach(), "dE": e.grad, "dMF": mf.grad}


def reference_unfolded(E, MF, go, scale, dtype=torch.float64):
    dE, dMF = mask_ref.backward_unfolded(E, MF, go, scale, dtype)
    return {"out": mask_ref.forward_unfolded(E, MF, scale, dtype), "dE": dE, "dMF": dMF}


@pytest.mark.parametrize("shape,e_exact,on_route", UNFOLDED_ROWS)
def test_mask_einsum_route_equals_fp64(ops, shape, e_exact, on_route):
    T, B, Q, C, HW = shape
    assert on_route(ops, *shape)
    g = torch.Generator().manual_seed(HW + int(e_exact))
    E = torch.randint(0, 9, (T, B, Q, C), generator=g).double() / 2 * (torch.rand(T, B, Q, C, generator=g) < 0.3)
    MF = torch.randint(-8, 9, (T, B, C, HW), generator=g).double() / 8
    go = torch.randint(-2, 3, (B, Q, HW), generator=g).double()
    assert_sums_exact(mask_ref.abs_sums_unfolded(E, MF, go), UNFOLDED_GRANULES)
    assert_equal64(run_unfolded(ops, E, MF, go, 1.0 / T, e_exact), reference_unfolded(E, MF, go, 1.0 / T), ("out", "dE", "dMF"))


@pytest.mark.parametrize("shape,e_exact,on_route", UNFOLDED_ROWS)
def test_mask_einsum_route_general_operands_within_the_fp32_bound(ops, shape, e_exact, on_route):
    T, B, Q, C, HW = shape
    assert on_route(ops, *shape)
    g = torch.Generator().manual_seed(HW + 2 + int(e_exact))
    E = torch.randn(T, B, Q, C, generator=g)
    E = (E.bfloat16().float() if e_exact else E).double()          # e_exact is the caller's promise that E is a bf16 value
    MF, go = torch.randn(T, B, C, HW, generator=g).double(), torch.randn(B, Q, HW, generator=g).double()
    c = {"out": 2e-6, "dE": 4e-6, "dMF": 2e-6} if e_exact else {"out": 4e-6, "dE": 4e-6, "dMF": 4e-6}
    sums = {k: v / T for k, v in mask_ref.abs_sums_unfolded(E, MF, go).items()}
    assert_within("mask_einsum " + "x".join(map(str, shape)) + f" exact={e_exact}", run_unfolded(ops, E, MF, go, 1.0 / T, e_exact),
                  reference_unfolded(E, MF, go, 1.0 / T), reference_unfolded(E, MF, go, 1.0 / T, torch.float32), sums, c, ("out", "dE", "dMF"))


# -------------------------------------------------------------------------------------------------------------- class_mask_product
#   (B, Q, K, h, w)
CLASS_ROWS = [
    pytest.param((3, 37, 19, 6, 10), lambda B, Q, K, h, w: (h * w) % 4 == 0 and (Q * K) % 4 != 0, id="packed-operand-k19-unaligned-scores"),
    pytest.param((3, 37, 150, 6, 10), lambda B, Q, K, h, w: (h * w) % 4 == 0 and K > 128, id="packed-operand-k150"),
    pytest.param((3, 37, 19, 5, 7), lambda B, Q, K, h, w: (h * w) % 4 != 0, id="ragged-map-on-bmm-small"),
]


@pytest.mark.parametrize("shape,on_route", CLASS_ROWS)
def test_class_mask_product_route_equals_fp64_and_keeps_the_fp32_bound(ops, shape, on_route):
    B, Q, K, h, w = shape
    assert on_route(*shape)
    g = torch.Generator().manual_seed(K + h)
    cls = torch.randint(-8, 9, (B, Q, K), generator=g).double() / 8
    mp = torch.randint(0, 9, (B, Q, h, w), generator=g).double() / 8
    assert mask_ref.class_mask(cls.abs(), mp).max().item() * 64 < 2 ** 24
    with torch.no_grad():
        got = ops.class_mask_product(cls.float().cuda(), mp.float().cuda())
        assert got.shape == (B, K, h, w) and torch.equal(got.cpu().double(), mask_ref.class_mask(cls, mp))
        cls, mp = torch.randn(B, Q, K, generator=g).double(), torch.rand(B, Q, h, w, generator=g).double()
        got = ops.class_mask_product(cls.float().cuda(), mp.float().cuda())
    A = mask_ref.class_mask(cls.abs(), mp.abs())
    assert_within("class_mask " + "x".join(map(str, shape)), {"out": got}, {"out": mask_ref.class_mask(cls, mp)},
                  {"out": mask_ref.class_mask(cls, mp, torch.float32)}, {"out": A}, {"out": 4e-6}, ("out",))


# -------------------------------------------------------------------------------------------------------------- linear_tm
LIN = ("y", "gx", "gw", "gb")
C_LINEAR = {"y": 4e-6, "gx": 4e-6, "gw": 4e-6, "gb": 2e-6}


def run_linear(ops, x, w, b, gy, lead=(3,)):
    n, c = x.shape
    xl = x.float().view(*lead, n // lead[0], c).cuda().requires_grad_(True)
    wl = torch.nn.Parameter(w.float().cuda())
    bl = None if b is None else torch.nn.Parameter(b.float().cuda())
    y = ops.linear_tm(xl, wl, bl)
    y.backward(gy.float().view(*lead, n // lead[0], -1).cuda())
    return xl, wl, bl, y


def linear_sums(x, w, b, gy):
    y, gx, gw, gb = mask_ref.linear(x.abs(), w.abs(), None if b is None else b.abs(), gy.abs())
    return {"y": y, "gx": gx, "gw": gw, "gb": gb}


def draw_linear(n, c, o, bias, seed, exact):
    g = torch.Generator().manual_seed(seed)
    if exact:
        r = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g).double()
        return r(-8, 9, n, c) / 8, r(-8, 9, o, c) / 8, (r(-8, 9, o) / 8 if bias else None), r(-2, 3, n, o)
    r = lambda *s: torch.randn(*s, generator=g).double()
    return r(n, c), (r(o, c) * c ** -0.5).float().double(), (r(o) if bias else None), r(n, o)


@pytest.mark.parametrize("n,c,o,bias,on_route", [
    pytest.param(111, 6, 10, True, lambda c: c % 4 != 0, id="bmm-small-c6-bias"),
    pytest.param(111, 6, 10, False, lambda c: c % 4 != 0, id="bmm-small-c6-no-bias"),
    pytest.param(111, 40, 10, True, lambda c: c % 4 == 0, id="matrix-cores-c40-o10"),
])
def test_linear_tm_route_equals_fp64_and_keeps_the_fp32_bound(ops, n, c, o, bias, on_route):
    assert on_route(c)
    for exact in (True, False):
        x, w, b, gy = draw_linear(n, c, o, bias, n + c + int(bias), exact)
        xl, wl, bl, y = run_linear(ops, x, w, b, gy)
        got = {"y": y.detach().reshape(n, o), "gx": xl.grad.reshape(n, c), "gw": wl.grad, "gb": None if bl is None else bl.grad}
        ref = dict(zip(LIN, mask_ref.linear(x, w, b, gy)))
        if exact:
            # x, w, b on multiples of 1/8, gy integers: granules 1/64 (y), 1/8 (gx, gw), 1 (gb)
            assert_sums_exact(linear_sums(x, w, b, gy), {"y": 64, "gx": 8, "gw": 8, "gb": 1})
            assert_equal64(got, ref, LIN)
        else:
            assert_within(f"linear_tm {n}x{c}x{o} bias={bias}", got, ref, dict(zip(LIN, mask_ref.linear(x, w, b, gy, torch.float32))),
                          linear_sums(x, w, b, gy), C_LINEAR, LIN)


def test_linear_tm_weight_gradient_adds_into_its_sink(ops):
    """with a gradient sink the weight gradient is ADDED to the flat buffer (beta = 1 of the packed-operand product): the slot is
    pre-filled with 0.75 and must hold 0.75 + gw afterwards, autograd gets no tensor for the weight"""
    from spike2former_amd.dist import FlatGradAllReduce
    n, c, o = 111, 40, 10
    x, w, b, gy = draw_linear(n, c, o, True, 5, True)
    assert_sums_exact(linear_sums(x, w, b, gy), {"y": 64, "gx": 8, "gw": 8, "gb": 1})
    xl = x.float().cuda().requires_grad_(True)
    wl, bl = torch.nn.Parameter(w.float().cuda()), torch.nn.Parameter(b.float().cuda())
    assert ops.GRAD_SINKS is None
    red = FlatGradAllReduce([wl], 1)
    try:
        red.install_sinks()
        red.zero()
        assert ops._sink_for(wl) is not None and ops._sink_for(wl).data_ptr() == red.views[0].data_ptr()
        red.views[0].fill_(0.75)
        y = ops.linear_tm(xl, wl, bl)
        y.backward(gy.float().cuda())
        ref = dict(zip(LIN, mask_ref.linear(x, w, b, gy)))
        assert wl.grad is None
        assert torch.equal(red.views[0].cpu().double(), ref["gw"] + 0.75)
        assert_equal64({"y": y.detach(), "gx": xl.grad, "gb": bl.grad}, ref, ("y", "gx", "gb"))
    finally:
        red.close()
        ops.GRAD_SINKS = None
        ops.wgrad_drop()


def test_token_major_helpers_on_bmm_small(ops):
    """the c % 4 != 0 legs of _mm_tm / _mtm_tm (no op of the package reaches the second: the ops above gate on their row width first)"""
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randint(-8, 9, s, generator=g).double() / 8
    x, w, a, bmat = r(37, 6), r(10, 6), r(37, 10), r(37, 6)
    assert x.shape[1] % 4 != 0 and bmat.shape[1] % 4 != 0
    f = lambda t: t.float().cuda()
    assert torch.equal(ops._mm_tm(f(x), f(w)).cpu().double(), x @ w.t())
    assert torch.equal(ops._mtm_tm(f(a), f(bmat)).cpu().double(), a.t() @ bmat)
    out = torch.full((10, 6), 7.0, device="cuda")
    assert ops._mtm_tm(f(a), f(bmat), out=out) is out and torch.equal(out.cpu().double(), a.t() @ bmat)
