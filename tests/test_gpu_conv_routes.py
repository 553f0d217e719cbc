"""Every route of the dense and depthwise convolutions (spike2former_amd/ops/conv.py: conv_dense, dwconv and the launch sequences
_ConvDense / _DWConv choose from the shape) against the fp64 restatement of tests/conv_ref.py, at the smallest shapes that reach it.
Each case is one row whose id names the route; the test first asserts from the shape the inequality that puts the row there (through
the library's own predicate where one decides), builds its operands as the model does -- fp32 w / bias leaves, a bf16 Spikes with its
autograd handle for a spike map, the gradient read from the fp32 leaf behind the neuron -- and proves the route by counting the lib.*
calls of the whole census below: a row lists the launches it must make, every other symbol of the census must stay at zero.

  exact rows      spikes sparse multiples of 1/8 in [0, 1] (a general fp32 map: multiples of 1/8 in [-1, 1]), w / bias / border
                  multiples of 1/8 in [-1, 1], gy integers in [-2, 2].  Each row first asserts on its own draw (fp64,
                  conv_ref.abs_sums) that every sum of ABSOLUTE terms stays below 2^24 granules -- 1/64 for y, 1/8 for dx, dw, db --
                  so every fp32 partial sum is exact in any order (split-K, atomics, matrix-core steps, FMA or not), and y, dx, dw,
                  db must EQUAL the fp64 values.
  three terms     the draws above fit the `hi` term of the bf16 x 3 operand split.  These rows give ONE operand 20 significant bits,
                  v = +-(a / 8 + b 2^-11 + c 2^-19) with 4 <= a <= 8, 1 <= b <= 3, c odd below 8: hi = bf16(v) is a / 8 (the rest is
                  below half its last place), and the rest, b 2^-11 + c 2^-19, has set bits from 2^-11 or above down to 2^-19, more
                  than the 8 significant bits of `mid` -- the test asserts for EVERY entry that bf16(v) + bf16(v - bf16(v)) != v.
                  The other operand is one-hot with value 1 (one spike per
                  image, or one gy entry per image; a second draw puts one on every third row and column, which a 3 x 3 window meets
                  once), so every non-zero output is ONE product v * 1, equal to the fp64 value only if hi, mid AND lo were
                  multiplied: a kernel that drops the lo term of any one split returns hi + mid there, which differs from v by the
                  assertion above, and the row fails.  (Run against two mutant builds, docs/EXPERIMENTS.md: with the lo plane of the
                  weight conversions zeroed the forward rows and the dX rows with the wide w fail, with the lo term of the in-kernel
                  splits dropped the dX rows with the wide gy and the stem rows, while every exact row passes.)
  general rows    randn w, bias, gy (fp32 values read back as fp64: the op and the reference see the same numbers), spikes stay
                  spikes, the stem image is randn: per entry |got - ref64| <= c A + 1e-30 with A the entry's sum of absolute terms
                  (conv_ref.abs_sums) and c from the constants of test_mask_einsum_matrix_core_path_vs_fp64 / C_FOLDED of
                  test_gpu_mask_contraction.py:
                    2e-6          a product with one operand exact in bf16 (spikes x three-term weight; dY split x spikes)
                    4e-6          a product of two general operands (dX of every dense route, the stem's forward and dW, every
                                  product on bmm_small)
                    K K 2^-24     the depthwise forward and dX: the worst case of a K K-term fp32 sum in any order
                    2e-5          the depthwise dW: the constant of test_dwconv_vs_aten_cpu, per entry against A
                    2e-6          a bias gradient: one fp32 sum
                  The same ratio max |err| / A of a plain fp32 CPU evaluation of conv_ref is printed next to the kernel's.

Measured on the MI355X, worst |err| / A over the entries, kernel | fp32 CPU (docs/EXPERIMENTS.md has the same table):
  conv_dense (N, C, M, H, W, k, stride, pad)
  implicit-pipe-dw     (2,64,128,32,32,3,1,1)   y 2.3e-7 | 8.3e-8   dx 2.4e-7 | 6.0e-8   dw 5.2e-8 | 4.9e-8
  implicit-general-dx  (2,96,64,32,32,3,1,1)    y 2.4e-7 | 8.1e-8   dx 2.4e-7 | 7.1e-8   dw 4.7e-8 | 4.8e-8
  implicit-wide-m      (1,96,256,32,32,3,1,1)   y 2.5e-7 | 8.6e-8   dx 2.4e-7 | 3.8e-8   dw 9.3e-8 | 7.2e-8
  implicit-bias        (1,32,32,32,32,3,1,1)    y 1.7e-7 | 6.9e-8   dx 2.1e-7 | 6.7e-8   dw 7.0e-8 | 6.8e-8   db 8.4e-9 | 1.3e-8
  implicit-stats       (2,96,64,32,32,3,1,1)    y 2.4e-7 | 8.1e-8   dx 2.4e-7 | 7.1e-8   dw 4.9e-8 | 4.8e-8
  implicit-fp32-spikes (1,32,64,32,32,3,1,1)    y 1.3e-7 | 9.9e-8   dx 2.2e-7 | 5.7e-8   dw 6.9e-8 | 7.3e-8
  threshold-above      (2,32,64,29,36,3,1,1)    y 2.4e-7 | 1.0e-7   dx 2.2e-7 | 8.7e-8   dw 4.1e-8 | 5.2e-8
  threshold-below      (2,32,64,28,36,3,1,1)    y 2.3e-7 | 9.4e-8   dx 2.3e-7 | 5.8e-8   dw 5.8e-8 | 5.4e-8
  columns-stride2      (2,32,40,16,16,3,2,1)    y 1.3e-7 | 7.1e-8   dx 1.8e-7 | 1.8e-7   dw 1.6e-7 | 1.9e-7
  columns-ragged       (2,32,40,9,9,3,2,1)      y 1.4e-7 | 7.4e-8   dx 1.9e-7 | 1.9e-7   dw 1.6e-7 | 1.5e-7
  columns-narrow-m     (2,32,8,16,16,3,2,1)     y 1.4e-7 | 5.7e-8   dx 1.9e-7 | 1.8e-7   dw 1.4e-7 | 1.2e-7
  transposed-dx-k3     (1,64,24,8,8,3,1,1)      y 2.0e-7 | 5.5e-8   dx 1.7e-7 | 6.2e-8   dw 1.8e-7 | 1.9e-7
  transposed-dx-k5     (1,48,16,8,8,5,1,2)      y 1.0e-7 | 4.7e-8   dx 2.6e-7 | 4.7e-8   dw 1.7e-7 | 2.0e-7
  stem                 (2,3,32,32,32,7,2,3)     y 2.1e-7 | 1.3e-7   dx 5.9e-8 | 5.7e-8   dw 4.6e-8 | 2.0e-7
  dwconv (N, C, H, W, K, pad)
  tile-vector-border   (2,6,33,40,3,1)          y 1.2e-7 | 1.2e-7   dx 1.7e-7 | 1.7e-7   dw 2.0e-8 | 1.0e-8
  tile-5               (2,4,37,45,5,2)          y 2.3e-7 | 1.8e-7   dx 2.2e-7 | 1.8e-7   dw 1.0e-8 | 7.4e-9
  pad-full-border      (1,3,6,8,5,4)            y 1.3e-7 | 1.4e-7   dx 7.7e-8 | 8.8e-8   dw 3.0e-8 | 2.4e-8
  wide-bf16-border     (1,3,33,132,3,1)         y 1.0e-7 | 1.2e-7   dx 2.0e-7 | 1.5e-7   dw 9.3e-9 | 1.1e-8
  stats-tile           (2,8,16,16,3,1)          y 1.1e-7 | 1.0e-7   dx 1.5e-7 | 1.6e-7   dw 2.2e-8 | 3.5e-8
  wgrad-walk-3         (4,685,33,33,3,1)        y 2.1e-7 | 2.0e-7   dx 2.3e-7 | 2.5e-7   dw 2.4e-8 | 1.6e-8
  i.e. every dense route is a factor of 8 or more inside its bound (the worst: 2.6e-7 against 4e-6, 2.5e-7 against 2e-6), the
  depthwise forward and dX a factor of 2.3 or more inside K K 2^-24 (2.3e-7 against 5.4e-7 at K = 3), the depthwise dW a factor of 600;
  the matrix-core routes are within 6.4x of the plain fp32 evaluation (the worst: dx of implicit-wide-m), the stencils within 2x.  The dw figures move by up to 1e-8 from run to run (atomic adds), y and dx repeat.

Not reached here: the settled switches in their off position (SPIKE_GEMM_ENABLED, CONV3X3_IMPLICIT, CONV3X3_DX_IMPLICIT = False send
every row to a route another row already takes); a column matrix of fp32 SPIKES (stride 2 on an fp32 spike tensor: s2f_spike_gemm_fwd
/ s2f_spike_gemm_dw under _spike_product / _spike_dw -- ops/gemm.py's branches, the model's spikes are bf16); the early returns for
gy is None (autograd does not call a backward without a gradient); the SPIKE_GEMM_CHECK assertion; weight gradients on the side
stream (WGRAD_STREAM, off since its measurement); a depthwise map whose address is no multiple of 16 bytes with stats=True (the
allocator never hands one out); a dwconv whose map or weight asks for no gradient; the deferred queue's general list (_defer_dw_general: only _DenseGemm queues there); and the eval-mode
fusions dwconv_bn_lif_eval / conv3x3_bn_lif_eval, which existing tests pin bit for bit to the unfused path this suite pins."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref  # noqa: E402

pytestmark = pytest.mark.gpu

# every launch ops/conv.py (and the helpers of ops/gemm.py and ops/core.py it calls) can make for a convolution
CENSUS = ("pgemm_conv3x3_bf16", "pgemm_conv3x3_bf16_stats", "spike_conv3x3_fwd", "spike_conv3x3_fwd_bf16", "pgemm_conv3x3_f32",
          "conv3x3_general", "shift1_bf16", "spike_conv3x3_dw_pipe", "spike_conv3x3_dw_bf16", "spike_conv3x3_dw", "im2col", "col2im",
          "pgemm_nn_bf16", "pgemm_nn_bf16_stats", "spike_gemm_fwd_bf16", "spike_gemm_fwd", "pgemm_dx_f32", "pgemm_dx_f32_stats",
          "pgemm_dx_f32_grouped", "bmm_f32", "spike_gemm_dw_bf16", "spike_gemm_dw", "spike_gemm_dw_pipe", "gemm_dw_general",
          "spike_gemm_dw_pipe_grouped", "spike_gemm_dw_grouped", "gemm_dw_general_grouped", "dwconv_fwd", "dwconv_fwd_stats",
          "dwconv_bwd_input", "dwconv_bwd_weight", "dwconv_bn_lif_fwd")
TS, WT, HT = 32, 64, 32          # csrc/dwconv.hip: the tile side, and the wide form's tile
GEMM_TILE = 128                  # columns behind one BatchNorm partial of the GEMM epilogues (include/s2f.h)
SWITCHES = ("CONV3X3_IMPLICIT_MIN_PIXELS", "BN_PARTIALS_SINGLE", "SPIKE_GEMM_TERMS", "DEFER_DW", "GRAD_SINKS")
DENSE, DW = ("y", "dx", "dw", "db"), ("y", "dx", "dw")
GRANULES = {"y": 64, "dx": 8, "dw": 8, "db": 8}          # per unit


@pytest.fixture(scope="module")
def ops():
    from spike2former_amd import ops
    return ops


@pytest.fixture
def census(ops, monkeypatch):
    """{symbol without its s2f_ prefix: [argument tuples]} of every call since the last clear()"""
    calls = {}

    def wrap(name, fn):
        def counted(*a):
            calls.setdefault(name, []).append(a)
            return fn(*a)
        return counted
    for name in CENSUS:
        monkeypatch.setattr(ops.lib, "s2f_" + name, wrap(name, getattr(ops.lib, "s2f_" + name)))
    return calls


@pytest.fixture
def switches(ops):
    """set(NAME=value, ...) for the switches a row needs; every switch of SWITCHES is put back and the deferred queue dropped"""
    old = {k: getattr(ops, k) for k in SWITCHES}

    def set_(**kw):
        for k, v in kw.items():
            assert k in SWITCHES, k
            setattr(ops, k, v)
    try:
        yield set_
    finally:
        for k, v in old.items():
            setattr(ops, k, v)
        ops.wgrad_drop()


def cdiv(a, b):
    return -(-a // b)


def counts(census):
    return {k: len(v) for k, v in census.items() if v}


# -------------------------------------------------------------------------------------------------------------- routes, from the shape
def out_hw(N, C, M, H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def out_len(*shape):
    Ho, Wo = out_hw(*shape)
    return Ho * Wo


def same3(N, C, M, H, W, k, s, p):
    return k == 3 and s == 1 and p == 1


def fwd_implicit(ops, N, C, M, H, W, k, s, p):
    return same3(N, C, M, H, W, k, s, p) and C % 32 == 0 and W % 4 == 0 and H * W >= ops.CONV3X3_IMPLICIT_MIN_PIXELS


def fwd_columns_spike(ops, *shape):
    return not fwd_implicit(ops, *shape) and out_len(*shape) % 4 == 0


def dx_implicit(N, C, M, H, W, k, s, p):
    return same3(N, C, M, H, W, k, s, p) and M % 32 == 0 and W % 4 == 0


def dx_pipelined(N, C, M, H, W, k, s, p):
    return dx_implicit(N, C, M, H, W, k, s, p) and (C <= 64 or M >= 256)


def dx_transposed(N, C, M, H, W, k, s, p):
    return not dx_implicit(N, C, M, H, W, k, s, p) and M < C and s == 1 and out_hw(N, C, M, H, W, k, s, p) == (H, W)


def dw_pipe(ops, N, C, M, H, W, k, s, p):
    return M >= 128 and C >= 64 and bool(ops.lib.s2f_spike_conv3x3_dw_pipe_ok(N, M, C, H, W))


def dense_fast(*shape):
    return out_len(*shape) % 4 == 0 and out_len(*shape) >= 128


def wide_form(N, C, H, W, K, pad):
    return K == 3 and pad == 1 and W % 4 == 0 and W >= 2 * WT and H >= HT


def dw_out(N, C, H, W, K, pad):
    return H + 2 * pad - K + 1, W + 2 * pad - K + 1


def wgrad_walk(N, C, H, W, K, pad):
    """(workgroups per plane, tiles per plane) of dw_wgrad_kernel: csrc/dwconv.hip s2f_dwconv_bwd_weight"""
    Ho, Wo = dw_out(N, C, H, W, K, pad)
    ntiles = cdiv(Wo, TS) * cdiv(Ho, TS)
    return max(1, min(cdiv(8192, N * C), ntiles)), ntiles


# -------------------------------------------------------------------------------------------------------------- draws
def _grid(g, lo, hi, *s):
    return torch.randint(lo, hi + 1, s, generator=g).double()


def draw_spikes(g, *s):
    return _grid(g, 1, 8, *s) / 8 * (torch.rand(*s, generator=g) < 0.25)


def draw_dense(shape, kind, seed, bias, exact):
    """-> x, w, bias or None, gy in fp64 (fp32 values); kind: 'bf16' / 'fp32-spikes' (a spike map) or 'image' (a general fp32 map)"""
    N, C, M, H, W, k, s, p = shape
    Ho, Wo = out_hw(*shape)
    g = torch.Generator().manual_seed(seed)
    r = lambda *sh: torch.randn(*sh, generator=g).double()
    if kind == "image":
        x = _grid(g, -8, 8, N, C, H, W) / 8 if exact else r(N, C, H, W)
    else:
        x = draw_spikes(g, N, C, H, W)
    if exact:
        return x, _grid(g, -8, 8, M, C, k, k) / 8, (_grid(g, -8, 8, M) / 8 if bias else None), _grid(g, -2, 2, N, M, Ho, Wo)
    return x, (r(M, C, k, k) * (C * k * k) ** -0.5).float().double(), (r(M) if bias else None), r(N, M, Ho, Wo)


def draw_dw(shape, kind, seed, border, exact):
    N, C, H, W, K, pad = shape
    Ho, Wo = dw_out(*shape)
    g = torch.Generator().manual_seed(seed)
    r = lambda *sh: torch.randn(*sh, generator=g).double()
    if kind == "bf16":
        x = draw_spikes(g, N, C, H, W)
    else:
        x = _grid(g, -8, 8, N, C, H, W) / 8 if exact else r(N, C, H, W)
    if exact:
        return x, _grid(g, -8, 8, C, 1, K, K) / 8, (_grid(g, -8, 8, C) / 8 if border else None), _grid(g, -2, 2, N, C, Ho, Wo)
    return x, (r(C, 1, K, K) / K).float().double(), (r(C) if border else None), r(N, C, Ho, Wo)


def wide_values(g, *s):
    """20 significant bits per entry, none of them representable by two bf16 terms (see the module docstring)"""
    v = _grid(g, 4, 8, *s) / 8 + _grid(g, 1, 3, *s) * 2.0 ** -11 + (2 * _grid(g, 0, 3, *s) + 1) * 2.0 ** -19
    v = v * (2 * _grid(g, 0, 1, *s) - 1)
    hi = v.bfloat16().double()
    assert torch.equal(v.float().double(), v) and bool((hi + (v - hi).bfloat16().double() != v).all())
    return v


def one_hot_map(g, N, C, H, W, lattice):
    """one entry 1 per image, or (lattice) a 1 in a drawn channel at every third row and column: any 3 x 3 window meets at most one"""
    x = torch.zeros(N, C, H, W, dtype=torch.float64)
    if lattice:
        hs, ws = torch.arange(1, H, 3), torch.arange(1, W, 3)
        ch = torch.randint(0, C, (N, len(hs), len(ws)), generator=g)
        for n in range(N):
            x[n, ch[n], hs.view(-1, 1).expand_as(ch[n]), ws.view(1, -1).expand_as(ch[n])] = 1.0
    else:
        for n in range(N):
            x[n, int(torch.randint(0, C, (1,), generator=g)), int(torch.randint(0, H, (1,), generator=g)),
              int(torch.randint(0, W, (1,), generator=g))] = 1.0
    return x


def assert_sums_exact(sums):
    for name, a in sums.items():
        if a is not None:
            assert a.max().item() * GRANULES[name] < 2 ** 24, name


# -------------------------------------------------------------------------------------------------------------- runners
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


def operand(ops, x, kind, grad=True):
    """-> (the fp32 leaf that receives dx or None, what the op is handed, spike_input)"""
    if kind == "bf16":
        return to_spikes(ops, x) + (True,) if grad else (None, plain_spikes(ops, x), True)
    src = x.float().cuda().requires_grad_(grad)
    return src, src, kind == "fp32-spikes"


def run_dense(ops, census, shape, kind, draw, stats=False, w=None, backward=1, dx=True):
    """-> ({y, dx, dw, db} (None: no gradient arrived), the BatchNorm partials handed over with y or None, the launch counts);
    `backward`: how many times the backward pass runs; `dx`: whether the map asks for its gradient"""
    N, C, M, H, W, k, s, p = shape
    x64, w64, b64, gy64 = draw
    w = torch.nn.Parameter(w64.float().cuda()) if w is None else w
    b = None if b64 is None else torch.nn.Parameter(b64.float().cuda())
    src, xin, spike_input = operand(ops, x64, kind, grad=dx and gy64 is not None)
    census.clear()
    y = ops.conv_dense(xin, w, b, s, p, spike_input, stats=stats)
    assert y.shape == (N, M) + out_hw(*shape) and y.dtype == torch.float32
    part = ops.stats_of(y)
    if gy64 is not None:
        assert type(y.grad_fn).__name__.startswith("_ConvDense"), type(y.grad_fn).__name__
        for i in range(backward):
            y.backward(gy64.float().cuda(), retain_graph=i + 1 < backward)
    got = {"y": y.detach(), "dx": None if src is None else src.grad, "dw": w.grad, "db": None if b is None else b.grad}
    return got, part, counts(census)


def run_dw(ops, census, shape, kind, draw, stats=False, w=None):
    N, C, H, W, K, pad = shape
    x64, w64, r64, gy64 = draw
    w = torch.nn.Parameter(w64.float().cuda()) if w is None else w
    border = None if r64 is None else r64.float().cuda()
    src, xin, _ = operand(ops, x64, kind)
    census.clear()
    y = ops.dwconv(xin, w, pad, border, stats=stats)
    assert y.shape == (N, C) + dw_out(*shape) and y.dtype == torch.float32
    part = ops.stats_of(y)
    assert type(y.grad_fn).__name__.startswith("_DWConv"), type(y.grad_fn).__name__
    y.backward(gy64.float().cuda())
    return {"y": y.detach(), "dx": src.grad, "dw": w.grad}, part, counts(census)


def describe(name, err, bad):
    """the worst entry with its index, the number of entries off, and every border of a map on its own"""
    e = err.detach()
    idx = tuple(int(i) for i in torch.unravel_index(e.argmax(), e.shape))
    msg = f"{name}: {int(bad.sum())} of {bad.numel()} entries off, worst {e.max().item():.3e} at {idx}"
    if e.dim() == 4 and e.shape[-1] > 1 and e.shape[-2] > 1:
        edges = {"first row": (Ellipsis, 0, slice(None)), "last row": (Ellipsis, -1, slice(None)),
                 "first column": (Ellipsis, slice(None), 0), "last column": (Ellipsis, slice(None), -1)}
        msg += "; " + ", ".join(f"{k} {int(bad[i].sum())} off (worst {e[i].max().item():.3e})" for k, i in edges.items())
    return msg


def assert_equal64(got, want, names):
    for name in names:
        a, b = got[name], want[name]
        if b is None:
            assert a is None, name
            continue
        assert a is not None and a.dtype == torch.float32 and a.shape == b.shape, name
        a = a.detach().cpu().double()
        assert torch.equal(a, b), describe(name, (a - b).abs(), a != b)


def assert_within(label, got, ref64, ref32, sums, c, names):
    """per entry |got - ref64| <= c A + 1e-30; prints the worst |err| / A of the kernel and of the plain fp32 evaluation"""
    failed = []
    for name in names:
        if ref64[name] is None:
            assert got[name] is None, name
            continue
        A = sums[name]
        assert got[name] is not None and got[name].dtype == torch.float32 and got[name].shape == ref64[name].shape, name
        err = (got[name].detach().cpu().double() - ref64[name]).abs()
        err32 = (ref32[name].double() - ref64[name]).abs()
        print(f"ratio {label} {name}: kernel {(err / (A + 1e-300)).max().item():.2e}  fp32-cpu {(err32 / (A + 1e-300)).max().item():.2e}"
              f"  bound {c[name]:.1e}")
        over = err - c[name] * A
        if over.max().item() > 1e-30:
            failed.append(describe(name, over.clamp_min(0), over > 1e-30))
    assert not failed, failed


def assert_partials(part, y, P, tile, exact):
    """the BatchNorm partials handed over with y: [channels, P, 2] fp32 (sum, sum of squares) per tile of at most `tile` values.  On
    the exact draw (the sum of |y| of a channel below 2^24 granules of 1/64) the sums add up to the channel's sum exactly; the sums of
    squares, `tile` rounded squares summed in fp32, within (tile + 1) 2^-24 of the channel's sum of squares"""
    ch = y.shape[1]
    assert part is not None and tuple(part.shape) == (ch, P, 2) and part.dtype == torch.float32
    y64 = y.double().transpose(0, 1).reshape(ch, -1).cpu()
    s1, s2 = part[:, :, 0].double().sum(1).cpu(), part[:, :, 1].double().sum(1).cpu()
    if exact:
        assert y64.abs().sum(1).max().item() * 64 < 2 ** 24
        assert torch.equal(s1, y64.sum(1)), (s1 - y64.sum(1)).abs().max().item()
    want = (y64 * y64).sum(1)
    assert bool(((s2 - want).abs() <= (tile + 1) * 2.0 ** -24 * want + 1e-30).all()), ((s2 - want).abs() / (want + 1e-300)).max().item()


def single_pass_switch(ops, switches, N, ch, L):
    """a map this BatchNorm would take in one pass stores partials only under BN_PARTIALS_SINGLE: ask the library, set it if so"""
    assert ops.BN_PARTIALS
    if ops.lib.s2f_bn_single_pass(N, ch, L):
        switches(BN_PARTIALS_SINGLE=True)


# -------------------------------------------------------------------------------------------------------------- conv_dense
#   id, (N, C, M, H, W, k, stride, pad), operand, bias, stats, switches, the inequality of the route, the launches, (c of y, c of dw)
SPIKE_C, BMM_C = 2e-6, 4e-6
_IMPL_DX, _IMPL_DXG = {"pgemm_conv3x3_f32": 1}, {"conv3x3_general": 1}
_DW_PIPE, _DW_R2 = {"shift1_bf16": 1, "spike_conv3x3_dw_pipe": 1}, {"spike_conv3x3_dw_bf16": 1}
_COLS = {"im2col": 1, "pgemm_nn_bf16": 1}
_COLS_DX = {"pgemm_dx_f32": 1, "col2im": 1}


def _row(id_, shape, kind, route, launches, c=(SPIKE_C, SPIKE_C), bias=False, stats=False, sw=None):
    return pytest.param(shape, kind, bias, stats, sw or {}, route, launches, c, id=id_)


ROW_PIPE_DW = _row("implicit-pipe-dw", (2, 64, 128, 32, 32, 3, 1, 1), "bf16",
                   lambda o, *s: fwd_implicit(o, *s) and dx_pipelined(*s) and s[1] <= 64 and dw_pipe(o, *s),
                   {"pgemm_conv3x3_bf16": 1, **_IMPL_DX, **_DW_PIPE})
ROW_GENERAL_DX = _row("implicit-general-dx", (2, 96, 64, 32, 32, 3, 1, 1), "bf16",
                      lambda o, *s: fwd_implicit(o, *s) and dx_implicit(*s) and not dx_pipelined(*s) and s[2] < 128,
                      {"pgemm_conv3x3_bf16": 1, **_IMPL_DXG, **_DW_R2})
STEM = (2, 3, 32, 32, 32, 7, 2, 3)
ROW_STEM = _row("stem", STEM, "image", lambda o, *s: not fwd_implicit(o, *s) and dense_fast(*s) and not dx_implicit(*s) and not dx_transposed(*s),
                {"im2col": 1, "pgemm_dx_f32": 2, "col2im": 1, "gemm_dw_general": 1}, c=(BMM_C, BMM_C))
ROW_STRIDE2 = _row("columns-stride2", (2, 32, 40, 16, 16, 3, 2, 1), "bf16",
                   lambda o, *s: fwd_columns_spike(o, *s) and not dx_implicit(*s) and not dx_transposed(*s) and s[2] >= 16,
                   {**_COLS, **_COLS_DX, "spike_gemm_dw_bf16": 1})
GENERAL_DENSE = [
    ROW_PIPE_DW,
    ROW_GENERAL_DX,
    _row("implicit-wide-m", (1, 96, 256, 32, 32, 3, 1, 1), "bf16",
         lambda o, *s: fwd_implicit(o, *s) and dx_pipelined(*s) and s[1] > 64 and s[2] >= 256 and dw_pipe(o, *s),
         {"pgemm_conv3x3_bf16": 1, **_IMPL_DX, **_DW_PIPE}),
    _row("implicit-bias-no-partials", (1, 32, 32, 32, 32, 3, 1, 1), "bf16", lambda o, *s: fwd_implicit(o, *s) and dx_pipelined(*s) and s[2] < 128,
         {"pgemm_conv3x3_bf16": 1, **_IMPL_DX, **_DW_R2}, bias=True, stats=True),
    _row("implicit-stats", (2, 96, 64, 32, 32, 3, 1, 1), "bf16", lambda o, *s: fwd_implicit(o, *s) and not dx_pipelined(*s) and s[2] < 128,
         {"pgemm_conv3x3_bf16_stats": 1, **_IMPL_DXG, **_DW_R2}, stats=True),
    _row("implicit-fp32-spikes", (1, 32, 64, 32, 32, 3, 1, 1), "fp32-spikes", lambda o, *s: fwd_implicit(o, *s) and dx_pipelined(*s),
         {"spike_conv3x3_fwd": 1, **_IMPL_DX, "spike_conv3x3_dw": 1}),
    _row("threshold-above-1044-pixels-width-36", (2, 32, 64, 29, 36, 3, 1, 1), "bf16",
         lambda o, *s: fwd_implicit(o, *s) and s[3] * s[4] - s[4] < o.CONV3X3_IMPLICIT_MIN_PIXELS and s[4] & (s[4] - 1) and dx_pipelined(*s),
         {"pgemm_conv3x3_bf16": 1, **_IMPL_DX, **_DW_R2}),
    _row("threshold-below-1008-pixels-columns-implicit-dx", (2, 32, 64, 28, 36, 3, 1, 1), "bf16",
         lambda o, *s: same3(*s) and not fwd_implicit(o, *s) and s[3] * s[4] + s[4] >= o.CONV3X3_IMPLICIT_MIN_PIXELS
         and fwd_columns_spike(o, *s) and dx_pipelined(*s) and s[2] >= 16, {**_COLS, **_IMPL_DX, "spike_gemm_dw_bf16": 1}),
    ROW_STRIDE2,
    _row("columns-ragged-l25-all-on-bmm", (2, 32, 40, 9, 9, 3, 2, 1), "bf16",
         lambda o, *s: not fwd_implicit(o, *s) and out_len(*s) == 25 and not dx_implicit(*s) and not dx_transposed(*s),
         {"im2col": 1, "bmm_f32": 3, "col2im": 1}, c=(BMM_C, BMM_C)),
    _row("columns-narrow-m8-dw-on-bmm", (2, 32, 8, 16, 16, 3, 2, 1), "bf16",
         lambda o, *s: fwd_columns_spike(o, *s) and s[2] < 16 and not dx_implicit(*s) and not dx_transposed(*s),
         {**_COLS, **_COLS_DX, "bmm_f32": 1}, c=(SPIKE_C, BMM_C)),
    _row("transposed-dx-k3", (1, 64, 24, 8, 8, 3, 1, 1), "bf16", lambda o, *s: fwd_columns_spike(o, *s) and s[2] % 32 != 0 and dx_transposed(*s) and s[2] >= 16,
         {"im2col": 2, "pgemm_nn_bf16": 1, "bmm_f32": 1, "spike_gemm_dw_bf16": 1}),
    _row("transposed-dx-k5", (1, 48, 16, 8, 8, 5, 1, 2), "bf16", lambda o, *s: fwd_columns_spike(o, *s) and s[2] % 32 != 0 and dx_transposed(*s) and s[2] >= 16,
         {"im2col": 2, "pgemm_nn_bf16": 1, "bmm_f32": 1, "spike_gemm_dw_bf16": 1}),
    ROW_STEM,
]
EXACT_ONLY_DENSE = [
    _row("implicit-two-terms", (1, 32, 64, 32, 32, 3, 1, 1), "bf16", lambda o, *s: fwd_implicit(o, *s) and dx_pipelined(*s) and s[2] < 128,
         {"spike_conv3x3_fwd_bf16": 1, **_IMPL_DX, **_DW_R2}, sw={"SPIKE_GEMM_TERMS": 2}),
    _row("stem-stats", STEM, "image", lambda o, *s: dense_fast(*s), {"im2col": 1, "pgemm_dx_f32_stats": 1, "pgemm_dx_f32": 1, "col2im": 1, "gemm_dw_general": 1},
         stats=True),
    _row("stem-bias-no-partials", STEM, "image", lambda o, *s: dense_fast(*s), {"im2col": 1, "pgemm_dx_f32": 2, "col2im": 1, "gemm_dw_general": 1},
         bias=True, stats=True),
    _row("stem-small-l64-forward-on-bmm", (2, 3, 32, 16, 16, 7, 2, 3), "image",
         lambda o, *s: not dense_fast(*s) and out_len(*s) % 4 == 0 and not dx_transposed(*s),
         {"im2col": 1, "bmm_f32": 1, **_COLS_DX, "gemm_dw_general": 1}),
]


def _dense_case(ops, switches, census, shape, kind, bias, stats, sw, on_route, launches, seed, exact):
    N, C, M = shape[:3]
    switches(**sw)
    assert on_route(ops, *shape)
    wants_part = stats and not bias
    if wants_part:
        single_pass_switch(ops, switches, N, M, out_len(*shape))
    draw = draw_dense(shape, kind, seed, bias, exact)
    sums = conv_ref.abs_sums(conv_ref.conv_dense, draw[0], draw[1], draw[2], shape[6], shape[7], draw[3])
    if exact:
        assert_sums_exact(sums)
    got, part, launched = run_dense(ops, census, shape, kind, draw, stats=stats)
    assert launched == launches, launched
    for name, a in census.items():          # no launch adds into anything: there is no sink
        if name in ("spike_gemm_dw_bf16", "gemm_dw_general"):
            assert all(args[-2] == 0 for args in a), name
    if wants_part:
        # the partials, and y bit for bit what the launch without them stores
        assert_partials(part, got["y"], int(ops.lib.s2f_bn_partials_count(N, out_len(*shape))), GEMM_TILE, exact)
        plain, none, _ = run_dense(ops, census, shape, kind, draw, stats=False)
        assert none is None and torch.equal(plain["y"], got["y"])
    else:
        assert part is None
    return draw, sums, got


@pytest.mark.parametrize("shape,kind,bias,stats,sw,on_route,launches,c", GENERAL_DENSE + EXACT_ONLY_DENSE)
def test_conv_dense_route_equals_fp64(ops, switches, census, shape, kind, bias, stats, sw, on_route, launches, c):
    draw, _, got = _dense_case(ops, switches, census, shape, kind, bias, stats, sw, on_route, launches, sum(shape) + int(bias), True)
    assert_equal64(got, conv_ref.conv_dense(draw[0], draw[1], draw[2], shape[6], shape[7], draw[3]), DENSE)


@pytest.mark.parametrize("shape,kind,bias,stats,sw,on_route,launches,c", GENERAL_DENSE)
def test_conv_dense_route_general_operands_within_the_fp32_bound(ops, switches, census, shape, kind, bias, stats, sw, on_route, launches, c):
    draw, sums, got = _dense_case(ops, switches, census, shape, kind, bias, stats, sw, on_route, launches, sum(shape) + 1000, False)
    args = (draw[0], draw[1], draw[2], shape[6], shape[7], draw[3])
    assert_within("conv_dense " + "x".join(map(str, shape)) + (" bias" if bias else "") + (" stats" if stats else ""), got,
                  conv_ref.conv_dense(*args), conv_ref.conv_dense(*args, torch.float32), sums,
                  {"y": c[0], "dx": 4e-6, "dw": c[1], "db": 2e-6}, DENSE)


# ---- three terms
def _forward_only(ops, census, shape, x, w):
    with torch.no_grad():
        got, _, launched = run_dense(ops, census, shape, "bf16", (x, w, None, None))
    return got["y"], launched


@pytest.mark.parametrize("lattice", [False, True], ids=["one-spike-per-image", "a-spike-every-third-pixel"])
@pytest.mark.parametrize("shape,launches", [pytest.param((2, 32, 64, 32, 32, 3, 1, 1), {"pgemm_conv3x3_bf16": 1}, id="implicit-forward"),
                                            pytest.param((2, 32, 40, 16, 16, 3, 2, 1), _COLS, id="column-matrix-forward")])
def test_conv_dense_forward_needs_all_three_terms_of_the_weight(ops, switches, census, shape, launches, lattice):
    """w with 20 significant bits, a spike map of single ones: every non-zero output is ONE product w[m, c, i, j] * 1"""
    N, C, M, H, W, k, s, p = shape
    assert fwd_implicit(ops, *shape) == ("pgemm_conv3x3_bf16" in launches) and out_len(*shape) % 4 == 0
    g = torch.Generator().manual_seed(H + int(lattice))
    w, x = wide_values(g, M, C, k, k), one_hot_map(g, N, C, H, W, lattice)
    ref = conv_ref.conv_dense(x, w, None, s, p, None)["y"]
    assert torch.equal(conv_ref.abs_sums(conv_ref.conv_dense, x, w, None, s, p, None)["y"], ref.abs()) and bool((ref != 0).any())
    y, launched = _forward_only(ops, census, shape, x, w)
    assert launched == launches, launched
    y = y.cpu().double()
    assert torch.equal(y, ref), describe("y", (y - ref).abs(), y != ref)


@pytest.mark.parametrize("lattice", [False, True], ids=["one-entry-per-image", "an-entry-every-third-pixel"])
@pytest.mark.parametrize("wide", ["w", "gy"])
@pytest.mark.parametrize("shape,launches", [pytest.param((2, 32, 64, 32, 32, 3, 1, 1), _IMPL_DX, id="pipelined"),
                                            pytest.param((2, 96, 64, 32, 32, 3, 1, 1), _IMPL_DXG, id="general")])
def test_conv_dense_implicit_dx_needs_all_three_terms_of_both_operands(ops, switches, census, shape, launches, wide, lattice):
    """dx = flip(w)^T (*) gy with ONE non-zero product per entry: the 20-bit values in w against single ones in gy, then the 20-bit
    values in the single entries of gy against w in {-1, -1/2, 1/2, 1} (a power of two moves the exponent only)"""
    N, C, M, H, W, k, s, p = shape
    assert dx_implicit(*shape) and dx_pipelined(*shape) == ("pgemm_conv3x3_f32" in launches)
    g = torch.Generator().manual_seed(C + int(lattice))
    gy = one_hot_map(g, N, M, H, W, lattice)
    if wide == "w":
        w = wide_values(g, M, C, k, k)
    else:
        w = (2 * _grid(g, 0, 1, M, C, k, k) - 1) / (1 + _grid(g, 0, 1, M, C, k, k))
        gy = gy * wide_values(g, N, M, H, W)
    x = draw_spikes(g, N, C, H, W)
    ref = conv_ref.conv_dense(x, w, None, s, p, gy)["dx"]
    assert torch.equal(conv_ref.abs_sums(conv_ref.conv_dense, x, w, None, s, p, gy)["dx"], ref.abs()) and bool((ref != 0).any())
    src, sp = to_spikes(ops, x)
    wl = w.float().cuda()          # no gradient asked for the weight: the input gradient alone is launched
    y = ops.conv_dense(sp, wl, None, s, p, True)
    census.clear()
    y.backward(gy.float().cuda())
    assert counts(census) == launches, counts(census)
    dx = src.grad.cpu().double()
    assert torch.equal(dx, ref), describe("dx", (dx - ref).abs(), dx != ref)


@pytest.mark.parametrize("wide", ["image", "gy"])
def test_stem_weight_gradient_needs_all_three_terms_of_both_operands(ops, switches, census, wide):
    """s2f_gemm_dw_general splits BOTH operands: gy holds one entry per image, in a channel of its own, so dw[m, c, i, j] is ONE
    product gy[n, m, l] * window(n, l)[c, i, j] -- first the 20-bit values in the image against a gy entry of 1, then the 20-bit
    values in the gy entries against an image of ones"""
    N, C, M, H, W, k, s, p = STEM
    assert dense_fast(*STEM) and not fwd_implicit(ops, *STEM)
    Ho, Wo = out_hw(*STEM)
    g = torch.Generator().manual_seed(len(wide))
    gy = torch.zeros(N, M, Ho, Wo, dtype=torch.float64)
    for n, m in enumerate(torch.randperm(M, generator=g)[:N].tolist()):
        gy[n, m, int(torch.randint(0, Ho, (1,), generator=g)), int(torch.randint(0, Wo, (1,), generator=g))] = 1.0
    if wide == "image":
        x = wide_values(g, N, C, H, W)
    else:
        x, gy = torch.ones(N, C, H, W, dtype=torch.float64), gy * wide_values(g, N, M, Ho, Wo)
    w = _grid(g, -8, 8, M, C, k, k) / 8
    ref = conv_ref.conv_dense(x, w, None, s, p, gy)["dw"]
    assert torch.equal(conv_ref.abs_sums(conv_ref.conv_dense, x, w, None, s, p, gy)["dw"], ref.abs()) and bool((ref != 0).any())
    wl = torch.nn.Parameter(w.float().cuda())
    y = ops.conv_dense(x.float().cuda(), wl, None, s, p, False)
    census.clear()
    y.backward(gy.float().cuda())
    assert counts(census) == {"gemm_dw_general": 1}, counts(census)
    dw = wl.grad.cpu().double()
    assert torch.equal(dw, ref), describe("dw", (dw - ref).abs(), dw != ref)


# ---- gradient sinks and the deferred queue
class _Sink:
    """FlatGradAllReduce([w], 1) with its sinks installed, zeroed, and w's view pre-filled with 0.75"""

    def __init__(self, ops, w):
        from spike2former_amd.dist import FlatGradAllReduce
        assert ops.GRAD_SINKS is None
        self.ops, self.red = ops, FlatGradAllReduce([w], 1)
        self.red.install_sinks()
        self.red.zero()
        self.view = self.red.views[0]
        assert ops._sink_for(w) is not None and ops._sink_for(w).data_ptr() == self.view.data_ptr()
        self.view.fill_(0.75)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.red.close()
        self.ops.GRAD_SINKS = None
        self.ops.wgrad_drop()
        return False

    def holds(self, want):
        got = self.view.detach().cpu().double()
        assert torch.equal(got, want), describe("sink", (got - want).abs(), got != want)


def _sink_draw(shape, kind, seed):
    draw = draw_dense(shape, kind, seed, False, True)
    assert_sums_exact(conv_ref.abs_sums(conv_ref.conv_dense, draw[0], draw[1], None, shape[6], shape[7], draw[3]))
    return draw, conv_ref.conv_dense(draw[0], draw[1], None, shape[6], shape[7], draw[3])


@pytest.mark.parametrize("times", [1, 2], ids=["one-backward", "two-backwards-into-the-same-sink"])
@pytest.mark.parametrize("row", [pytest.param(r.values, id=r.id) for r in (ROW_PIPE_DW, ROW_GENERAL_DX)])
def test_implicit_weight_gradient_adds_into_its_sink(ops, switches, census, row, times):
    """the tap-major staging tensor [M, 3, 3, C] (zeroed first for the pipelined kernel, which adds into it) reaches the sink by ONE
    permuted add: the sink, pre-filled with 0.75, holds times * dw + 0.75 exactly, and autograd gets no tensor for the weight -- a
    missing zero fill, a wrong permutation and a double add all show"""
    shape, kind, _, _, _, on_route, launches, _ = row
    assert on_route(ops, *shape)
    draw, ref = _sink_draw(shape, kind, 31 + times)
    w = torch.nn.Parameter(draw[1].float().cuda())
    with _Sink(ops, w) as sink:
        # (two backwards: the map asks for no gradient, so only the weight gradient runs twice)
        got, _, launched = run_dense(ops, census, shape, kind, draw, w=w, backward=times, dx=times == 1)
        dx_launches = ("pgemm_conv3x3_f32", "conv3x3_general")
        want = {k: v * (times if "dw" in k or k == "shift1_bf16" else 1) for k, v in launches.items() if times == 1 or k not in dx_launches}
        assert launched == want, launched
        assert w.grad is None and got["dw"] is None
        sink.holds(times * ref["dw"] + 0.75)
        assert_equal64(got, ref, ("y",) + (("dx",) if times == 1 else ()))


@pytest.mark.parametrize("defer", [True, False], ids=["deferred-queue", "direct-accumulate"])
def test_column_matrix_weight_gradient_into_its_sink(ops, switches, census, defer):
    """columns-stride2 with a sink.  DEFER_DW: the backward launches no weight gradient and leaves the sink alone; wgrad_flush() then
    makes exactly ONE grouped launch -- the pipelined one where s2f_spike_gemm_dw_pipe_ok takes the job -- and dw + 0.75 is there.
    Without DEFER_DW: the direct launch with accumulate = 1"""
    shape, kind, _, _, _, on_route, launches, _ = ROW_STRIDE2.values
    N, C, M = shape[:3]
    K, L = C * 9, out_len(*shape)
    assert on_route(ops, *shape) and (N, M, K, L) == (2, 40, 288, 64)
    switches(DEFER_DW=defer)
    draw, ref = _sink_draw(shape, kind, 41)
    w = torch.nn.Parameter(draw[1].float().cuda())
    with _Sink(ops, w) as sink:
        got, _, launched = run_dense(ops, census, shape, kind, draw, w=w)
        assert w.grad is None and got["dw"] is None
        assert_equal64(got, ref, ("y", "dx"))
        if defer:
            assert launched == {k: v for k, v in launches.items() if k != "spike_gemm_dw_bf16"}, launched
            assert bool((sink.view == 0.75).all())          # nothing is in the sink before the flush
            census.clear()
            ops.wgrad_flush()
            pipe = bool(ops.DW_PIPE) and bool(ops.lib.s2f_spike_gemm_dw_pipe_ok(N, M, K, L))
            assert pipe, "s2f_spike_gemm_dw_pipe_ok no longer takes (2, 40, 288, 64)"
            assert counts(census) == {"spike_gemm_dw_pipe_grouped": 1}, counts(census)
            assert census["spike_gemm_dw_pipe_grouped"][0][1] == 1          # one job
            census.clear()
            ops.wgrad_flush()          # the queue is empty afterwards
            assert counts(census) == {}
        else:
            assert launched == launches, launched
            assert census["spike_gemm_dw_bf16"][0][-2] == 1          # accumulate
        sink.holds(ref["dw"] + 0.75)


def test_deferred_weight_gradient_on_the_round2_grouped_kernel(ops, switches, census):
    """a job the pipelined grouped kernel does not take (L = 16 < 32) stays on s2f_spike_gemm_dw_grouped"""
    shape = (2, 32, 40, 8, 8, 3, 2, 1)
    N, C, M = shape[:3]
    K, L = C * 9, out_len(*shape)
    assert fwd_columns_spike(ops, *shape) and L == 16 and not ops.lib.s2f_spike_gemm_dw_pipe_ok(N, M, K, L) and ops.DEFER_DW
    draw, ref = _sink_draw(shape, "bf16", 43)
    w = torch.nn.Parameter(draw[1].float().cuda())
    with _Sink(ops, w) as sink:
        got, _, launched = run_dense(ops, census, shape, "bf16", draw, w=w)
        assert launched == {**_COLS, **_COLS_DX}, launched
        assert bool((sink.view == 0.75).all())
        census.clear()
        ops.wgrad_flush()
        assert counts(census) == {"spike_gemm_dw_grouped": 1}, counts(census)
        sink.holds(ref["dw"] + 0.75)
        assert_equal64(got, ref, ("y", "dx"))


def test_stem_weight_gradient_adds_into_its_sink(ops, switches, census):
    """s2f_gemm_dw_general with accumulate = 1 straight into the sink"""
    shape, kind, _, _, _, on_route, launches, _ = ROW_STEM.values
    assert on_route(ops, *shape)
    draw, ref = _sink_draw(shape, kind, 47)
    w = torch.nn.Parameter(draw[1].float().cuda())
    with _Sink(ops, w) as sink:
        got, _, launched = run_dense(ops, census, shape, kind, draw, w=w)
        assert launched == launches, launched
        args = census["gemm_dw_general"][0]
        assert args[-2] == 1 and args[4] == sink.view.data_ptr()
        assert w.grad is None and got["dw"] is None
        sink.holds(ref["dw"] + 0.75)
        assert_equal64(got, ref, ("y", "dx"))


# -------------------------------------------------------------------------------------------------------------- dwconv
#   id, (N, C, H, W, K, pad), operand, border, stats, the inequality of the route, general draw too
_DW_LAUNCHES = {"dwconv_fwd": 1, "dwconv_bwd_input": 1, "dwconv_bwd_weight": 1}
_DW_STATS = {"dwconv_fwd_stats": 1, "dwconv_bwd_input": 1, "dwconv_bwd_weight": 1}


def _dwrow(id_, shape, kind, route, border=False, stats=False, launches=_DW_LAUNCHES, general=False):
    return pytest.param(shape, kind, border, stats, route, launches, general, id=id_)


def _tiles(*s):
    Ho, Wo = dw_out(*s)
    return cdiv(Ho, TS) * cdiv(Wo, TS)


def _one_tile_per_workgroup(*s):
    return wgrad_walk(*s)[0] == wgrad_walk(*s)[1]


ROW_TILE_BORDER = _dwrow("tile-vector-border-bf16-four-ragged-tiles", (2, 6, 33, 40, 3, 1), "bf16",
                         lambda o, *s: s[3] % 4 == 0 and not wide_form(*s) and _tiles(*s) == 4 and s[2] % TS and s[3] % TS, border=True, general=True)
WIDE_F32, WIDE_BF16 = (1, 2, 32, 128, 3, 1), (1, 3, 33, 132, 3, 1)
DW_ROWS = [
    _dwrow("tile-scalar-w7", (2, 5, 9, 7, 3, 1), "fp32", lambda o, *s: s[3] % 4 != 0 and not wide_form(*s)),
    ROW_TILE_BORDER,
    _dwrow("tile-5", (2, 4, 37, 45, 5, 2), "fp32", lambda o, *s: s[4] == 5 and _tiles(*s) == 4, general=True),
    _dwrow("tile-7-map-smaller-than-its-halo", (1, 3, 4, 4, 7, 3), "fp32", lambda o, *s: s[4] == 7 and s[2] < s[4] and s[3] < s[4] and dw_out(*s) == (4, 4)),
    _dwrow("pad-0", (2, 4, 10, 12, 3, 0), "fp32", lambda o, *s: s[5] == 0 and dw_out(*s) == (8, 10)),
    _dwrow("pad-full-border", (1, 3, 6, 8, 5, 4), "fp32", lambda o, *s: s[5] == s[4] - 1 and dw_out(*s) == (10, 12), border=True, general=True),
    _dwrow("wide-fp32", WIDE_F32, "fp32", lambda o, *s: wide_form(*s) and s[2] == HT and s[3] == 2 * WT),
    _dwrow("wide-bf16-border-ragged-both-ways", WIDE_BF16, "bf16", lambda o, *s: wide_form(*s) and s[2] % HT and s[3] % WT, border=True, general=True),
    _dwrow("wide-not-taken-h31", (1, 2, 31, 128, 3, 1), "fp32", lambda o, *s: not wide_form(*s) and wide_form(s[0], s[1], s[2] + 1, *s[3:])),
    _dwrow("wide-not-taken-w124", (1, 2, 32, 124, 3, 1), "fp32", lambda o, *s: not wide_form(*s) and wide_form(*s[:3], s[3] + 4, *s[4:])),
    _dwrow("stats-tile", (2, 8, 16, 16, 3, 1), "bf16", lambda o, *s: not wide_form(*s), stats=True, launches=_DW_STATS, general=True),
    _dwrow("stats-wide", WIDE_F32, "fp32", lambda o, *s: wide_form(*s), stats=True, launches=_DW_STATS),
    _dwrow("stats-asked-border-takes-the-plain-launch", (2, 8, 16, 16, 3, 1), "bf16", lambda o, *s: s[4] == 3 and s[5] == 1, border=True, stats=True),
    _dwrow("stats-asked-k5-takes-the-plain-launch", (2, 4, 37, 45, 5, 2), "fp32", lambda o, *s: s[4] != 3, stats=True),
    _dwrow("wgrad-walk-3-workgroups-over-4-tiles", (4, 685, 33, 33, 3, 1), "bf16", lambda o, *s: wgrad_walk(*s) == (3, 4), border=True, general=True),
    _dwrow("wgrad-walk-7x7-3-workgroups-over-4-tiles", (2, 1370, 33, 33, 7, 3), "fp32", lambda o, *s: wgrad_walk(*s) == (3, 4)),
]


def _dw_case(ops, switches, census, shape, kind, border, stats, on_route, launches, seed, exact):
    N, C, H, W, K, pad = shape
    assert on_route(ops, *shape)
    wants_part = "dwconv_fwd_stats" in launches
    if stats:
        single_pass_switch(ops, switches, N, C, H * W)
    draw = draw_dw(shape, kind, seed, border, exact)
    sums = conv_ref.abs_sums(conv_ref.dwconv, draw[0], draw[1], pad, draw[2], draw[3])
    if exact:
        assert_sums_exact(sums)
    got, part, launched = run_dw(ops, census, shape, kind, draw, stats=stats)
    assert launched == launches, launched
    assert census["dwconv_bwd_weight"][0][10] == 0          # accumulate: there is no sink
    if wants_part:
        P = int(ops.lib.s2f_dwconv_stats_slots(N, H, W))
        assert P == N * (cdiv(W, WT) * cdiv(H, HT) if wide_form(*shape) else cdiv(W, TS) * cdiv(H, TS))
        assert_partials(part, got["y"], P, WT * HT if wide_form(*shape) else TS * TS, exact)
        plain, none, _ = run_dw(ops, census, shape, kind, draw, stats=False)
        assert none is None and torch.equal(plain["y"], got["y"])
    else:
        assert part is None
    return draw, sums, got


@pytest.mark.parametrize("shape,kind,border,stats,on_route,launches,general", DW_ROWS)
def test_dwconv_route_equals_fp64(ops, switches, census, shape, kind, border, stats, on_route, launches, general):
    draw, _, got = _dw_case(ops, switches, census, shape, kind, border, stats, on_route, launches, sum(shape) + int(border), True)
    assert_equal64(got, conv_ref.dwconv(draw[0], draw[1], shape[5], draw[2], draw[3]), DW)


@pytest.mark.parametrize("shape,kind,border,stats,on_route,launches,general", [r for r in DW_ROWS if r.values[-1]])
def test_dwconv_route_general_operands_within_the_fp32_bound(ops, switches, census, shape, kind, border, stats, on_route, launches, general):
    K = shape[4]
    draw, sums, got = _dw_case(ops, switches, census, shape, kind, border, stats, on_route, launches, sum(shape) + 1000, False)
    args = (draw[0], draw[1], shape[5], draw[2], draw[3])
    assert_within("dwconv " + "x".join(map(str, shape)) + (" border" if border else "") + (" stats" if stats else ""), got,
                  conv_ref.dwconv(*args), conv_ref.dwconv(*args, torch.float32), sums,
                  {"y": K * K * 2.0 ** -24, "dx": K * K * 2.0 ** -24, "dw": 2e-5}, DW)


def test_dwconv_weight_gradient_adds_into_its_sink(ops, switches, census):
    """tile-vector-border through a sink pre-filled with 0.75: s2f_dwconv_bwd_weight with accumulate = 1 (no zero fill) leaves
    dw + 0.75 exactly, and autograd gets no tensor for the weight"""
    shape, kind, border, _, on_route, launches, _ = ROW_TILE_BORDER.values
    assert on_route(ops, *shape)
    draw = draw_dw(shape, kind, 53, border, True)
    assert_sums_exact(conv_ref.abs_sums(conv_ref.dwconv, draw[0], draw[1], shape[5], draw[2], draw[3]))
    ref = conv_ref.dwconv(draw[0], draw[1], shape[5], draw[2], draw[3])
    w = torch.nn.Parameter(draw[1].float().cuda())
    with _Sink(ops, w) as sink:
        got, _, launched = run_dw(ops, census, shape, kind, draw, w=w)
        assert launched == launches, launched
        args = census["dwconv_bwd_weight"][0]
        assert args[10] == 1 and args[3] == sink.view.data_ptr()
        assert w.grad is None and got["dw"] is None
        sink.holds(ref["dw"] + 0.75)
        assert_equal64(got, ref, ("y", "dx"))
