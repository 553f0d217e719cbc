"""csrc/glue.hip and its two front ends on the GPU.

Section 1: the default-path kernels (ops.mean_all, channel_sum, sum_lead, fan_out, the 2x up-sampling's pass-through adjoint) against
fp64 or the engine's own sums.  Section 2: every route of ops.GlueMode against eager ATen on the same inputs -- bit for bit for the
element-wise, copy, fill and shape routes; the sums against fp64.

Tolerance rule for every sum: per output |got - ref| <= gamma(B) * sum|x|, gamma(B) = B u / (1 - B u), u = 2^-24, where B bounds the
number of roundings any addend meets in the kernel's own order of additions (longest serial chain per lane + wave and block trees +
the serial chain of the final pass), computed from the kernel's partitioning.  Outliers are planted on partition boundaries, each ten
times the bound computed without them, so a dropped or doubled element or range fails."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

aten = torch.ops.aten
U = 2.0 ** -24
WORST = {}


def gamma(B):
    return B * U / (1 - B * U)


def _lib():
    from spike2former_amd._lib import lib
    return lib


def report(form, err, absum):
    """worst error of a kernel form in units of 2^-24 sum|x| (printed: quoted in the change's description)"""
    e = float((err / (U * absum)).max())
    WORST[form] = max(WORST.get(form, 0.0), e)
    print(f"[glue] {form}: worst |err| = {WORST[form]:.3f} x 2^-24 sum|x|")


def check_sum(got, ref, absum, B, form):
    got, ref, absum = got.double().reshape(-1).cpu(), ref.double().reshape(-1).cpu(), absum.double().reshape(-1).cpu()
    err = (got - ref).abs()
    bad = err > gamma(B) * absum
    assert not bool(bad.any()), (form, B, int(bad.nonzero()[0]), float((err / (U * absum)).max()))
    report(form, err, absum)


def plant(y, cols, B):
    """y [n_out, n_red] fp32 (in place): positive outliers at the reduced positions `cols`, each > 10 gamma(B) sum|row|"""
    s = y.double().abs().sum(1)
    o = (10 * gamma(B) * s * 1.01 + 4.0).float()
    for k, j in enumerate(sorted(set(cols))):
        y[:, j] = o * (1 + 0.25 * k)
    return y


# ============================================================================================== section 1: the default-path kernels
PER_BLOCK = 16384          # glue.hip kPerBlock: elements per workgroup of s2f_sum_all


def _mean_all_bound(n):
    # a full workgroup: 16 float4 per lane, (x + y) + (z + w) then the lane's chain of 16; a tail workgroup: <= 64 elements per lane;
    # + 6 (wave tree) + 4 (thread 0 adds the four waves); the final pass adds the partials in fp64 (+1 covers it), then the fp32
    # scale 1/n and the product's rounding: +2
    full = 2 + 16 if n >= PER_BLOCK else 0
    tail = math.ceil((n % PER_BLOCK) / 256)
    return max(full, tail) + 6 + 4 + 1 + 2


def _mean_data(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, device="cuda", generator=g) + 1.0
    return plant(x.view(1, n), [0, min(PER_BLOCK, n - 1), n - 1], _mean_all_bound(n)).view(n)


def _mean_ref(x):
    xd = x.double()
    return xd.sum() / x.numel(), xd.abs().sum() / x.numel()


@pytest.mark.parametrize("n", [1, 3, 4, 16383, 16384, 16385, 5 * 2 ** 20 + 7, 2 ** 25 + 3])
def test_mean_all_vs_fp64(n):
    """ops.mean_all (s2f_sum_all) over a contiguous tensor: within the bound of its order, bit-repeatable; the backward fills
    float32(g) * float32(1/n) with x's strides"""
    from spike2former_amd import ops
    assert int(_lib().s2f_sum_all_parts(n)) == math.ceil(n / PER_BLOCK)
    x = _mean_data(n, n)
    got = ops.mean_all(x)
    ref, absum = _mean_ref(x)
    check_sum(got, ref, absum, _mean_all_bound(n), "s2f_sum_all (mean_all)")
    assert torch.equal(got.view(1).view(torch.int32), ops.mean_all(x).view(1).view(torch.int32))
    xl = x.detach().requires_grad_(True)
    seen = []
    xl.register_hook(lambda g: seen.append(g))
    ops.mean_all(xl).backward(torch.tensor(0.7, device="cuda"))
    gx = seen[0]
    want = np.float32(0.7) * np.float32(1.0 / n)
    assert gx.stride() == xl.stride()
    assert bool((gx.view(torch.int32) == int(np.array(want).view(np.int32))).all())


@pytest.mark.parametrize("shape,perm", [((7, 16384, 3), (2, 0, 1)), ((5, 1024, 1024), (1, 2, 0)), ((3, 5461), (1, 0))])
def test_mean_all_permuted_view_takes_the_kernel(shape, perm):
    """a permuted dense view sums the memory it covers: the same bits as the contiguous tensor (the kernel path); its gradient has
    the view's strides"""
    from spike2former_amd import ops
    n = int(np.prod(shape))
    x = _mean_data(n, 7 + n).view(shape)
    v = x.permute(perm)
    got = ops.mean_all(v)
    assert torch.equal(got.view(1).view(torch.int32), ops.mean_all(x).view(1).view(torch.int32))
    ref, absum = _mean_ref(x)
    check_sum(got, ref, absum, _mean_all_bound(n), "s2f_sum_all (mean_all)")
    vl = v.detach().requires_grad_(True)
    seen = []
    vl.register_hook(lambda g: seen.append(g))
    ops.mean_all(vl).backward(torch.tensor(-1.5, device="cuda"))
    assert seen[0].stride() == vl.stride()
    want = np.float32(-1.5) * np.float32(1.0 / n)
    assert bool((seen[0].view(torch.int32) == int(np.array(want).view(np.int32))).all())


@pytest.mark.parametrize("n", [16385, 5 * 2 ** 20 + 7])
def test_mean_all_aten_layouts(n):
    """a storage offset of 1 (misaligned) and an expanded view take ATen's mean: still the mean (ATen's tree reduction: an empirical
    ceiling of 256 roundings, below the planted outliers)"""
    from spike2former_amd import ops
    base = torch.empty(n + 1, device="cuda")
    base[1:] = _mean_data(n, 3 * n)
    x = base[1:]
    assert x.data_ptr() % 16 != 0
    ref, absum = _mean_ref(x)
    check_sum(ops.mean_all(x), ref, absum, 256, "ATen mean (misaligned)")
    row = _mean_data(4096, 5).view(1, 4096)
    e = row.expand(n // 4096, 4096)
    ref, absum = _mean_ref(e.contiguous())
    check_sum(ops.mean_all(e), ref, absum, 256, "ATen mean (expanded)")


def _channel_sum_bound(N, C, L):
    S = int(_lib().s2f_channel_sum_slices(N, C, L))
    # lane: ceil(N / S) rows x ceil(L / 4 / 256) float4 steps, each float4 summed as (x + y) + (z + w): +2; wave 6, block 4;
    # the final pass adds the S slices in order: S
    return math.ceil(N / S) * math.ceil(L / 4 / 256) + 2 + 6 + 4 + S, S


@pytest.mark.parametrize("N,C,L", [(1, 1, 4), (1, 2049, 4), (8, 1, 4096), (300, 3, 1028), (1, 800, 16384), (8, 256, 1024)])
def test_channel_sum_vs_fp64(N, C, L):
    """ops.channel_sum (s2f_channel_sum) against the fp64 x.sum((0, 2)): shapes across s2f_channel_sum_slices (S capped by N or
    by 2048 / C); a non-contiguous input; bit-repeatable"""
    from spike2former_amd import ops
    B, S = _channel_sum_bound(N, C, L)
    g = torch.Generator(device="cuda").manual_seed(N * C + L)
    y = torch.randn(C, N * L, device="cuda", generator=g) + 0.5
    # rows n = 0, min(S, N - 1) (the next slice's first row) and N - 1; columns 0, 1024 (a lane's second float4 step), L - 1
    pos = [0 * L + 0, min(S, N - 1) * L + min(1024, L - 1), (N - 1) * L + L - 1]
    plant(y, pos, B)
    x = y.view(C, N, L).permute(1, 0, 2)          # [N, C, L], non-contiguous
    ref, absum = y.double().sum(1), y.double().abs().sum(1)
    xc = x.contiguous()
    got = ops.channel_sum(xc)
    check_sum(got, ref, absum, B, "s2f_channel_sum")
    assert torch.equal(got.view(torch.int32), ops.channel_sum(xc).view(torch.int32))
    assert torch.equal(ops.channel_sum(x).view(torch.int32), got.view(torch.int32))


def test_channel_sum_unaligned_rows_take_aten():
    """L % 4 != 0: ATen's sum, still the sum"""
    from spike2former_amd import ops
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(4, 8, 1030, device="cuda", generator=g)
    check_sum(ops.channel_sum(x), x.double().sum((0, 2)), x.double().abs().sum((0, 2)), 4 * 1030, "ATen channel sum")


@pytest.mark.parametrize("T", [1, 2, 4, 8])
@pytest.mark.parametrize("M", [4, 260, 2 ** 20])
def test_sum_lead_is_the_sequential_sum(T, M):
    """ops.sum_lead (s2f_sum_lead) adds x[0] + x[1] + ... in that order: bit for bit the sequential ATen adds"""
    from spike2former_amd import ops
    g = torch.Generator(device="cuda").manual_seed(T * M)
    x = torch.randn(T, M, device="cuda", generator=g) * torch.logspace(-3, 3, T, device="cuda").view(T, 1)
    want = x[0].clone()
    for t in range(1, T):
        want = want + x[t]
    assert torch.equal(ops.sum_lead(x).view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("N,C,h,w", [(2, 3, 8, 16), (2, 3, 4, 6), (1, 2, 5, 8), (1, 3, 7, 10)])
def test_upsample2x_pass_through_port(N, C, h, w):
    """ops.upsample_bilinear(x, (2h, 2w), skip=True): the second reader's gradient summed inside the 2x adjoint
    (s2f_upsample2x_bwd_add; float4 form for w % 4 == 0 and even h, else the scalar form) -- ports on == ports off bit for bit, and
    within 2e-6 of the CPU F.interpolate adjoint plus the pass-through gradient"""
    from spike2former_amd import ops
    g = torch.Generator().manual_seed(N * 100 + h * 10 + w)
    x = torch.randn(N, C, h, w, generator=g)
    gy = torch.randn(N, C, 2 * h, 2 * w, generator=g) * 0.25
    gs = torch.randn(N, C, h, w, generator=g) * 0.25
    out = []
    for on in (False, True):
        was = ops.FANOUT_PORTS
        ops.FANOUT_PORTS = on
        try:
            xc = x.cuda().requires_grad_(True)
            y, xs = ops.upsample_bilinear(xc, (2 * h, 2 * w), skip=True)
            assert (xs is not xc) == on
            ((y * gy.cuda()).sum() + (xs * gs.cuda()).sum()).backward()
            out.append(xc.grad.cpu())
        finally:
            ops.FANOUT_PORTS = was
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))
    xd = x.double().requires_grad_(True)
    F.interpolate(xd, scale_factor=2, mode="bilinear", align_corners=False).backward(gy.double())
    assert (out[1].double() - (xd.grad + gs.double())).abs().max().item() <= 2e-6


def _port_transpose(ops, x):
    return ops.transpose_last2(x, skip=True)


def _port_up2x(ops, x):
    return ops.upsample_bilinear(x, (2 * x.shape[-2], 2 * x.shape[-1]), skip=True)


PORT_OPS = {
    "transpose_16B_ragged": (_port_transpose, (2, 65, 68)),          # 16-byte form, ragged against the 64 x 64 tile both ways
    "transpose_scalar": (_port_transpose, (2, 5, 7)),
    "up2x_float4": (_port_up2x, (1, 2, 4, 8)),
    "up2x_scalar": (_port_up2x, (1, 2, 3, 6)),
    "resize": (lambda ops, x: ops.resize_bilinear(x, (9, 4), align_corners=False, skip=True), (1, 2, 5, 7)),
    "resize_align_corners": (lambda ops, x: ops.resize_bilinear(x, (9, 4), align_corners=True, skip=True), (1, 2, 5, 7)),
}


@pytest.mark.parametrize("pattern", ["both", "y_only", "through_only"])
@pytest.mark.parametrize("name", list(PORT_OPS))
def test_pass_through_port_gradient_patterns(name, pattern):
    """The three ops that share the pass-through protocol (transpose_last2, the exact-2x upsample_bilinear, resize_bilinear; skip=True)
    with a gradient on both outputs, on y alone and on the pass-through alone: the input gradient with ops.FANOUT_PORTS on equals the
    one with it off bit for bit.  Only y: both settings run the same adjoint kernel with a null addend; only the pass-through: both
    return the incoming gradient; both: the adjoint kernel's sum is the engine's."""
    from spike2former_amd import ops
    op, shape = PORT_OPS[name]
    g = torch.Generator().manual_seed(len(name) * 7 + len(pattern))
    x = torch.randn(shape, generator=g)
    out = []
    for on in (False, True):
        was = ops.FANOUT_PORTS
        ops.FANOUT_PORTS = on
        try:
            xc = x.cuda().requires_grad_(True)
            y, xs = op(ops, xc)
            assert (xs is not xc) == on
            if not out:
                gy = (torch.randn(y.shape, generator=g) * 0.25).cuda()
                gs = (torch.randn(shape, generator=g) * 0.25).cuda()
            loss = 0.0
            if pattern != "through_only":
                loss = loss + (y * gy).sum()
            if pattern != "y_only":
                loss = loss + (xs * gs).sum()
            loss.backward()
            out.append(xc.grad.cpu())
        finally:
            ops.FANOUT_PORTS = was
    assert torch.isfinite(out[0]).all() and out[0].abs().max().item() > 0
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))


# ============================================================================================== section 2: every GlueMode route
def _g():
    from spike2former_amd import ops
    return ops, ops.glue


SPECIALS = [0.0, -0.0, math.inf, -math.inf, math.nan, 1.4e-45, -1.4e-45, 3.4028234663852886e38, -3.4028234663852886e38,
            1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, -(1.0 + 2.0 ** -23)]


def vals(shape, seed):
    """random normals with the planted IEEE specials at the first and the last positions (rotated by seed)"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(shape, generator=g)
    f = v.view(-1)
    k = min(f.numel(), len(SPECIALS))
    for i in range(k):
        f[i] = SPECIALS[(i + seed) % len(SPECIALS)]
        f[f.numel() - 1 - i] = SPECIALS[(i + 2 * seed + 5) % len(SPECIALS)]
    return v


def lay(v, kind, dtype=torch.float32):
    """the logical CPU tensor v as a CUDA tensor of the layout `kind`"""
    if kind == "cpu":           # a host scalar as a 0-dim fp64 CPU tensor (ATen rounds it to fp32)
        return torch.tensor(0.3, dtype=torch.float64)
    if kind == "perm":          # [A, B, C] viewing [C, A, B] memory: the strided kernel
        A, B, C = v.shape
        t = torch.empty(C, A, B, dtype=dtype, device="cuda").permute(1, 2, 0)
    elif kind == "inner4":      # innermost contiguous, % 4 == 0, outer strides and offset multiples of 4: the float4 strided kernel
        A, B, C = v.shape
        t = torch.empty(A, B + 2, C + 8, dtype=dtype, device="cuda")[:, 1:1 + B, 4:4 + C]
    elif kind == "off1":        # storage offset 1: misaligned
        t = torch.empty(v.numel() + 1, dtype=dtype, device="cuda")[1:].view(v.shape)
    elif kind == "rev":         # every dimension reversed in memory: nothing coalesces
        nd = v.dim()
        t = torch.empty(tuple(reversed(v.shape)), dtype=dtype, device="cuda").permute(tuple(reversed(range(nd))))
    elif kind == "bcast":       # v [A, 1, C] expanded to [A, 6, C]: a stride-0 input
        return v.to(dtype).cuda().expand(v.shape[0], 6, v.shape[2])
    else:
        t = torch.empty(v.shape, dtype=dtype, device="cuda")
    t.copy_(v.to(dtype).cuda())
    return t


# layout -> operand specs (logical shape, kind); a binary op uses the first two, a ternary one all three
LAYOUTS = {
    "flat%4=0": [((1024,), "flat")] * 3,
    "flat%4=1": [((1025,), "flat")] * 3,
    "flat%4=3": [((1027,), "flat")] * 3,
    "permuted": [((6, 7, 10), "perm"), ((6, 7, 10), "flat"), ((6, 7, 10), "perm")],
    "inner4": [((5, 6, 12), "inner4")] * 3,
    "offset1": [((7, 9, 11), "off1"), ((7, 9, 11), "flat"), ((7, 9, 11), "off1")],
    "broadcast": [((5, 1, 8), "flat"), ((1, 6, 8), "flat"), ((5, 6, 1), "flat")],
    "0-dim cuda": [((5, 6, 7), "flat"), ((), "flat"), ((), "flat")],
    "0-dim cpu": [((5, 6, 7), "flat"), ((), "cpu")],
    "ones": [((1, 1, 1), "flat")] * 3,
    "6-D": [((2, 3, 2, 3, 2, 3), "rev"), ((2, 3, 2, 3, 2, 3), "flat"), ((2, 3, 2, 3, 2, 3), "rev")],
    "7-D": [((2,) * 7, "flat")] * 3,
}
UNARY = ["flat%4=0", "flat%4=1", "flat%4=3", "permuted", "inner4", "offset1", "broadcast", "ones", "6-D", "7-D"]
BINARY = [k for k in LAYOUTS]
TERNARY = [k for k in LAYOUTS if k != "0-dim cpu"]
INPLACE = [k for k in LAYOUTS if k != "broadcast"] + ["broadcast into"]


def operands(layout, arity, dtype=torch.float32):
    if layout == "broadcast into":          # an in-place destination [5, 6, 8] with a broadcast second operand [1, 6, 1]
        specs = [((5, 6, 8), "flat"), ((1, 6, 1), "flat")]
    elif layout == "broadcast" and arity == 1:
        specs = [((5, 1, 8), "bcast")]
    else:
        specs = LAYOUTS[layout][:arity]
    return [lay(vals(s, 3 * i + len(layout)), k, dtype if i == 0 else torch.float32) for i, (s, k) in enumerate(specs)]


def _host(t):
    return t.detach().contiguous().cpu() if torch.is_tensor(t) else t


def assert_bitwise(got, want, what=""):
    """int32 bit views equal (+0 and -0 differ); NaN matches NaN whatever its payload"""
    assert torch.is_tensor(got) and tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (what, got, want)
    a, b = _host(got), _host(want)
    if a.dtype == torch.float32:
        same = (a.view(torch.int32) == b.view(torch.int32)) | (a.isnan() & b.isnan())
    else:
        same = a == b
    if not bool(same.all()):
        i = int((~same).view(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int((~same).sum())} of {a.numel()} differ; first at {i}: glue {a.view(-1)[i].item()!r} "
                             f"ATen {b.view(-1)[i].item()!r}")


def glue_run(op, args, kw=None):
    """op(*args, **kw) under GlueMode: it must be routed (ROUTED grew, nothing UNROUTED)"""
    ops, G = _g()
    torch.cuda.synchronize()
    G.reset_counts()
    with ops.glue_mode(force=True):
        out = op(*args, **(kw or {}))
    torch.cuda.synchronize()
    assert G.ROUTED[str(op)] >= 1 and not G.UNROUTED, (str(op), dict(G.ROUTED), dict(G.UNROUTED))
    return out


def host_scalar_sum(op, args, kw):
    """t + alpha * s for a host scalar s and alpha != 1: ATen's own bits depend on its kernel -- its vectorised loop hoists the
    rounded product alpha * s, its strided and tail loops fuse it into the add -- so the reference is the IEEE sum of t and the fp32
    product, which the glue gives on every layout (the printed count: elements where eager ATen has the fused bits)"""
    t, sc = args[0], args[1]
    sign = -1.0 if op in (aten.sub.Tensor, aten.sub.Scalar) else 1.0
    p = np.float32(np.float32(kw["alpha"]) * np.float32(float(sc)))
    want = aten.add.Tensor(t.clone(), torch.tensor(sign * float(p), device="cuda"))
    eager = op(*args, **kw)
    differ = ~((_host(eager).view(torch.int32) == _host(want).view(torch.int32)) | (_host(eager).isnan() & _host(want).isnan()))
    print(f"[glue] {op} host scalar, alpha {kw['alpha']}: eager ATen differs from the rounded-product sum in {int(differ.sum())} "
          f"of {t.numel()} elements ({tuple(t.stride())})")
    return want


def both(op, make, kw=None, what=""):
    """eager ATen and GlueMode on identical fresh inputs; bitwise"""
    args = make()
    if (kw or {}).get("alpha", 1) != 1 and len(args) > 1 and not (torch.is_tensor(args[1]) and args[1].is_cuda):
        want = host_scalar_sum(op, args, kw)
    else:
        want = op(*args, **(kw or {}))
    got = glue_run(op, make(), kw)
    assert_bitwise(got, want, f"{op} {what} {kw or ''}")
    return got, want


def unrouted(op, make, kw=None):
    """7-D operands: not routed -- counted in UNROUTED, and an error under STRICT_GLUE"""
    ops, G = _g()
    G.reset_counts()
    with ops.glue_mode(force=True):
        op(*make(), **(kw or {}))
    assert G.UNROUTED[str(op)] >= 1 and not G.ROUTED[str(op)], (str(op), dict(G.ROUTED), dict(G.UNROUTED))
    strict = ops.STRICT_GLUE
    ops.STRICT_GLUE = True
    try:
        with pytest.raises(RuntimeError, match="STRICT_GLUE"):
            with ops.glue_mode(force=True):
                op(*make(), **(kw or {}))
    finally:
        ops.STRICT_GLUE = strict


def ew_case(op, arity, layouts, kws=({},), scalars=None, dtype=torch.float32):
    """an element-wise route over its layouts (x every kwargs set); `scalars`: the second operand is each of these host scalars"""
    def run():
        for layout in layouts:
            for kw in kws:
                for s in (scalars or [None]):
                    def make(layout=layout, s=s):
                        t = operands(layout, arity if s is None else 1, dtype)
                        return t if s is None else t + [s]
                    if layout == "7-D":
                        unrouted(op, make, kw)
                    else:
                        both(op, make, kw, f"[{layout}{'' if s is None else f', {s!r}'}]")
    return run


def scalar_first_case(op, kws=({},)):
    """the host scalar as the FIRST operand (a 0-dim CPU tensor): ATen's `s + t * alpha` / `s * t`"""
    def run():
        for kw in kws:
            both(op, lambda: [torch.tensor(0.3, dtype=torch.float64), lay(vals((5, 6, 7), 1), "perm")], kw, "[scalar first]")
    return run


def chain(*fs):
    def run():
        for f in fs:
            f()
    return run


ALPHAS = ({}, {"alpha": 2.5})
SCALARS = [0.7, -3, 0.0, 1e-3]
DIVISORS = [3.0, 0.1, -7, 0.0]


def copy_case():
    for layout in ["flat%4=0", "flat%4=3", "permuted", "inner4", "offset1", "ones", "6-D"]:
        (shape, kind) = LAYOUTS[layout][0]
        for src_dtype in (torch.float32, torch.bfloat16):
            both(aten.copy_.default, lambda: [lay(vals(shape, 1), kind), lay(vals(shape, 2), "flat", src_dtype)], what=f"[{layout} {src_dtype}]")
            both(aten.copy_.default, lambda: [lay(vals(shape, 1), "flat"), lay(vals(shape, 2), kind, src_dtype)], what=f"[from {layout} {src_dtype}]")
    # broadcast source
    both(aten.copy_.default, lambda: [lay(vals((5, 6, 8), 1), "perm"), lay(vals((6, 1), 2), "flat")], what="[broadcast source]")
    unrouted(aten.copy_.default, lambda: [lay(vals((2,) * 7, 1), "flat"), lay(vals((2,) * 7, 2), "flat")])


def to_copy_case():
    for dt in (torch.bfloat16, torch.float32):
        ew_case(aten._to_copy.default, 1, UNARY, kws=({"dtype": torch.float32},), dtype=dt)()


def clone_case():
    ew_case(aten.clone.default, 1, UNARY)()
    ew_case(aten.clone.default, 1, ["permuted", "inner4"], kws=({"memory_format": torch.contiguous_format},))()


FILL_TARGETS = {"contiguous": ((33, 31), "flat"), "permuted": ((6, 7, 10), "perm"), "sliced": ((5, 6, 12), "inner4"),
                "offset1": ((7, 9, 11), "off1"), "6-D": ((2, 3, 2, 3, 2, 3), "rev")}


def fill_case(op, args=()):
    def run():
        for name, (shape, kind) in FILL_TARGETS.items():
            for a in (args or [()]):
                got, _ = both(op, lambda: [lay(vals(shape, 4), kind)] + list(a), what=f"[{name}]")
        unrouted(op, lambda: [lay(vals((2,) * 7, 4), "flat")] + list((args or [()])[0]))
    return run


def new_case(op, args_list):
    def run():
        for args, kw in args_list:
            both(op, lambda: list(args), dict(kw, device="cuda"), what=str(args))
    return run


def like_case(op):
    def run():
        for name, (shape, kind) in FILL_TARGETS.items():
            got, want = both(op, lambda: [lay(vals(shape, 5), kind)], what=f"[{name}]")
            assert got.stride() == want.stride(), (name, got.stride(), want.stride())
        x4 = lambda: [lay(vals((2, 6, 5, 4), 5), "flat")]          # noqa: E731
        for mf in (torch.channels_last, torch.contiguous_format, torch.preserve_format):
            got, want = both(op, x4, {"memory_format": mf}, what=str(mf))
            assert got.stride() == want.stride(), (mf, got.stride(), want.stride())
    return run


# ---------------------------------------------------------------------------------------------- sums and means (fp64, not bitwise)
def _red_pieces(n_out, n_red, cols):          # glue.hip red_pieces
    if n_out >= 16384:
        return 1
    S = min(math.ceil(16384 / n_out), math.ceil(n_red / (16 if cols else 64)))
    return min(max(S, 1), 8192)


def _reduce_form(x, dims):
    """(form, S, B) of s2f_reduce_sum for x summed over dims, as glue.hip chooses it"""
    nd = x.dim()
    dims = sorted(d % nd for d in dims) if dims else list(range(nd))
    keep = [d for d in range(nd) if d not in dims]
    n_out = int(np.prod([x.shape[d] for d in keep])) if keep else 1
    n_red = int(np.prod([x.shape[d] for d in dims]))
    assert int(_lib().s2f_reduce_sum_workspace(n_out, n_red)) == max(_red_pieces(n_out, n_red, False),
                                                                       _red_pieces(n_out, n_red, True)) * n_out
    cols = bool(keep) and x.stride(keep[-1]) == 1 and n_out >= 256
    S = _red_pieces(n_out, n_red, cols)
    chunk = math.ceil(n_red / S)
    # rows: lanes stride the piece (ceil(chunk / 64)), wave tree 6; cols: one lane walks the piece serially; final: lanes stride the
    # S partials (ceil(S / 64)), wave tree 6
    B = (chunk if cols else math.ceil(chunk / 64) + 6) + (math.ceil(S / 64) + 6 if S > 1 else 0)
    form = f"s2f_reduce_sum {'cols' if cols else 'rows'} {'S=1' if S == 1 else 'S>1'}"
    return form, S, chunk, B, keep, dims, n_out, n_red


def arrange(y, shape, keep, dims):
    """y [n_out, n_red] as a tensor of `shape` whose kept / reduced dims flatten (row-major) to y's two axes"""
    order = keep + dims
    return y.view([shape[d] for d in order]).permute(tuple(int(i) for i in np.argsort(order)))


REDUCTIONS = [          # (shape, dims, keepdim, transposed input)
    ((3, 100000), [1], False, False),            # rows, S > 1, long pieces
    ((2 ** 20,), [0], False, False),             # rows, S at the 8192-piece cap
    ((300, 4096), [1], False, False),            # rows: >= 256 outputs with a non-unit output stride
    ((16384, 40), [1], False, False),            # rows, S == 1
    ((2048, 512), [0], False, False),            # cols, S > 1
    ((1024, 16384), [0], False, False),          # cols, S == 1: one lane sums 1024 elements serially
    ((12, 40, 9), [0, 2], False, False),         # two reduced dimensions that are not adjacent
    ((6, 50, 70), [-1], True, False),            # keepdim, negative dim
    ((300, 70), [], False, False),               # dim=[]: everything, 0-dim output
    ((300, 500), [1], False, True),              # transposed input
    ((4, 8, 16, 16), [0, 2, 3], True, False),    # a bias gradient's sum
]


def reduce_case(op, mean):
    def run():
        ops, G = _g()
        for shape, dims, keepdim, transposed in REDUCTIONS:
            full = op in (aten.sum.default, aten.mean.default)
            if full and keepdim:
                continue
            g = torch.Generator(device="cuda").manual_seed(len(shape) * 1000 + sum(shape))
            x0 = torch.empty(shape, device="cuda")
            form, S, chunk, B, keep, rdims, n_out, n_red = _reduce_form(x0, [] if full else dims)
            if transposed:
                x0 = x0.t().contiguous().t()
                form, S, chunk, B, keep, rdims, n_out, n_red = _reduce_form(x0, [] if full else dims)
            B += 2 if mean else 0          # (the fp32 scale 1/n and the product's rounding)
            y = torch.randn(n_out, n_red, device="cuda", generator=g) + 0.5
            plant(y, [0, min(chunk, n_red - 1), n_red - 1], B)
            xl = arrange(y, shape, keep, rdims)
            x = xl.t().contiguous().t() if transposed else xl.contiguous()
            args = [x] if full else [x, dims, keepdim]
            want = op(*args)
            got = glue_run(op, args)
            assert got.shape == want.shape, (shape, dims, got.shape, want.shape)
            again = glue_run(op, args)
            assert torch.equal(got.reshape(-1).view(torch.int32), again.reshape(-1).view(torch.int32))
            ref, absum = y.double().sum(1), y.double().abs().sum(1)
            if mean:
                ref, absum = ref / n_red, absum / n_red
            check_sum(got, ref, absum, B, form)
            ea = ((want.double().reshape(-1).cpu() - ref.cpu()).abs() / (U * absum.cpu())).max().item()
            print(f"[glue] {op} {shape} dims={dims}: {form}, B={B}, ATen's error {ea:.3f} x 2^-24 sum|x|")
    return run


# ---------------------------------------------------------------------------------------------- the shape routes
def cat_case():
    P = lambda shapes, kind="flat": lambda: [[lay(vals(s, i + 1), kind) for i, s in enumerate(shapes)]]  # noqa: E731
    both(aten.cat.default, P([(4, 8), (2, 8), (6, 8)]), what="[dim 0, segments]")
    both(aten.cat.default, P([(2, 6)] * 11), what="[dim 0, 11 pieces]")
    both(aten.cat.default, P([(3, 5), (2, 5), (1, 5)]), what="[numel % 4 != 0]")
    both(aten.cat.default, lambda: [[lay(vals((6, 7, 10), 1), "perm"), lay(vals((2, 7, 10), 2), "flat")]], what="[permuted piece]")
    for d in (1, -1):
        both(aten.cat.default, lambda: [[lay(vals((3, 4, 5), 1), "flat"), lay(vals((3, 4, 5), 2), "flat")], d], what=f"[dim {d}]")
    both(aten.cat.default, lambda: [[lay(vals((3, 4, 5), 1), "flat"), lay(vals((3, 2, 5), 2), "flat")], 1], what="[dim 1]")
    both(aten.cat.default, lambda: [[lay(vals((4, 8), 1), "flat"), torch.empty(0, device="cuda"), lay(vals((4, 8), 2), "flat")], 1],
         what="[legacy empty piece]")


def cat_out_case():
    for shapes, dim in (([(4, 8), (2, 8)], 0), ([(3, 4, 5), (3, 2, 5)], 1), ([(3, 5), (3, 5), (3, 5)], -1)):
        out_shape = list(shapes[0])
        out_shape[dim] = sum(s[dim] for s in shapes)
        pieces = lambda: [lay(vals(s, i + 1), "flat") for i, s in enumerate(shapes)]          # noqa: E731
        want = aten.cat.out(pieces(), dim, out=torch.full(out_shape, math.nan, device="cuda"))
        got = glue_run(aten.cat.out, [pieces(), dim], {"out": torch.full(out_shape, math.nan, device="cuda")})
        assert_bitwise(got, want, f"cat.out {shapes}")


def stack_case():
    for shape, dim in (((4, 8), 0), ((3, 5), 0), ((3, 4, 5), 1), ((3, 4, 5), -1), ((6, 7, 10), 2)):
        both(aten.stack.default, lambda: [[lay(vals(shape, i + 1), "flat") for i in range(3)], dim], what=f"[{shape} dim {dim}]")
    both(aten.stack.default, lambda: [[lay(vals((6, 7, 10), i + 1), "perm") for i in range(3)], 1], what="[permuted pieces]")


def pad_case():
    for pad, value in (([1, 2], 0.0), ([1, 2, 0, 3], 1.5), ([1, 1, 2, 2, 3, 3], -0.0), ([0, 0, 4, 0], 0)):
        both(aten.constant_pad_nd.default, lambda: [lay(vals((3, 5, 7), 1), "perm"), pad, value], what=str(pad))


def repeat_case():
    for shape, reps in (((3, 4), (2, 3)), ((3, 4), (2, 1, 3)), ((3, 4), (1, 1)), ((5,), (3, 2, 2)), ((2, 3, 4), (2, 1, 2))):
        both(aten.repeat.default, lambda: [lay(vals(shape, 1), "flat"), list(reps)], what=f"{shape} x {reps}")
    both(aten.repeat.default, lambda: [lay(vals((6, 7, 10), 1), "perm"), [2, 1, 1]], what="[permuted]")


def flip_case():
    for dims in ((2,), (0,), (0, 1), (0, 2), (-1,), (0, 1, 2), (-3, -1)):
        both(aten.flip.default, lambda: [lay(vals((4, 5, 6), 1), "flat"), list(dims)], what=str(dims))
        both(aten.flip.default, lambda: [lay(vals((6, 7, 10), 1), "perm"), list(dims)], what=f"[permuted] {dims}")
    # repeated dims: ATen's error, not routed
    ops, G = _g()
    x = lay(vals((4, 5, 6), 1), "flat")
    with pytest.raises(RuntimeError) as eager:
        aten.flip.default(x, [0, -3])
    G.reset_counts()
    with pytest.raises(RuntimeError) as glued:
        with ops.glue_mode(force=True):
            aten.flip.default(x, [0, -3])
    assert str(glued.value) == str(eager.value) and not G.ROUTED


def select_backward_case():
    for gshape, sizes, dim, index in (((5, 6), [4, 5, 6], 0, 2), ((4, 5), [4, 5, 6], -1, -1), ((4, 6), [4, 5, 6], 1, -3)):
        both(aten.select_backward.default, lambda: [lay(vals(gshape, 1), "flat"), sizes, dim, index], what=f"{sizes} {dim} {index}")


CASES = {
    aten.add.Tensor: chain(ew_case(aten.add.Tensor, 2, BINARY, ALPHAS), scalar_first_case(aten.add.Tensor, ALPHAS)),
    aten.add.Scalar: ew_case(aten.add.Scalar, 1, UNARY, ALPHAS, SCALARS),
    aten.add_.Tensor: ew_case(aten.add_.Tensor, 2, INPLACE, ALPHAS),
    aten.add_.Scalar: ew_case(aten.add_.Scalar, 1, UNARY[:-4] + UNARY[-3:], ALPHAS, SCALARS),
    aten.sub.Tensor: ew_case(aten.sub.Tensor, 2, BINARY, ALPHAS),
    aten.sub.Scalar: ew_case(aten.sub.Scalar, 1, UNARY, ALPHAS, SCALARS),
    aten.mul.Tensor: chain(ew_case(aten.mul.Tensor, 2, BINARY), scalar_first_case(aten.mul.Tensor)),
    aten.mul.Scalar: ew_case(aten.mul.Scalar, 1, UNARY, scalars=SCALARS),
    aten.mul_.Tensor: ew_case(aten.mul_.Tensor, 2, INPLACE),
    aten.mul_.Scalar: ew_case(aten.mul_.Scalar, 1, UNARY[:-4] + UNARY[-3:], scalars=SCALARS),
    aten.div.Tensor: ew_case(aten.div.Tensor, 2, BINARY),
    aten.div.Scalar: ew_case(aten.div.Scalar, 1, UNARY, scalars=DIVISORS),
    aten.div_.Tensor: ew_case(aten.div_.Tensor, 2, INPLACE),
    aten.div_.Scalar: ew_case(aten.div_.Scalar, 1, UNARY[:-4] + UNARY[-3:], scalars=DIVISORS),
    aten.neg.default: ew_case(aten.neg.default, 1, UNARY),
    aten.addcmul.default: ew_case(aten.addcmul.default, 3, TERNARY, ({}, {"value": 0.5})),
    aten.sigmoid.default: ew_case(aten.sigmoid.default, 1, UNARY),
    aten.sigmoid_backward.default: ew_case(aten.sigmoid_backward.default, 2, TERNARY),
    aten.clone.default: clone_case,
    aten.copy_.default: copy_case,
    aten._to_copy.default: to_copy_case,
    aten.zero_.default: fill_case(aten.zero_.default),
    aten.fill_.Scalar: fill_case(aten.fill_.Scalar, [(2.5,), (-0.0,), (math.inf,)]),
    aten.zeros.default: new_case(aten.zeros.default, [(([3, 5],), {}), (([2, 3, 4],), {"dtype": torch.float32})]),
    aten.ones.default: new_case(aten.ones.default, [(([3, 5],), {}), (([1027],), {})]),
    aten.full.default: new_case(aten.full.default, [(([3, 5], 0.1), {}), (([7, 9], -0.0), {}), (([4], math.nan), {})]),
    aten.zeros_like.default: like_case(aten.zeros_like.default),
    aten.ones_like.default: like_case(aten.ones_like.default),
    aten.sum.dim_IntList: reduce_case(aten.sum.dim_IntList, False),
    aten.sum.default: reduce_case(aten.sum.default, False),
    aten.mean.dim: reduce_case(aten.mean.dim, True),
    aten.mean.default: reduce_case(aten.mean.default, True),
    aten.cat.default: cat_case,
    aten.cat.out: cat_out_case,
    aten.stack.default: stack_case,
    aten.constant_pad_nd.default: pad_case,
    aten.repeat.default: repeat_case,
    aten.flip.default: flip_case,
    aten.select_backward.default: select_backward_case,
}


def test_every_handler_has_a_case():
    """a new GlueMode handler without a case here fails"""
    _, G = _g()
    assert set(CASES) == set(G.HANDLERS)


@pytest.mark.parametrize("op", list(CASES), ids=str)
def test_glue_route_vs_aten(op):
    """each route, run eagerly and under GlueMode on the same inputs: routed (never ATen against ATen) and ATen's bits -- or, for
    the sums, within the bound of the kernel's order and bit-repeatable"""
    CASES[op]()


# ---------------------------------------------------------------------------------------------- the defects, one test each
@pytest.mark.parametrize("junk", [math.nan, math.inf, -1.0])
def test_fill_never_reads_its_target(junk):
    """zero_ / fill_ on permuted and sliced views of a tensor holding NaN, Inf or -1: the value, never `target * 0` (NaN stays
    NaN, -1 * 0 = -0); the memory outside a sliced view is untouched"""
    for name, make in (("permuted", lambda: torch.full((6, 7, 10), junk, device="cuda").permute(2, 0, 1)),
                       ("sliced", lambda: torch.full((5, 8, 20), junk, device="cuda")[:, 1:7, 4:16]),
                       ("strided", lambda: torch.full((9, 10), junk, device="cuda")[::2, 1::3])):
        for op, args in ((aten.zero_.default, ()), (aten.fill_.Scalar, (2.5,))):
            t = make()
            got = glue_run(op, [t] + list(args))
            assert_bitwise(got, op(make(), *args), f"{op} {name} {junk}")
            if name == "sliced":
                base = t._base
                outside = torch.ones(base.shape, dtype=torch.bool, device="cuda")
                outside[:, 1:7, 4:16] = False
                assert_bitwise(base[outside], torch.full((int(outside.sum()),), junk, device="cuda"), "outside")


@pytest.mark.parametrize("op", [aten.zeros_like.default, aten.ones_like.default])
def test_like_of_a_permuted_tensor_after_a_nan_block(op):
    """zeros_like / ones_like of a permuted dense tensor: empty_like keeps the permuted strides, and the caching allocator hands back
    the NaN-filled block just freed -- the fill must not multiply it"""
    x = torch.randn(64, 32, 16, device="cuda").permute(2, 0, 1)
    junk = torch.full((64 * 32 * 16,), math.nan, device="cuda")
    ptr = junk.data_ptr()
    del junk
    got = glue_run(op, [x])
    assert got.data_ptr() == ptr, "the allocator did not hand the NaN block back: the test proves nothing"
    want = op(x)
    assert got.stride() == want.stride()
    assert_bitwise(got, want, str(op))


def test_adding_zero_gives_ieee_signed_zeros():
    """x + 0.0 is the IEEE add: -0.0 + 0.0 = +0.0 (ATen), not x * 1"""
    mk = lambda: [lay(vals((1027,), 0), "flat")]          # noqa: E731
    assert (mk()[0].cpu() == 0).sum() >= 2
    for op in (aten.add.Tensor, aten.add.Scalar, aten.add_.Scalar, aten.sub.Scalar):
        for kw in ALPHAS:
            both(op, lambda: mk() + [0.0], kw, "x + 0.0")
    both(aten.add.Tensor, lambda: mk() + [torch.tensor(0.0)], what="x + cpu 0.0")


def test_division_by_a_cpu_scalar():
    """x / 3.0 and x / 0.1 with the divisor on the host (a Python number or a 0-dim CPU tensor): ATen's bits.  Prints whether
    ATen multiplies by the fp32 reciprocal (BinaryDivTrueKernel.cu) or divides."""
    x = lay(vals((4099,), 3), "flat")
    for b in (3.0, 0.1):
        recip = (x * torch.tensor(np.float32(1) / np.float32(b), device="cuda"))
        quot = x / torch.tensor(b, device="cuda")
        eager = aten.div.Scalar(x, b)
        how = "reciprocal product" if torch.equal(eager.view(torch.int32), recip.view(torch.int32)) else "true division"
        print(f"[glue] ATen x / {b} (CPU scalar): {how}; {int((quot != eager).sum())} of {x.numel()} differ from the true quotient")
        both(aten.div.Scalar, lambda: [x.clone(), b], what=str(b))
        both(aten.div.Tensor, lambda: [x.clone(), torch.tensor(b)], what=f"cpu {b}")
        both(aten.div_.Scalar, lambda: [x.clone(), b], what=f"in place {b}")


def test_memory_format_is_honoured():
    """clone / _to_copy / zeros_like / ones_like with memory_format=torch.channels_last: ATen's strides and bits"""
    for op, kw, dt in ((aten.clone.default, {}, torch.float32), (aten._to_copy.default, {"dtype": torch.float32}, torch.bfloat16),
                       (aten._to_copy.default, {"dtype": torch.float32}, torch.float32), (aten.zeros_like.default, {}, torch.float32),
                       (aten.ones_like.default, {}, torch.float32)):
        for mf in (torch.channels_last, torch.contiguous_format):
            make = lambda: [lay(vals((2, 6, 5, 4), 2), "flat", dt)]          # noqa: E731
            got, want = both(op, make, dict(kw, memory_format=mf), str(mf))
            assert got.stride() == want.stride(), (op, mf, got.stride(), want.stride())


def test_partial_overlap_raises_like_aten():
    """an in-place op or copy whose destination partly overlaps its input: ATen's RuntimeError, nothing routed, nothing written;
    the same view (full aliasing) stays routed"""
    ops, G = _g()
    cases = [("x[1:].add_(x[:-1])", lambda x: aten.add_.Tensor(x[1:], x[:-1])),
             ("x.add_(x[:1])", lambda x: aten.add_.Tensor(x, x[:1])),
             ("x[1:].mul_(x[:-1])", lambda x: aten.mul_.Tensor(x[1:], x[:-1])),
             ("x[2:].div_(x[:-2])", lambda x: aten.div_.Tensor(x[2:], x[:-2])),
             ("x[1:].copy_(x[:-1])", lambda x: aten.copy_.default(x[1:], x[:-1])),
             ("x[:1].expand(...).add_(1)", lambda x: aten.add_.Tensor(x[:1].expand(4, 5), x[1:5]))]
    for what, f in cases:
        x = torch.randn(6, 5, device="cuda")
        with pytest.raises(RuntimeError) as eager:
            f(x.clone())
        before = x.clone()
        G.reset_counts()
        with pytest.raises(RuntimeError) as glued:
            with ops.glue_mode(force=True):
                f(x)
        torch.cuda.synchronize()
        assert str(glued.value) == str(eager.value), what
        assert not G.ROUTED, (what, dict(G.ROUTED))
        assert torch.equal(x, before), what
    for op in (aten.add_.Tensor, aten.mul_.Tensor, aten.copy_.default):
        def make():
            x = lay(vals((6, 7, 10), 1), "perm")
            return [x, x]
        both(op, make, what="[the same view]")
