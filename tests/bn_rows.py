"""The rows of tests/test_gpu_bn_routes.py, their draws and their bounds -- shared with tests/test_bn_ref_host.py, which holds every
cap to the reference's own fp32 evaluation on the CPU.  A test helper: torch on the CPU and tests/bn_ref.py only.

A row names the route it must take (the GPU test proves it from the library's predicates), the shape, the forward variant (lif, v_in,
bf16), the incoming gradients (`grads`: a subset of "uyv", "2" adds a second reader of the spike map) and what else is distinct code:
mode, bias, residual ("res" / "lo": the up-sampling residual), D, vth, want_pre, the data ("randn", "large": mean 50, std 1e-2 .. 1,
channel 0 constant; "exact": see exact_draw)."""
import zlib
from types import SimpleNamespace

import torch

import bn_ref

C_U = 2e-6          # 32 x 2^-24, see the docstring of test_gpu_bn_routes.py
C_G = 5.2e-6        # 8 x the worst fp32-CPU ratio |err| / A over the rows (6.5e-7: gz of fused-rest-f32-y), below the cap 1e-5
C_G_CAP = 1e-5
TINY = 1e-30
EPS = 1e-5
MOMENTUM = 0.1


def row(id, route, shape, lif=False, v_in=False, bf16=False, grads="u", training=True, bias=False, res=None, D=8, vth=1.0, want_pre=True,
        data="randn", kind="act", G=1, tile=0, eps=EPS, momentum=MOMENTUM):
    assert not (set(grads) - set("uyv2")) and (lif or not (set(grads) & set("yv2"))) and ("2" not in grads or "y" in grads)
    return SimpleNamespace(id=id, route=route, shape=shape, lif=lif, v_in=v_in, bf16=bf16, grads=grads, training=training, bias=bias,
                           res=res, D=D, vth=vth, want_pre=want_pre, data=data, kind=kind, G=G, tile=tile, eps=eps, momentum=momentum)


# the seven incoming-gradient combinations, each on one of the five forward variants (kFwdVariants x kBwdGrads of csrc/bn_lif.hip)
VARIANTS = (("bn-u", dict(grads="u")),
            ("rest-f32-y", dict(lif=True, grads="y")),
            ("rest-bf16-uy", dict(lif=True, bf16=True, grads="uy")),
            ("v-f32-v", dict(lif=True, v_in=True, grads="v")),
            ("v-bf16-yv", dict(lif=True, v_in=True, bf16=True, grads="yv")),
            ("rest-f32-uv", dict(lif=True, grads="uv")),
            ("v-bf16-uyv", dict(lif=True, v_in=True, bf16=True, grads="uyv")))
# the smallest shapes of every form, derived from the predicates of csrc/bn_lif.hip (S2F_BN_TPW = 4, kSmallIters = 8, kMidIters = 5)
FORMS = {"fused": ((4, 64, 256), (5, 64, 256), (8, 64, 2048)),
         "small": ((2, 32, 4), (2, 32, 100), (16, 32, 128)),
         "mid": ((1, 32, 2052), (4, 32, 4200), (4, 32, 5116)),
         "rows-aligned": ((2, 3, 256), (1, 2, 4096)),
         "rows-straddling": ((3, 5, 260), (1, 2, 4100))}


def _rows():
    out = []
    for form, shapes in FORMS.items():
        for i, (name, kw) in enumerate(VARIANTS):
            out.append(row(f"{form}-{name}", form, shapes[i % len(shapes)], bias=i % 2 == 1, res="res" if i % 3 == 0 else None, **kw))
    out += [
        row("flat-u", "flat", (2, 7, 36), grads="u", bias=True),
        row("flat-y", "flat", (2, 7, 36), lif=True, bf16=True, grads="y"),
        row("flat-uyv", "flat", (2, 7, 36), lif=True, v_in=True, grads="uyv", res="res"),
        row("anyl-uyv", "anyl", (3, 5, 7), lif=True, v_in=True, grads="uyv", bias=True, res="res"),
        row("anyl-one-column-y", "anyl", (2, 3, 1), lif=True, grads="y"),
        row("anyl-slices-u", "anyl", (1, 2, 4099), grads="u", bias=True),
        # (SPIKES_BF16 on: spikes_bf16_ok must refuse bf16 for a D that is no power of two -- the row expects fp32 spikes)
        row("d6-off-the-rows-uyv", "flat", (2, 3, 512), lif=True, v_in=True, bf16=True, grads="uyv", D=6),
        row("up-image-rows", "up", (1, 2, 16, 16), lif=True, bf16=True, grads="uy", res="lo", bias=True),
        row("up-wide-row", "up", (1, 1, 2, 256), lif=True, v_in=True, grads="uyv", res="lo"),
        row("bn2-u", "bn2", (4, 64, 256), grads="u", kind="bn2"),
        row("bn2-bf16-uy-res", "bn2", (8, 64, 1024), lif=True, bf16=True, grads="uy", res="res", kind="bn2"),
        row("bn2-v-uyv", "bn2", (4, 64, 256), lif=True, v_in=True, grads="uyv", kind="bn2"),
        row("grouped-2-bf16-uy", "grouped", (2, 32, 100), lif=True, bf16=True, grads="uy", bias=True, kind="grouped", G=2),
        row("grouped-4-u", "grouped", (2, 32, 100), grads="u", kind="grouped", G=4),
        row("grouped-2-f32-y", "grouped", (2, 32, 100), lif=True, grads="y", kind="grouped", G=2),
        row("partials-per-wave", "partials", (1, 6, 1040), lif=True, grads="uy", bias=True, kind="partials", tile=16),
        row("partials-per-channel", "partials", (1, 6, 4112), lif=True, v_in=True, grads="uyv", bias=True, kind="partials", tile=16),
        row("second-reader-fused", "fused", (5, 64, 256), lif=True, bf16=True, grads="uy2", res="res"),
        row("second-reader-rows-aligned", "rows-aligned", (2, 3, 256), lif=True, bf16=True, grads="y2v"),
        row("second-reader-rows-straddling", "rows-straddling", (3, 5, 260), lif=True, bf16=True, grads="uy2", bias=True),
        row("second-reader-added-by-the-op-layer", "small", (2, 32, 100), lif=True, bf16=True, grads="y2"),
        row("eval-flat", "flat", (2, 7, 36), lif=True, bf16=True, grads="uy", training=False, bias=True),
        row("eval-anyl", "anyl", (3, 5, 7), lif=True, v_in=True, grads="uyv", training=False, bias=True, res="res"),
        row("eval-rows-aligned", "rows-aligned", (2, 3, 256), lif=True, v_in=True, bf16=True, grads="yv", training=False, bias=True),
        row("eval-rows-straddling", "rows-straddling", (3, 5, 260), grads="u", training=False, bias=True, res="res"),
        row("vth-fused", "fused", (4, 64, 256), lif=True, v_in=True, bf16=True, grads="uyv", vth=0.75),
        row("vth-rows-aligned", "rows-aligned", (2, 3, 256), lif=True, v_in=True, grads="yv", vth=0.75, bias=True),
        row("vth-flat", "flat", (2, 7, 36), lif=True, v_in=True, bf16=True, grads="v", vth=0.75),
        row("d4-small", "small", (2, 32, 100), lif=True, bf16=True, grads="uy", D=4),
        row("d16-mid", "mid", (1, 32, 2052), lif=True, v_in=True, grads="yv", D=16),
        # (the row-walking kernels multiply by 1 / D, the others divide by D: a D other than 8 on each of them too)
        row("d4-rows-aligned", "rows-aligned", (2, 3, 256), lif=True, v_in=True, bf16=True, grads="yv", D=4),
        row("d16-rows-straddling", "rows-straddling", (3, 5, 260), lif=True, bf16=True, grads="uy", D=16, bias=True),
        row("d16-fused", "fused", (4, 64, 256), lif=True, grads="uy", D=16),
        row("no-pre-fused", "fused", (4, 64, 256), lif=True, bf16=True, grads="y", want_pre=False),
        row("no-pre-small", "small", (2, 32, 100), lif=True, grads="y", want_pre=False, bias=True),
        row("no-pre-mid", "mid", (1, 32, 2052), lif=True, bf16=True, grads="y", want_pre=False),
        row("no-pre-rows", "rows-straddling", (3, 5, 260), lif=True, v_in=True, bf16=True, grads="yv", want_pre=False),
        row("no-pre-flat", "flat", (2, 7, 36), lif=True, grads="y", want_pre=False, res="res"),
        row("large-mean-stats-two-slices", "rows-aligned", (1, 2, 4096), grads="u", data="large"),
        row("large-mean-stats-any", "anyl", (1, 2, 4099), grads="u", data="large", bias=True),
        row("large-mean-rows-straddling", "rows-straddling", (3, 5, 260), lif=True, bf16=True, grads="uy", data="large"),
        row("large-mean-partials", "partials", (1, 6, 1040), grads="u", data="large", bias=True, kind="partials", tile=16),
    ]
    return out


ROWS = _rows()
# one exact row per single-pass, row-walking and flat-vector route (N L even)
EXACT = (("fused", (4, 64, 256)), ("small", (2, 32, 100)), ("mid", (1, 32, 2052)), ("rows-aligned", (2, 3, 256)),
         ("rows-straddling", (3, 5, 260)), ("flat", (2, 7, 36)))


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def stats_slice(C, L):
    """pick_slices of csrc/bn_lif.hip: the columns per (channel, slice) workgroup of s2f_bn_stats"""
    S = 1
    while C * S < 1024 and L // (S * 2) >= 2048:
        S *= 2
    return S, ((L + S - 1) // S + 3) // 4 * 4


def single_pass(route):
    return route in ("fused", "small", "mid", "bn2", "grouped")


# ---------------------------------------------------------------------------------------------- draws
def draw(r):
    """every operand of row r as fp32 CPU tensors (grouped rows: a list of G such draws in .groups, operands of group 0 on top)"""
    g = gen(r.id)
    if r.kind == "grouped":
        ds = [_draw_one(r, g) for _ in range(r.G)]
        ds[0].groups = ds
        return ds[0]
    return _draw_one(r, g)


def _draw_one(r, g):
    shape = r.shape
    N, C = shape[:2]
    rn = lambda *s: torch.randn(*s, generator=g)
    d = SimpleNamespace(groups=None)
    if r.data == "large":
        z = 50.0 + torch.logspace(-2, 0, C).flip(0).view(1, C, *([1] * (len(shape) - 2))) * rn(*shape)
        z[:, 0] = 3.25
    else:
        z = rn(*shape) * 2 + 0.5
    d.z = z
    d.bias = rn(C) if r.bias else None
    sign = (torch.rand(C, generator=g) < 0.75).float() * 2 - 1
    d.gamma, d.beta = (torch.rand(C, generator=g) + 0.5) * sign, rn(C) * 0.3 + 0.5
    d.rm, d.rv = rn(C) * 0.1, torch.rand(C, generator=g) + 0.5
    d.residual = rn(*shape) if r.res == "res" else None
    d.residual_lo = rn(N, C, shape[2] // 2, shape[3] // 2) if r.res == "lo" else None
    d.v_in = rn(*shape) * 0.5 if r.v_in else None
    d.w = {k: rn(*shape) for k in "uyv2"}
    d.bn2 = None
    if r.kind == "bn2":
        d.bn2 = dict(gamma=torch.rand(C, generator=g) + 0.5, beta=rn(C) * 0.3 + 0.5, rm=rn(C) * 0.1, rv=torch.rand(C, generator=g) + 0.5,
                     eps=EPS, momentum=MOMENTUM)
    return d


def _eighths(g, lo, hi, *s):
    return torch.randint(lo, hi + 1, s, generator=g).float() / 8


def exact_draw(route, shape):
    """Operands on which every route is exact in fp32 in any order of evaluation (eps = 0, D = 8, vth = 1).  Per channel half of the
    N L elements of t = z + b are m + a and half m - a, m a multiple of 1/8, a in {1/2, 1, 2}: mean = m, var = a^2, rstd = 1 / a,
    xhat = +-1; b, gamma (non-zero), beta, the residual and v_in multiples of 1/8.  BatchNorm-only backward: gu = gu0 + k1 + k2 xhat,
    gu0 integers that cancel in pairs inside each half, k1 / k2 non-zero integers: E[gu] = k1, E[gu xhat] = k2, so gz = gamma rstd gu0,
    dbeta = k1 N L, dgamma = k2 N L.  Eval mode: running_mean a multiple of 1/8, running_var in {4, 1, 1/4}; g_u, g_v integers, g_y a
    multiple of 8.  All of it is asserted here in fp64 on the draw itself."""
    g = gen("exact-" + route)
    N, C, L = shape
    n = N * L
    assert n % 2 == 0
    d = SimpleNamespace(groups=None, bn2=None, residual_lo=None)
    m, a = _eighths(g, -16, 16, C), torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
    sgn = torch.empty(C, n)
    gu0 = torch.zeros(C, n)
    for c in range(C):
        perm = torch.randperm(n, generator=g)
        sgn[c, perm[:n // 2]], sgn[c, perm[n // 2:]] = 1.0, -1.0
        for half in (perm[:n // 2], perm[n // 2:]):
            k = len(half) // 2
            q = torch.randint(1, 4, (k,), generator=g).float()
            gu0[c, half[:k]], gu0[c, half[k:2 * k]] = q, -q
    to_map = lambda x: x.view(C, N, L).permute(1, 0, 2).contiguous()
    d.bias = _eighths(g, -8, 8, C)
    d.z = m.view(1, C, 1) + a.view(1, C, 1) * to_map(sgn) - d.bias.view(1, C, 1)
    d.gamma = _eighths(g, 4, 16, C) * ((torch.rand(C, generator=g) < 0.75).float() * 2 - 1)
    d.beta = _eighths(g, -8, 24, C)
    d.residual, d.v_in = _eighths(g, -16, 16, N, C, L), _eighths(g, -8, 8, N, C, L)
    d.rm, d.rv = _eighths(g, -8, 8, C), torch.tensor([4.0, 1.0, 0.25])[torch.randint(0, 3, (C,), generator=g)]
    pm = lambda: torch.randint(1, 4, (C,), generator=g).float() * ((torch.rand(C, generator=g) < 0.5).float() * 2 - 1)
    d.k1, d.k2, d.gu0 = pm(), pm(), to_map(gu0)
    d.gu_train = d.gu0 + d.k1.view(1, C, 1) + d.k2.view(1, C, 1) * to_map(sgn)
    ints = lambda: torch.randint(-3, 4, (N, C, L), generator=g).float()
    d.w = {"u": ints(), "y": ints() * 8, "v": ints()}
    # the claims, in fp64 on this draw
    fw = bn_ref.forward(d.z, d.bias, d.gamma, d.beta, None, None, True, 0.0, 0.0)
    assert torch.equal(fw.mean, m.double()) and torch.equal(fw.var, (a * a).double()) and torch.equal(fw.rstd, (1 / a).double())
    assert torch.equal(fw.xhat, to_map(sgn).double()) and bool((d.gamma != 0).all())
    bw = bn_ref.backward(d.z, d.bias, d.gamma, d.beta, None, None, True, 0.0, g_u=d.gu_train)
    assert torch.equal(bw.dbeta, (d.k1 * n).double()) and torch.equal(bw.dgamma, (d.k2 * n).double())
    assert torch.equal(bw.gz, (d.gamma / a).double().view(1, C, 1) * d.gu0.double())
    for t in (fw.u + d.residual.double() + d.v_in.double(), bw.gz):          # eighths (gz: sixteenths), far inside fp32
        assert torch.equal(t * 16, (t * 16).round()) and t.abs().max() < 2 ** 10
    ev = bn_ref.forward(d.z, d.bias, d.gamma, d.beta, d.rm, d.rv, False, 0.0, 0.0, residual=d.residual)
    h = ev.u + d.v_in.double()
    assert torch.equal(h * 128, (h * 128).round()) and h.abs().max() < 2 ** 7          # fits fp32 at any association, fused or not
    bits = bn_ref.neuron(h, 8, 1.0)[3]
    A = bn_ref.abs_sums(d.z, d.bias, d.gamma, d.beta, d.rm, d.rv, False, 0.0, 0.0, residual=d.residual, g_u=d.w["u"], g_y=d.w["y"],
                        g_v=d.w["v"], bits=bits)
    # integer gu times xhat in sixteenths: every partial sum of dgamma is a whole number of sixteenths below 2^24
    assert float((A.A_dgamma * 16).max()) < 2 ** 24 and float(A.A_dbeta.max()) < 2 ** 24
    return d


# ---------------------------------------------------------------------------------------------- the reference of a row, and the bounds
def loss_grads(r, d):
    """the incoming gradients the row's loss sends: sum(u w_u) + sum(y w_y) + sum(y w_2) + sum(v_out w_v)"""
    pick = lambda k: d.w[k] if k in r.grads else None
    return dict(g_u=pick("u"), g_y=pick("y"), g_y2=pick("2"), g_v=pick("v"))


def route_pivot(r, d):
    if not r.training:
        return None
    z3 = d.z.flatten(2)
    if r.kind == "partials":
        return bn_ref.pivot_map(z3, d.bias, "partials")
    if single_pass(r.route):
        return bn_ref.pivot_map(z3, d.bias, "single")
    return bn_ref.pivot_map(z3, d.bias, "stats", stats_slice(z3.shape[1], z3.shape[2])[1])


def route_sums32(r, d):
    """the channel sums the row's route hands its apply kernel, formed in fp32 on the CPU (None: eval mode)"""
    if not r.training:
        return None
    z3 = d.z.flatten(2)
    if r.kind == "partials":
        return bn_ref.partial_sums(bn_ref.tile_partials(z3, r.tile), d.bias, z3.shape[0] * z3.shape[2])
    return bn_ref.route_sums(z3, d.bias, None if single_pass(r.route) else stats_slice(z3.shape[1], z3.shape[2])[1])


def fwd_args(r, d):
    return (d.z, d.bias, d.gamma, d.beta, d.rm, d.rv, r.training, r.momentum, r.eps)


def _ratio(got, ref, A):
    """worst (|got - ref| - TINY) / A over the entries; inf when an entry of `got` is not finite (a NaN must fail every bound, and
    neither max() nor a comparison would see it) or errs where A is 0"""
    got = got.detach().cpu().double()
    err = (got - ref).abs()
    assert err.shape == A.shape, (err.shape, A.shape)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(A).all())
    if not bool(torch.isfinite(got).all()) or bool(((A == 0) & (err > TINY)).any()):
        return float("inf")
    return float(((err - TINY).clamp_min(0) / A.clamp_min(1e-300)).max())


def worse(acc, new):
    """acc[k] = the worse of acc[k] and new[k]; a NaN counts as inf (max(0.0, nan) is 0.0)"""
    for k, v in new.items():
        v = float("inf") if v != v else v
        acc[k] = max(acc.get(k, 0.0), v)
    return acc


def within(ratios, c):
    """every ratio is a number no larger than c (written so that a NaN fails)"""
    return bool(ratios) and all(v <= c for v in ratios.values())


def forward_ratios(r, d, got):
    """worst |got - fp64| / A over the entries of u and of every per-channel output present in `got` (a dict of tensors: u, mean, rstd,
    running_mean, running_var, border [, rstd2, running_mean2, running_var2])"""
    fw = bn_ref.forward(*fwd_args(r, d), residual=d.residual, residual_lo=d.residual_lo, bn2=d.bn2)
    A = bn_ref.abs_sums(*fwd_args(r, d), residual=d.residual, residual_lo=d.residual_lo, bn2=d.bn2, pivot=route_pivot(r, d))
    scale = {"u": A.A_u, "mean": A.A_mean, "rstd": A.A_rstd, "running_mean": A.A_rm, "running_var": A.A_rv, "border": A.A_border}
    if d.bn2 is not None:
        m2 = _f(d.bn2["momentum"])
        n = fw.n
        # the second BatchNorm's statistics are functions of the first one's: beta, gamma^2 var rstd^2 (relative error 3 kappa)
        scale.update(rstd2=3 * A.kappa * fw.rstd2, running_mean2=(1 - m2) * d.bn2["rm"].double().abs() + m2 * d.beta.double().abs(),
                     running_var2=(1 - m2) * d.bn2["rv"].double().abs() + m2 * 3 * A.kappa * fw.var2 * n / (n - 1.0))
    return {k: _ratio(v, getattr(fw, k), scale[k]) for k, v in got.items() if v is not None}


def _f(x):
    return bn_ref._f32(x)


def backward_ratios(r, d, got, bits):
    """worst |got - fp64| / A of every gradient present in `got` (gz, g_residual, dgamma, dbeta, dbias [, dgamma2, dbeta2]); the fp64
    reference and the sums of absolute terms take the in-range map `bits` the caller read off the evaluation under test"""
    kw = dict(loss_grads(r, d), bits=bits, D=r.D, vth=r.vth)
    bw = bn_ref.backward(d.z, d.bias, d.gamma, d.beta, d.rm, d.rv, r.training, r.eps, up=d.residual_lo is not None, bn2=d.bn2, **kw)
    A = bn_ref.abs_sums(*fwd_args(r, d), residual=d.residual, residual_lo=d.residual_lo, bn2=d.bn2, pivot=route_pivot(r, d), **kw)
    scale = {"gz": A.A_gz, "g_residual": A.A_gres, "dgamma": A.A_dgamma, "dbeta": A.A_dbeta, "dbias": A.A_dbias}
    if d.bn2 is not None:
        scale.update(dgamma=A.A_dgamma1, dbeta=torch.zeros_like(A.A_dbeta), dgamma2=A.A_dgamma2, dbeta2=A.A_dbeta2)
    out = {k: _ratio(v, getattr(bw, k), scale[k]) for k, v in got.items() if v is not None}
    if d.bn2 is not None and got.get("dbeta") is not None:
        # the first BatchNorm's shift is removed by the second: exactly 0 (the fp64 autograd value is its own round-off, 1e-16)
        assert float(bw.dbeta.abs().max()) <= 1e-12 * float(bw.dbeta2.abs().max())
        out["dbeta"] = 0.0 if bool((got["dbeta"] == 0).all()) else float("inf")
    return out


def cpu32(r, d):
    """bn_ref's own expressions evaluated in fp32 on the CPU, the statistics formed as the row's route forms them
    -> (forward outputs, gradients, the in-range map of ITS h) in the dictionaries forward_ratios / backward_ratios take"""
    f32 = torch.float32
    sums = route_sums32(r, d)
    fw = bn_ref.forward(*fwd_args(r, d), residual=d.residual, residual_lo=d.residual_lo, bn2=d.bn2, dtype=f32, sums=sums)
    fwd = {k: getattr(fw, k) for k in ("u", "mean", "rstd", "running_mean", "running_var", "border")}
    bits = None
    if r.lif:
        bits = bn_ref.neuron(fw.u if d.v_in is None else d.v_in + fw.u, r.D, r.vth)[3]
    bw = bn_ref.backward(d.z, d.bias, d.gamma, d.beta, d.rm, d.rv, r.training, r.eps, up=d.residual_lo is not None, bn2=d.bn2, dtype=f32,
                         sums=sums, bits=bits, D=r.D, vth=r.vth, **loss_grads(r, d))
    names = ["gz", "dgamma", "dbeta"] + (["g_residual"] if r.res else []) + (["dbias"] if (r.bias and not r.training) else []) + \
            (["dgamma2", "dbeta2"] if d.bn2 is not None else [])
    return fwd, {k: getattr(bw, k) for k in names}, bits
