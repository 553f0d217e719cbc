"""Plain fp64 restatement of the fused BatchNorm (+ conv bias, + residual, + Q_IFNode) of include/s2f.h ("BatchNorm fused with the
conv bias, the residual add and the following Q_IFNode", "BatchNorm o BatchNorm", s2f_upsample2x_fwd) with its gradients -- a test
helper, no conftest, nothing of the package imported: torch on the CPU only.  Written from the header's formulas, not from the kernels:

  t = z + b ;  training: mean = E[t], var = E[(t - mean)^2] (biased, two passes) ;  eval: mean, var = the running statistics
  rstd = 1 / sqrt(var + eps) ;  xhat = (t - mean) rstd ;  u = gamma xhat + beta [+ r]
  training: running_mean' = (1 - m) running_mean + m mean ;  running_var' = (1 - m) running_var + m var n / (n - 1)
  border = beta - running_mean' gamma / sqrt(running_var' + eps)                       (BN(0) from the UPDATED running statistics)
  r = residual, or the exact-2x bilinear up-sampling (align_corners = False) of residual_lo [N, C, H/2, W/2]:
      out[2i] = 3/4 x[i] + 1/4 x[max(i - 1, 0)] ,  out[2i + 1] = 3/4 x[i] + 1/4 x[min(i + 1, h - 1)]   along H, then along W
  bn2: u = BN2(BN1(t)) [+ r], BOTH BatchNorms evaluated literally in train mode (the second one takes its own batch mean and biased
       variance of the first one's output) -- not the header's shortcut r2 = 1 / sqrt(gamma^2 var rstd^2 + eps2)
  neuron: h = v_in + u ; s = rint(clamp(h, 0, D)) half-even ; y = s / D ; v_out = h - s vth ; bit = (0 <= h <= D)
  backward: gu = g_u + g_v + ((g_y + g_y2) / D - g_v vth) bit ;  g_residual = gu (g_lo: the up-sampling's adjoint of it)
      training: gz = gamma rstd (gu - E[gu] - xhat E[gu xhat]) ;  eval: gz = gamma rstd gu, dbias = sum gz
      dgamma = sum gu xhat ;  dbeta = sum gu ;  bn2: every gradient by fp64 autograd through the literal composition

Every fp32 input is read exactly (eps and momentum as the fp32 numbers the C ABI receives).  `dtype=torch.float32` evaluates the same
expressions plainly in fp32, for measuring; `sums` hands it the channel sums the way a route of csrc/bn_lif.hip forms them
(route_sums / partial_sums below).  tests/test_bn_ref_host.py checks all of it against autograd of F.batch_norm and the oracle."""
from types import SimpleNamespace

import numpy as np
import torch

F64 = torch.float64


def _f32(x):
    return float(np.float32(x))


def _c(v, ndim):
    """a per-channel vector against [N, C, *]"""
    return v.view(1, -1, *([1] * (ndim - 2)))


def _dims(t):
    return (0,) + tuple(range(2, t.dim()))


def _to(dtype, *ts):
    if dtype is None:          # the autograd pass of backward(bn2=...): its fp64 leaves go through untouched, the graph stays
        return ts
    return tuple(None if t is None else t.detach().cpu().to(dtype) for t in ts)


def _up_matrix(h):
    """[2h, h]: the exact-2x bilinear up-sampling along one axis (align_corners = False); weights 3/4 and 1/4 are exact"""
    U = torch.zeros(2 * h, h, dtype=F64)
    for i in range(h):
        U[2 * i, i] += 0.75
        U[2 * i, max(i - 1, 0)] += 0.25
        U[2 * i + 1, i] += 0.75
        U[2 * i + 1, min(i + 1, h - 1)] += 0.25
    return U


def upsample2x(x):
    """[.., h, w] -> [.., 2h, 2w]"""
    Uh, Uw = _up_matrix(x.shape[-2]).to(x.dtype), _up_matrix(x.shape[-1]).to(x.dtype)
    return Uh @ x @ Uw.t()


def upsample2x_adjoint(g):
    """[.., 2h, 2w] -> [.., h, w]: the transpose of upsample2x"""
    Uh, Uw = _up_matrix(g.shape[-2] // 2).to(g.dtype), _up_matrix(g.shape[-1] // 2).to(g.dtype)
    return Uh.t() @ g @ Uw


def _batch_stats(t, sums, dtype):
    """-> mean, biased var [C].  sums None: two passes in `dtype`; else from (sum t, sum t^2) [C, 2] (fp64) as the kernels' chan_stat_of:
    fp64 arithmetic on the sums, the results rounded to `dtype`"""
    n = t.numel() // t.shape[1]
    if sums is None:
        mean = t.mean(_dims(t))
        return mean, ((t - _c(mean, t.dim())) ** 2).mean(_dims(t))
    m = sums[:, 0].double() / n
    return m.to(dtype), (sums[:, 1].double() / n - m * m).clamp_min(0).to(dtype)


def forward(z, bias, gamma, beta, rm, rv, training, momentum, eps, residual=None, residual_lo=None, bn2=None, dtype=F64, sums=None):
    """z [N, C, L] or [N, C, H, W]; bias, rm, rv may be None (rm / rv None in training: no running statistics, the border is
    formed from (0, 1) as the kernels do).  bn2: dict(gamma, beta, rm, rv, momentum, eps) of the second BatchNorm.
    -> mean, var (biased), rstd, running_mean, running_var, border, xhat, u  (+ mean2, var2, rstd2, running_mean2, running_var2)"""
    z, bias, gamma, beta, rm, rv, residual, residual_lo = _to(dtype, z, bias, gamma, beta, rm, rv, residual, residual_lo)
    eps, momentum = _f32(eps), _f32(momentum)
    nd = z.dim()
    n = z.numel() // z.shape[1]
    t = z if bias is None else z + _c(bias, nd)
    o = SimpleNamespace(t=t, n=n)
    rm0 = torch.zeros_like(gamma) if rm is None else rm
    rv0 = torch.ones_like(gamma) if rv is None else rv
    if training:
        o.mean, o.var = _batch_stats(t, sums, dtype)
        unb = o.var * (n / (n - 1.0)) if n > 1 else o.var
        o.running_mean = (1 - momentum) * rm0 + momentum * o.mean if rm is not None else rm0
        o.running_var = (1 - momentum) * rv0 + momentum * unb if rv is not None else rv0
    else:
        o.mean, o.var, o.running_mean, o.running_var = rm0, rv0, rm0, rv0
    o.rstd = 1.0 / torch.sqrt(o.var + eps)
    o.border = beta - o.running_mean * gamma / torch.sqrt(o.running_var + eps)
    o.xhat = (t - _c(o.mean, nd)) * _c(o.rstd, nd)
    u = o.xhat * _c(gamma, nd) + _c(beta, nd)
    if bn2 is not None:
        assert training
        g2, b2, rm2, rv2 = _to(dtype, bn2["gamma"], bn2["beta"], bn2.get("rm"), bn2.get("rv"))
        eps2, mom2 = _f32(bn2["eps"]), _f32(bn2["momentum"])
        o.mean2, o.var2 = _batch_stats(u, None, dtype)
        o.rstd2 = 1.0 / torch.sqrt(o.var2 + eps2)
        unb2 = o.var2 * (n / (n - 1.0)) if n > 1 else o.var2
        o.running_mean2 = None if rm2 is None else (1 - mom2) * rm2 + mom2 * o.mean2
        o.running_var2 = None if rv2 is None else (1 - mom2) * rv2 + mom2 * unb2
        u = (u - _c(o.mean2, nd)) * _c(o.rstd2, nd) * _c(g2, nd) + _c(b2, nd)
    if residual_lo is not None:
        assert residual is None
        residual = upsample2x(residual_lo).reshape(z.shape)
    o.residual = residual
    o.u = u if residual is None else u + residual
    return o


def neuron(h, D, vth):
    """-> y, v_out, s, bit in h's dtype (bit: bool)"""
    s = torch.round(torch.clamp(h, 0, D))
    return s / D, h - s * vth, s, (h >= 0) & (h <= D)


def form_gu(like, g_u, g_y, g_y2, g_v, bits, D, vth, absolute=False):
    """gu = g_u + g_v + ((g_y + g_y2) / D - g_v vth) bit; absolute: every term's absolute value added"""
    a = (lambda x: x.abs()) if absolute else (lambda x: x)
    gu = torch.zeros_like(like)
    if g_u is not None:
        gu = gu + a(g_u)
    if g_y is not None or g_y2 is not None or g_v is not None:
        m = bits.to(like.dtype)
        for gy in (g_y, g_y2):
            if gy is not None:
                gu = gu + a(gy) / D * m
        if g_v is not None:
            gu = gu + a(g_v) + ((a(g_v) * vth) if absolute else (-g_v * vth)) * m
    return gu


def backward(z, bias, gamma, beta, rm, rv, training, eps, g_u=None, g_y=None, g_y2=None, g_v=None, bits=None, D=8, vth=1.0, up=False,
             bn2=None, dtype=F64, sums=None):
    """The gradients of forward(...) under the incoming gradients given (any subset; the spike gradients need `bits`, the in-range map
    of the neuron, which the CALLER supplies).  up: the residual was residual_lo, g_lo is returned in place of g_residual.
    -> gu, gz, g_residual or g_lo, dgamma, dbeta, dbias (eval mode with a bias, else None) (+ dgamma2, dbeta2 for bn2)"""
    g_u, g_y, g_y2, g_v = _to(dtype, g_u, g_y, g_y2, g_v)
    fw = forward(z, bias, gamma, beta, rm, rv, training, 0.0, eps, dtype=dtype, sums=sums)
    nd, dims = fw.t.dim(), _dims(fw.t)
    gam = _to(dtype, gamma)[0]
    o = SimpleNamespace()
    o.gu = gu = form_gu(fw.t, g_u, g_y, g_y2, g_v, None if bits is None else bits.cpu(), D, _f32(vth))
    o.g_residual = upsample2x_adjoint(gu) if up else gu
    o.dbias = None
    if bn2 is not None and dtype != F64:
        # for measuring only: the header's closed form in `dtype` (the literal composition's own fp32 autograd would lose dgamma of
        # the first BatchNorm, 1e-5 of the second's, in its cancellation)
        g2, eps2 = _to(dtype, bn2["gamma"])[0], _f32(bn2["eps"])
        r2 = 1.0 / torch.sqrt(gam * gam * (fw.var * fw.rstd * fw.rstd) + eps2)
        S1, S2 = gu.sum(dims), (gu * fw.xhat).sum(dims)
        o.dbeta2, o.dgamma2, o.dbeta, o.dgamma = S1, gam * r2 * S2, torch.zeros_like(S1), g2 * eps2 * r2 ** 3 * S2
        o.gz = _c(gam * fw.rstd * g2 * r2, nd) * (gu - _c(S1 / fw.n, nd) - fw.xhat * _c(r2 * r2 * (gam * gam + eps2) * S2 / fw.n, nd))
        return o
    if bn2 is not None:
        assert training
        leaves = [t.detach().cpu().double().clone().requires_grad_(True) for t in (z, gamma, beta, bn2["gamma"], bn2["beta"])]
        b64 = None if bias is None else bias.detach().cpu().double()
        u = forward(leaves[0], b64, leaves[1], leaves[2], None, None, True, 0.0, eps,
                    bn2=dict(gamma=leaves[3], beta=leaves[4], eps=bn2["eps"], momentum=0.0), dtype=None).u
        (u * gu).sum().backward()
        o.gz, o.dgamma, o.dbeta, o.dgamma2, o.dbeta2 = (t.grad for t in leaves)
        return o
    o.dbeta = gu.sum(dims)
    o.dgamma = (gu * fw.xhat).sum(dims)
    scale = _c(gam * fw.rstd, nd)
    if training:
        o.gz = scale * (gu - _c(o.dbeta / fw.n, nd) - fw.xhat * _c(o.dgamma / fw.n, nd))
    else:
        o.gz = scale * gu
        if bias is not None:
            o.dbias = o.gz.sum(dims)
    return o


# ---------------------------------------------------------------------------------------------- the statistics as a route forms them
def route_sums(z, bias, slice_len=None):
    """(sum t, sum t^2) [C, 2] in fp64 the way s2f_bn_stats and the single-pass kernels form them: per (channel, slice of `slice_len`
    columns; None: the whole channel) the fp32 sums of d = (z + b) - pivot and d^2, pivot = the slice's first element of row 0,
    un-shifted in fp64 (sum t = sum d + n p, sum t^2 = sum d^2 + 2 p sum d + n p^2) and added over the slices."""
    z32 = z.detach().cpu().float().flatten(2)
    N, C, L = z32.shape
    t = z32 if bias is None else z32 + bias.detach().cpu().float().view(1, C, 1)
    out = torch.zeros(C, 2, dtype=F64)
    step = L if slice_len is None else slice_len
    for l0 in range(0, L, step):
        part = t[:, :, l0:l0 + step]
        p = part[0, :, 0]
        d = part - p.view(1, C, 1)
        s1, s2, cnt, p = d.sum((0, 2)).double(), (d * d).sum((0, 2)).double(), float(part.shape[0] * part.shape[2]), p.double()
        out[:, 0] += s1 + cnt * p
        out[:, 1] += s2 + 2 * p * s1 + cnt * p * p
    return out


def tile_partials(z, tile):
    """[C, P, 2] fp32: a producer's per-tile (sum z, sum z^2) over consecutive runs of `tile` columns of every row (L % tile == 0),
    p = n * (L / tile) + column tile -- the exact fp64 tile sums, rounded to fp32 once"""
    z64 = z.detach().cpu().double().flatten(2)
    N, C, L = z64.shape
    assert L % tile == 0
    zt = z64.view(N, C, L // tile, tile)
    return torch.stack([zt.sum(3), (zt * zt).sum(3)], -1).permute(1, 0, 2, 3).reshape(C, N * (L // tile), 2).float()


def partial_sums(partials, bias, n):
    """s2f_bn_partials_finalize: the P partials added in fp64, shifted by the conv bias -> (sum t, sum t^2) [C, 2]"""
    s = partials.detach().cpu().double().sum(1)
    if bias is None:
        return s
    b = bias.detach().cpu().double()
    return torch.stack([s[:, 0] + n * b, s[:, 1] + 2 * b * s[:, 0] + n * b * b], 1)


def pivot_map(z, bias, route, slice_len=None):
    """the pivot p (in t = z + b) behind every column of a channel, [C, L] fp64: 'stats' -- the first element of the column's slice,
    'single' -- the first element of the channel, 'partials' -- t - p = z (the un-shifted tile sums of the producer: the issue's
    "p = -b" in z + p = t - b), 'two-pass' -- the mean itself (kappa = 1 + var / (var + eps) <= 2)"""
    z64 = z.detach().cpu().double().flatten(2)
    N, C, L = z64.shape
    b = torch.zeros(C, dtype=F64) if bias is None else bias.detach().cpu().double()
    t0 = z64[0] + b.view(C, 1)
    if route == "partials":
        return b.view(C, 1).expand(C, L)
    if route == "single":
        return t0[:, :1].expand(C, L)
    if route == "stats":
        step = L if slice_len is None else slice_len
        return t0[:, torch.arange(L) // step * step]
    assert route == "two-pass"
    return (z64 + b.view(1, C, 1)).mean((0, 2)).view(C, 1).expand(C, L)


# ---------------------------------------------------------------------------------------------- sums of absolute terms
def abs_sums(z, bias, gamma, beta, rm, rv, training, momentum, eps, residual=None, residual_lo=None, bn2=None, pivot=None, g_u=None, g_y=None,
             g_y2=None, g_v=None, bits=None, D=8, vth=1.0):
    """The per-entry sums of absolute terms the bounds of tests/test_gpu_bn_routes.py multiply (fp64).  pivot: pivot_map(...) of the route
    (None / eval mode: kappa = 1).
      kappa    = 1 + E[(t - p)^2] / (var + eps): the conditioning of the variance as the route computes it
      A_u      = |gamma| rstd (|z| + |b| + |mean|) + kappa |gamma xhat| + |beta| + |r|
      X        = rstd (|t| + |mean|) + kappa |xhat|: the forward-error scale of xhat;   Xh = |xhat| + X
      A_dbeta  = sum |gu| ;  A_dgamma = sum |gu| Xh ;  A_gres = |gu| (A_glo: its up-sampling adjoint)
      A_gz     = |gamma| rstd (|gu| + E|gu| + Xh E[|gu| Xh])   (eval: |gamma| rstd |gu|, A_dbias = sum A_gz)
      |gu|     = |g_u| + |g_v| + ((|g_y| + |g_y2|) / D + |g_v| vth) bit
    and the scales of the per-channel outputs: A_mean = E|z| + |b| + |mean|, A_var = kappa (var + eps), A_rstd = kappa rstd,
    A_rm / A_rv (the momentum blend of |running| and A_mean / A_var n/(n-1)), A_border.
    bn2 (u = g xhat + beta2 + r with g = gamma gamma2 r2): gamma -> g and kappa -> 2 kappa in A_u and A_gz (r2 = 1 / sqrt(gamma^2 var
    rstd^2 + eps2) moves by at most half the relative error of var rstd^2, which carries var's and twice rstd's: at most kappa more);
    A_gz's xhat term carries the header's factor r2^2 (gamma^2 + eps2) <= 1 + eps2 r2^2; A_dgamma2 = |gamma| r2 A_dgamma,
    A_dgamma1 = |gamma2| eps2 r2^3 sum |gu xhat| (the issue's own scale: no X), A_dbeta2 = A_dbeta."""
    fw = forward(z, bias, gamma, beta, rm, rv, training, momentum, eps, residual, residual_lo, bn2)
    z64, b64, gam, bet, rm64, rv64 = _to(F64, z, bias, gamma, beta, rm, rv)
    eps, momentum = _f32(eps), _f32(momentum)
    nd, dims, n = z64.dim(), _dims(z64), fw.n
    C = z64.shape[1]
    o = SimpleNamespace()
    if training and pivot is not None:
        d = fw.t.flatten(2) - pivot.view(1, C, -1)
        o.kappa = 1 + (d * d).mean((0, 2)) / (fw.var + eps)
    else:
        o.kappa = torch.ones(C, dtype=F64)
    babs = torch.zeros(C, dtype=F64) if b64 is None else b64.abs()
    kap, geff, beff = o.kappa, gam.abs(), bet.abs()
    if bn2 is not None:
        g2, b2 = _to(F64, bn2["gamma"], bn2["beta"])
        kap, geff, beff = 2 * o.kappa, (gam * g2 * fw.rstd2).abs(), b2.abs()
    o.A_u = _c(geff * fw.rstd, nd) * (z64.abs() + _c(babs + fw.mean.abs(), nd)) + _c(kap * geff, nd) * fw.xhat.abs() + _c(beff, nd)
    if fw.residual is not None:
        o.A_u = o.A_u + (fw.residual.abs() if residual_lo is None else upsample2x(_to(F64, residual_lo)[0].abs()).reshape(z64.shape))
    o.A_mean = z64.abs().mean(dims) + babs + fw.mean.abs()
    o.A_var = o.kappa * (fw.var + eps)
    o.A_rstd = o.kappa * fw.rstd
    unb = n / (n - 1.0) if n > 1 else 1.0
    o.A_rm = (1 - momentum) * (rm64.abs() if rm64 is not None else 0) + momentum * o.A_mean if training else fw.running_mean.abs()
    o.A_rv = (1 - momentum) * (rv64.abs() if rv64 is not None else 0) + momentum * unb * o.A_var if training else fw.running_var.abs()
    den = torch.sqrt(fw.running_var + eps)
    o.A_border = bet.abs() + gam.abs() * (o.A_rm + fw.running_mean.abs()) / den + (fw.running_mean * gam).abs() * 0.5 * o.A_rv / den ** 3
    if g_u is None and g_y is None and g_y2 is None and g_v is None:
        return o
    g_u, g_y, g_y2, g_v = _to(F64, g_u, g_y, g_y2, g_v)
    ga = form_gu(z64, g_u, g_y, g_y2, g_v, None if bits is None else bits.cpu(), D, _f32(vth), absolute=True)
    Xh = fw.xhat.abs() + _c(fw.rstd, nd) * (fw.t.abs() + _c(fw.mean.abs(), nd)) + _c(kap, nd) * fw.xhat.abs()
    o.A_gres = upsample2x_adjoint(ga) if residual_lo is not None else ga
    o.A_dbeta = ga.sum(dims)
    o.A_dgamma = (ga * Xh).sum(dims)
    scale = _c(geff * fw.rstd, nd)
    o.A_dbias = None
    if training:
        k2 = 1.0 if bn2 is None else _c(fw.rstd2 ** 2 * (gam ** 2 + _f32(bn2["eps"])), nd)
        o.A_gz = scale * (ga + _c(o.A_dbeta / n, nd) + Xh * k2 * _c(o.A_dgamma / n, nd))
    else:
        o.A_gz = scale * ga
        o.A_dbias = o.A_gz.sum(dims)
    if bn2 is not None:
        o.A_dgamma1 = g2.abs() * _f32(bn2["eps"]) * fw.rstd2 ** 3 * (ga * fw.xhat.abs()).sum(dims)
        o.A_dgamma2, o.A_dbeta2 = gam.abs() * fw.rstd2 * o.A_dgamma, o.A_dbeta
    return o
