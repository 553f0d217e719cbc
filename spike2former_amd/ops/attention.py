"""The spike-driven attention core (csrc/sdsa.hip) and the DCNv3 sampling core (csrc/dcnv3.hip)."""
import ctypes

import torch

from .config import cfg
from .core import *          # noqa: F401,F403  (the shared plumbing: _ptr, _stream, check, lib, Spikes, ...)


# ------------------------------------------------------------------------------------------------ attention core
class _SDSA(torch.autograd.Function):
    """o = scale * q (k^T v) on channel-major spikes [TB, C, N] (sdtv2.py:335-339; transformer.py:253-274)."""

    @staticmethod
    def forward(ctx, q, k, v, heads, scale):
        _need_cuda(q, k, v)
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        TB, C, Nq = q.shape
        Nk = k.shape[2]
        d = C // heads
        o = torch.empty_like(q)
        kv = torch.empty(TB, heads, d, d, dtype=torch.float32, device=q.device)
        check(lib.s2f_sdsa_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(kv), TB, heads, d, Nq, Nk, scale, _stream()),
              "s2f_sdsa_fwd")
        ctx.save_for_backward(q, k, v, kv)
        ctx.heads, ctx.scale = heads, scale
        return o

    @staticmethod
    def backward(ctx, go):
        q, k, v, kv = ctx.saved_tensors
        go = go.contiguous()
        TB, C, Nq = q.shape
        Nk = k.shape[2]
        d = C // ctx.heads
        gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ws = torch.empty_like(kv)
        check(lib.s2f_sdsa_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(kv), _ptr(go), _ptr(gq), _ptr(gk), _ptr(gv), _ptr(ws),
                               TB, ctx.heads, d, Nq, Nk, ctx.scale, _stream()), "s2f_sdsa_bwd")
        return gq, gk, gv, None, None


class _SDSASpikes(torch.autograd.Function):
    """The attention core on bf16 spike operands (s2f.h s2f_sdsa_*_bf16), optionally fused with the neuron that follows it
    (s2f_sdsa_lif_fwd_bf16: kv on the matrix cores, o never written, spikes + mask + counters from the epilogue).
    packed: `qd` is the stacked q|k|v map [TB, 3C, N] of the batched projection chain (one autograd handle `qt`, one
    [TB, 3C, N] gradient -- no split / stack copies); packed == 2: `qd` is the group-outermost buffer [3, TB, C, N] of the decoder's
    sibling projection chains (q, k, v = its three contiguous slices; one handle, one [3, TB, C, N] gradient); otherwise three
    [TB, C, N*] tensors with a handle each."""

    @staticmethod
    def forward(ctx, qd, kd, vd, qt, kt, vt, heads, scale, packed, fuse, D, vth, stats):
        qd = qd.contiguous()
        TB = qd.shape[0]
        if packed == 2:
            _, TB, C, Nq = qd.shape
            Nk = Nq
            qs = ks = vs = C * Nq
            qp = qd.data_ptr()
            kp, vp = qp + 2 * TB * C * Nq, qp + 4 * TB * C * Nq
        elif packed:
            C, Nq = qd.shape[1] // 3, qd.shape[2]
            Nk = Nq
            qs = ks = vs = 3 * C * Nq
            qp = qd.data_ptr()
            kp, vp = qp + 2 * C * Nq, qp + 4 * C * Nq
        else:
            kd, vd = kd.contiguous(), vd.contiguous()
            C, Nq, Nk = qd.shape[1], qd.shape[2], kd.shape[2]
            qs, ks, vs = C * Nq, C * Nk, C * Nk
            qp, kp, vp = qd.data_ptr(), kd.data_ptr(), vd.data_ptr()
        d = C // heads
        dev = qd.device
        kv = torch.empty(TB, heads, d, d, dtype=torch.float32, device=dev)
        ctx.cfg = (TB, C, Nq, Nk, d, heads, scale, packed, fuse, D, (qs, ks, vs))
        ctx.ptrs_of = (kp - qp, vp - qp)
        need = any(ctx.needs_input_grad[3:6])
        if fuse:
            y = torch.empty(TB, C, Nq, dtype=torch.bfloat16, device=dev)
            mask = torch.empty(mask_words(y.numel()), dtype=torch.int64, device=dev) if need else None
            _time_next("sdsa_lif_fwd", 4 * TB * C * (2 * Nk + 2 * Nq), 4 * TB * heads * d * d * (Nk + Nq),
                       moved=2 * TB * C * (2 * Nk + 2 * Nq))
            check(lib.s2f_sdsa_lif_fwd_bf16(qp, kp, vp, qs, ks, vs, _ptr(y), _ptr(mask), _ptr(stats), _ptr(kv), TB, heads, d, Nq,
                                            scale, vth, D, _stream()), "s2f_sdsa_lif_fwd_bf16")
            ctx.save_for_backward(qd, kd, vd, kv, mask)
            return _Outputs(ctx, kv).spikes(y, True, spare=False).done()
        o = torch.empty(TB, C, Nq, dtype=torch.float32, device=dev)
        check(lib.s2f_sdsa_fwd_bf16(qp, kp, vp, qs, ks, vs, _ptr(o), _ptr(kv), TB, heads, d, Nq, Nk, scale, _stream()),
              "s2f_sdsa_fwd_bf16")
        ctx.save_for_backward(qd, kd, vd, kv, None)
        return _Outputs(ctx, kv).spikes(o, False).done()

    @staticmethod
    def backward(ctx, g, _gdata, _g2):
        qd, kd, vd, kv, mask = ctx.saved_tensors
        TB, C, Nq, Nk, d, heads, scale, packed, fuse, D, (qs, ks, vs) = ctx.cfg
        if g is None:
            return _grads(ctx)
        g = g.contiguous()
        dev = g.device
        qp = qd.data_ptr()
        if packed == 2:
            G = torch.empty(3, TB, C, Nq, dtype=torch.float32, device=dev)
            gq, gk, gv = G.data_ptr(), G.data_ptr() + 4 * TB * C * Nq, G.data_ptr() + 8 * TB * C * Nq
            gs = (C * Nq,) * 3
            kp, vp = qp + ctx.ptrs_of[0], qp + ctx.ptrs_of[1]
            out = (G, None, None)
        elif packed:
            G = torch.empty(TB, 3 * C, Nq, dtype=torch.float32, device=dev)
            gq, gk, gv = G.data_ptr(), G.data_ptr() + 4 * C * Nq, G.data_ptr() + 8 * C * Nq
            gs = (3 * C * Nq,) * 3
            kp, vp = qp + ctx.ptrs_of[0], qp + ctx.ptrs_of[1]
            out = (G, None, None)
        else:
            Gq = torch.empty(TB, C, Nq, dtype=torch.float32, device=dev)
            Gk = torch.empty(TB, C, Nk, dtype=torch.float32, device=dev)
            Gv = torch.empty(TB, C, Nk, dtype=torch.float32, device=dev)
            gq, gk, gv = Gq.data_ptr(), Gk.data_ptr(), Gv.data_ptr()
            gs = (C * Nq, C * Nk, C * Nk)
            kp, vp = kd.data_ptr(), vd.data_ptr()
            out = (Gq, Gk, Gv)
        ws = torch.empty_like(kv)
        check(lib.s2f_sdsa_bwd_bf16(qp, kp, vp, qs, ks, vs, _ptr(kv), _ptr(g), _ptr(mask) if fuse else 0, D, gq, gk, gv, *gs,
                                    _ptr(ws), TB, heads, d, Nq, Nk, scale, _stream()), "s2f_sdsa_bwd_bf16")
        return _grads(ctx, None, None, None, *out)


class _SDSAMasked(torch.autograd.Function):
    """out = (scale q k^T).masked_fill(mask, 0) v on channel-major fp32 maps (transformer.py:259-272, 343-355; s2f.h
    s2f_sdsa_masked_fwd / _bwd).  mask: uint8 [B, heads, Nq, Nk], shared over the time steps."""

    @staticmethod
    def forward(ctx, q, k, v, mask, heads, scale):
        _need_cuda(q, k, v)
        q, k, v, mask = q.contiguous(), k.contiguous(), v.contiguous(), mask.contiguous()
        TB, C, Nq = q.shape
        Nk = k.shape[2]
        B = mask.shape[0]
        o = torch.empty_like(q)
        check(lib.s2f_sdsa_masked_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(mask), _ptr(o), TB, B, heads, C // heads, Nq, Nk, scale,
                                      _stream()), "s2f_sdsa_masked_fwd")
        ctx.save_for_backward(q, k, v, mask)
        ctx.cfg = (heads, scale)
        return o

    @staticmethod
    def backward(ctx, go):
        q, k, v, mask = ctx.saved_tensors
        heads, scale = ctx.cfg
        go = go.contiguous()
        TB, C, Nq = q.shape
        Nk = k.shape[2]
        gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        check(lib.s2f_sdsa_masked_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(mask), _ptr(go), _ptr(gq), _ptr(gk), _ptr(gv), TB, mask.shape[0],
                                      heads, C // heads, Nq, Nk, scale, _stream()), "s2f_sdsa_masked_bwd")
        return gq, gk, gv, None, None, None


def _tap_sdsa(q, k, v, heads):
    """the two products of the softmax-free core as csrc/sdsa.hip contracts them: k^T v per head, then q (k^T v)"""
    TB, C, Nq = q.shape
    kv, q_kv = sdsa_macs(TB, heads, C // heads, Nq, k.shape[2])
    _TAP[0]("sdsa:kv", None, kv, (("k", k), ("v", v)))
    _TAP[0]("sdsa:q_kv", None, q_kv, (("q", q),))


def _tap_sdsa_stacked(y, dim, heads):
    """the same for q | k | v stacked along `dim` of one spike map"""
    data = y.data if isinstance(y, Spikes) else y
    C = data.shape[dim] // 3
    q, k, v = (data.narrow(dim, i * C, C) for i in range(3))
    if dim == 0:
        q, k, v = q[0], k[0], v[0]
    if isinstance(y, Spikes):
        q, k, v = Spikes(q), Spikes(k), Spikes(v)
    _tap_sdsa(q, k, v, heads)


def sdsa_masked(q, k, v, attn_mask, heads, scale, B):
    """The attention core with an `attn_mask` (True / non-zero = the score is replaced by 0).  q [T*B, C, Nq], k, v [T*B, C, Nk]: fp32
    tensors or Spikes.  attn_mask: b * heads * Nq * Nk booleans in any shape -- the reference reshapes to (t, heads, nq, nk) and
    broadcasts against (t, b, heads, nq, nk), which only runs for t == b and then applies mask[b, h] to every time step; that is the
    semantics here, for any t.  -> fp32 [T*B, C, Nq]."""
    TB, C, Nq = q.shape
    Nk = k.shape[2]
    if C // heads > 64:
        raise NotImplementedError("sdsa_masked: head dimension > 64")
    if attn_mask.numel() != B * heads * Nq * Nk:
        raise RuntimeError(f"attn_mask has {attn_mask.numel()} elements; (batch {B}) x (heads {heads}) x (nq {Nq}) x (nk {Nk}) wanted")
    if _TAP[0] is not None:
        # the mask forbids the q (k^T v) association: q k^T, then (q k^T) v (csrc/sdsa_masked.hip), TB heads Nq Nk d each
        qk, av = sdsa_masked_macs(TB, heads, C // heads, Nq, Nk)
        _TAP[0]("sdsa_masked:qk", None, qk, (("q", q), ("k", k)))
        _TAP[0]("sdsa_masked:av", None, av, (("v", v),))
    m = attn_mask.reshape(B, heads, Nq, Nk).to(device=q.device, dtype=torch.uint8)
    return _SDSAMasked.apply(spikes_float(q), spikes_float(k), spikes_float(v), m, heads, float(scale))


def sdsa(q, k, v, heads, scale, lif=None):
    """o = scale * q (k^T v) on channel-major spike maps.  q, k, v: fp32 tensors or Spikes.  `lif`: the Q_IFNode applied to o
    (the attention's attn_spike); given, the result is its spike map (Spikes) -- from ONE fused kernel when the neuron starts
    from a reset membrane and keeps none and the shapes allow it (backbone self-attention), else core + neuron."""
    if _TAP[0] is not None:
        _tap_sdsa(q, k, v, heads)
    bf = all(isinstance(t, Spikes) and t.tok is not None for t in (q, k, v))
    bf = bf and q.shape[2] % 4 == 0 and k.shape[2] % 4 == 0 and q.shape[1] // heads <= 64
    if not bf:
        o = _SDSA.apply(spikes_float(q), spikes_float(k), spikes_float(v), heads, scale)
        return o if lif is None else lif.fire(o)
    return _sdsa_spikes(q.data, k.data, v.data, q.tok, k.tok, v.tok, heads, scale, False, lif)


def sdsa_packed(y, heads, scale, lif=None):
    """The same with q | k | v = the three channel ranges of one spike map y [TB, 3C, N] (the batched projection chain)."""
    if not (isinstance(y, Spikes) and y.tok is not None and y.shape[2] % 4 == 0 and y.shape[1] // 3 // heads <= 64):
        q, k, v = split3(spikes_float(y))
        return sdsa(q, k, v, heads, scale, lif)
    if _TAP[0] is not None:
        _tap_sdsa_stacked(y, 1, heads)
    return _sdsa_spikes(y.data, None, None, y.tok, None, None, heads, scale, True, lif)


def sdsa_siblings(y, heads, scale, lif=None):
    """The same with q, k, v = the three [TB, C, N] slices of one group-outermost bf16 spike map y [3, TB, C, N] (the decoder's
    sibling projection chains, ops.bn_act_siblings): read in place, one [3, TB, C, N] gradient."""
    if not (isinstance(y, Spikes) and y.tok is not None and y.data.dim() == 4 and y.shape[0] == 3 and y.shape[3] % 4 == 0
            and y.shape[2] // heads <= 64):
        raise RuntimeError("sdsa_siblings: a bf16 spike map [3, TB, C, N] with N % 4 == 0 and heads of at most 64 channels wanted")
    if _TAP[0] is not None:
        _tap_sdsa_stacked(y, 0, heads)
    return _sdsa_spikes(y.data, None, None, y.tok, None, None, heads, scale, 2, lif)


def _sdsa_spikes(qd, kd, vd, qt, kt, vt, heads, scale, packed, lif):
    C = qd.shape[2] if packed == 2 else qd.shape[1] // 3 if packed else qd.shape[1]
    Nq = qd.shape[-1]
    Nk = Nq if packed else kd.shape[2]
    pure = (lif is not None and isinstance(lif.v, float) and not lif.keep_membrane
            and not lif._forward_hooks and not lif._forward_pre_hooks)          # hooks want the module call
    fuse = pure and Nq == Nk and Nq % 256 == 0 and (C * Nq) % 8 == 0 and spikes_bf16_ok(lif.D)
    no_grad = not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (qt, kt, vt)))
    if (pure and no_grad and not packed and Nq % 4 == 0 and Nk % 4 == 0 and spikes_bf16_ok(lif.D) and C // heads <= 64
            and not (Nq == Nk and Nq % 256 == 0)):
        # inference on maps the masked kernel does not take (the decoder's 100 queries): attention core + neuron as one launch pair,
        # o never written (s2f_sdsa_lif_fwd_bf16_nomask)
        qd, kd, vd = qd.contiguous(), kd.contiguous(), vd.contiguous()
        TB = qd.shape[0]
        d = C // heads
        y = torch.empty(TB, C, Nq, dtype=torch.bfloat16, device=qd.device)
        kv = torch.empty(TB, heads, d, d, dtype=torch.float32, device=qd.device)
        if lif.stats is not None:
            lif.stats_elems += TB * C * Nq
        check(lib.s2f_sdsa_lif_fwd_bf16_nomask(_ptr(qd), _ptr(kd), _ptr(vd), C * Nq, C * Nk, C * Nk, _ptr(y), _ptr(lif.stats),
                                               _ptr(kv), TB, heads, d, Nq, Nk, scale, lif.v_threshold, lif.D, _stream()),
              "s2f_sdsa_lif_fwd_bf16_nomask")
        lif.v = 0.0
        return _spikes(None, y)
    if fuse and lif.stats is not None:
        lif.stats_elems += (qd.shape[1] if packed == 2 else qd.shape[0]) * C * Nq
    o, ydata, _ = _SDSASpikes.apply(qd, kd, vd, qt, kt, vt, heads, scale, packed, fuse, lif.D if fuse else 8,
                                    lif.v_threshold if fuse else 1.0, lif.stats if fuse else None)
    if fuse:
        lif.v = 0.0
        return _spikes(o, ydata)
    return o if lif is None else lif.fire(o)


# ------------------------------------------------------------------------------------------------ DCNv3 core
class _DCNv3(torch.autograd.Function):
    """dcnv3_core_pytorch (ops_dcnv3/functions/dcnv3_func.py:147-189), NHWC in/out."""

    @staticmethod
    def forward(ctx, x, offset, mask, kh, kw, sh, sw, ph, pw, dh, dw, G, Cg, offset_scale):
        _need_cuda(x, offset, mask)
        x, offset, mask = x.contiguous(), offset.contiguous(), mask.contiguous()
        N, H, W, _ = x.shape
        Ho, Wo = offset.shape[1], offset.shape[2]
        out = torch.empty(N, Ho, Wo, G * Cg, dtype=torch.float32, device=x.device)
        geo = (N, H, W, G, Cg, kh, kw, sh, sw, ph, pw, dh, dw)
        check(lib.s2f_dcnv3_fwd(_ptr(x), _ptr(offset), _ptr(mask), _ptr(out), *geo, offset_scale, _stream()),
              "s2f_dcnv3_fwd")
        ctx.save_for_backward(x, offset, mask)
        ctx.geo, ctx.osc = geo, offset_scale
        return out

    @staticmethod
    def backward(ctx, go):
        x, offset, mask = ctx.saved_tensors
        go = go.contiguous()
        N, H, W, G, Cg = ctx.geo[:5]
        Ho, Wo = offset.shape[1], offset.shape[2]
        gx = torch.empty_like(x)                      # s2f_dcnv3_bwd overwrites all three gradients
        goff, gm = torch.empty_like(offset), torch.empty_like(mask)
        check(lib.s2f_dcnv3_bwd(_ptr(x), _ptr(offset), _ptr(mask), _ptr(go), _ptr(gx), _ptr(goff), _ptr(gm), *ctx.geo,
                                ctx.osc, _stream()), "s2f_dcnv3_bwd")
        return _grads(ctx, gx, goff, gm)


def _tap_dcnv3(x, offset, mask, kh, kw, G, Cg):
    """per output pixel, group channel and sampling point 4 bilinear taps of x and 1 modulation by the mask: 5 N Ho Wo G Cg K in two
    rows, because the two read different operands (the map; the mask neuron's spikes)"""
    sample, modulate = dcnv3_macs(offset.shape[0], offset.shape[1], offset.shape[2], G, Cg, kh * kw)
    _TAP[0]("dcnv3:sample", None, sample, (("x", x),))
    _TAP[0]("dcnv3:modulate", None, modulate, (("mask", mask),))


def dcnv3_core(x, offset, mask, kh, kw, sh, sw, ph, pw, dh, dw, G, Cg, offset_scale):
    """`mask` may arrive as a Spikes pair (the module's mask neuron): the gather reads it as fp32."""
    if _TAP[0] is not None:
        _tap_dcnv3(x, offset, mask, kh, kw, G, Cg)
    return _DCNv3.apply(x, offset, spikes_float(mask), kh, kw, sh, sw, ph, pw, dh, dw, G, Cg, float(offset_scale))


class _DCNv3CM(torch.autograd.Function):
    """The same core on channel-major maps: x [N, C, H, W] -> [N, C, Ho, Wo]; offset / mask [N, Ho, Wo, .] as above."""

    @staticmethod
    def forward(ctx, x, offset, mask, kh, kw, sh, sw, ph, pw, dh, dw, G, Cg, offset_scale):
        _need_cuda(x, offset, mask)
        x, offset, mask = x.contiguous(), offset.contiguous(), mask.contiguous()
        N, _, H, W = x.shape
        Ho, Wo = offset.shape[1], offset.shape[2]
        out = torch.empty(N, G * Cg, Ho, Wo, dtype=torch.float32, device=x.device)
        geo = (N, H, W, G, Cg, kh, kw, sh, sw, ph, pw, dh, dw)
        check(lib.s2f_dcnv3_fwd_cm(_ptr(x), _ptr(offset), _ptr(mask), _ptr(out), *geo, offset_scale, _stream()),
              "s2f_dcnv3_fwd_cm")
        ctx.save_for_backward(x, offset, mask)
        ctx.geo, ctx.osc = geo, offset_scale
        return out

    @staticmethod
    def backward(ctx, go):
        x, offset, mask = ctx.saved_tensors
        go = go.contiguous()
        gx = torch.empty_like(x)                      # s2f_dcnv3_bwd_cm overwrites all three gradients
        goff, gm = torch.empty_like(offset), torch.empty_like(mask)
        check(lib.s2f_dcnv3_bwd_cm(_ptr(x), _ptr(offset), _ptr(mask), _ptr(go), _ptr(gx), _ptr(goff), _ptr(gm), *ctx.geo,
                                   ctx.osc, _stream()), "s2f_dcnv3_bwd_cm")
        return _grads(ctx, gx, goff, gm)


def dcnv3_cm_ok(N, H, W, kh, kw, sh, sw, ph, pw, dh, dw, G, Cg):
    """An (image, group) slice of this geometry fits one workgroup's LDS: dcnv3_core_cm takes it (no launch)."""
    return bool(lib.s2f_dcnv3_cm_ok(N, H, W, G, Cg, kh, kw, sh, sw, ph, pw, dh, dw))


# include/s2f.h: the route ids of s2f_dcnv3_route (tests/test_abi.py holds every one against its #define)
DCN_ROUTE_FIELDS = 7
DCN_FWD_K3C8, DCN_FWD_VEC4, DCN_FWD_SCALAR = 1, 2, 3
DCN_BWD_LDS, DCN_BWD_BANDED, DCN_BWD_ATOMIC_VEC4, DCN_BWD_ATOMIC_SCALAR = 11, 12, 13, 14
DCN_CM_FWD_K3C8, DCN_CM_FWD_GENERIC = 21, 22
DCN_CM_BWD_PLAIN, DCN_CM_BWD_PIPE, DCN_CM_BWD_PIPE_K3C8 = 31, 32, 33


def dcnv3_route(N, H, W, kh, kw, sh, sw, ph, pw, dh, dw, G, Cg, aligned16=True):
    """The kernels dcnv3_core / dcnv3_core_cm run for this geometry, from the function the entry points dispatch on (no launch):
    {fwd, bwd, bands, cm, cm_fwd, cm_rs, cm_bwd} with the DCN_* ids above; `aligned16`: the maps start at multiples of 16 bytes
    (every tensor the allocator hands out does)."""
    out = (ctypes.c_int * DCN_ROUTE_FIELDS)()
    check(lib.s2f_dcnv3_route(N, H, W, G, Cg, kh, kw, sh, sw, ph, pw, dh, dw, int(bool(aligned16)), out), "s2f_dcnv3_route")
    return dict(zip(("fwd", "bwd", "bands", "cm", "cm_fwd", "cm_rs", "cm_bwd"), out))


def dcnv3_core_cm(x, offset, mask, kh, kw, sh, sw, ph, pw, dh, dw, G, Cg, offset_scale):
    """dcnv3_core on channel-major maps, x [N, C, H, W] -> [N, C, Ho, Wo], without the transposition pair around the NHWC core;
    for geometries with dcnv3_cm_ok (any other is an error here: the caller keeps the transposing route for them)."""
    if _TAP[0] is not None:
        _tap_dcnv3(x, offset, mask, kh, kw, G, Cg)
    return _DCNv3CM.apply(x, offset, spikes_float(mask), kh, kw, sh, sw, ph, pw, dh, dw, G, Cg, float(offset_scale))



__all__ = [n for n in dir() if not n.startswith('__')]
