"""Tiled transposes (csrc/transpose.hip) and the fan-out of one tensor to n readers (s2f_sum_n of csrc/glue.hip)."""
import torch

from .config import cfg
from .core import *          # noqa: F401,F403  (the shared plumbing: _ptr, _stream, check, lib, Spikes, ...)


def _transpose_fwd(x):
    B, R, C = x.shape
    y = torch.empty(B, C, R, dtype=torch.float32, device=x.device)
    check(lib.s2f_transpose_last2(_ptr(x), _ptr(y), B, R, C, _stream()), "s2f_transpose_last2")
    return y


def _transpose_bwd_add(gy, gskip, gx):
    B, C, R = gy.shape
    check(lib.s2f_transpose_last2_add(_ptr(gy), _ptr(gskip), _ptr(gx), B, C, R, _stream()), "s2f_transpose_last2_add")


_TransposeLast2 = _pass_through_function(
    "_TransposeLast2",
    """x [B, R, C] -> [B, C, R], contiguous (the adjoint is the same kernel the other way round).  -> (x^T, pass-through of x or an
    empty stand-in): the pass-through serves a second reader of x, whose gradient the adjoint sums (s2f_transpose_last2_add).""",
    _transpose_fwd, _transpose_bwd_add)


class _FanOut(torch.autograd.Function):
    """x -> n aliases of x, one per reader; backward: the readers' gradients summed by ONE launch (s2f_sum_n) in the order the autograd
    engine would have accumulated them (last reader first) -- instead of n - 1 add launches (cfg.FANOUT_PORTS; the decoder's query
    position embedding has twelve readers per step)."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        live = [g.contiguous() for g in reversed(gs) if g is not None]
        if not live:
            return None, None
        if len(live) == 1:
            return live[0], None
        import ctypes
        out = torch.empty_like(live[0])
        while len(live) > 1:          # (16 addends per launch)
            part = live[:16]
            arr = (ctypes.c_void_p * len(part))(*[t.data_ptr() for t in part])
            check(lib.s2f_sum_n(arr, len(part), _ptr(out), out.numel(), _stream()), "s2f_sum_n")
            live = [out] + live[16:]
            if len(live) > 1:
                out = torch.empty_like(out)
        return live[0], None


def fan_out(x, n):
    """-> n tensors that are x, for n readers whose gradients one launch sums (float32 CUDA tensors with cfg.FANOUT_PORTS; otherwise
    x itself n times: the autograd engine adds)"""
    if n > 1 and cfg.FANOUT_PORTS and x.is_cuda and x.dtype == torch.float32 and x.requires_grad and torch.is_grad_enabled():
        return list(_FanOut.apply(x, n))
    return [x] * n


class _TransposeScaleAdd(torch.autograd.Function):
    """q + g[c] * x^T: x [B, R, C] token-major, q [B, C, R] channel-major, g [C] (s2f.h s2f_transpose_scale_add_fwd/bwd)."""

    @staticmethod
    def forward(ctx, x, q, g):
        _need_cuda(x, q, g)
        x, q, g = x.contiguous(), q.contiguous(), g.contiguous()
        B, R, C = x.shape
        y = torch.empty_like(q)
        check(lib.s2f_transpose_scale_add_fwd(_ptr(x), _ptr(q), _ptr(g), _ptr(y), B, R, C, _stream()), "s2f_transpose_scale_add_fwd")
        ctx.save_for_backward(x, g)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, g = ctx.saved_tensors
        gy = gy.contiguous()
        B, R, C = x.shape
        gx = torch.empty_like(x)
        gg = torch.zeros_like(g)
        check(lib.s2f_transpose_scale_add_bwd(_ptr(gy), _ptr(x), _ptr(g), _ptr(gx), _ptr(gg), B, R, C, _stream()),
              "s2f_transpose_scale_add_bwd")
        return gx, gy, gg


def transpose_scale_add(x, q, g):
    """q [..., C, R] + g[c] * x[..., R, C]^T in one pass (the layer-scaled FFN residual of the pixel decoder); falls back to
    transpose + addcmul for shapes the kernel does not take."""
    R, C = x.shape[-2:]
    if x.dtype == torch.float32 and x.is_cuda and R % 64 == 0 and C % 64 == 0 and g.data_ptr() % 16 == 0:
        return _TransposeScaleAdd.apply(x.reshape(-1, R, C), q.reshape(-1, C, R), g).view(q.shape)
    return torch.addcmul(q, transpose_last2(x).view(q.shape), g.view(*([1] * (q.dim() - 2)), C, 1))


def transpose_last2(x, skip=False):
    """x [..., R, C] (fp32, CUDA) -> contiguous [..., C, R]: the `.permute(...).contiguous()` copies around the DCNv3 sampling
    core as one tiled kernel (s2f_transpose_last2).  `skip`: -> (x^T, x') with x' = x for a second reader of x, whose gradient the
    adjoint kernel sums (cfg.FANOUT_PORTS; x' is x itself where that does not apply)."""
    lead = x.shape[:-2]
    R, C = x.shape[-2:]
    if x.dtype != torch.float32 or x.numel() == 0:
        y = x.transpose(-1, -2).contiguous()
        return (y, x) if skip else y
    port = bool(skip and cfg.FANOUT_PORTS and x.is_cuda)
    y, through = _TransposeLast2.apply(x.reshape(-1, R, C), port)
    y = y.view(*lead, C, R)
    return (y, through.view(x.shape) if port else x) if skip else y


__all__ = [n for n in dir() if not n.startswith('__')]
