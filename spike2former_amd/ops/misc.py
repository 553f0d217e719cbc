"""Tiled transposes, exact-2x and general bilinear resizing, the mask-loss kernels of the Hungarian-matched loss."""
import numpy as _np
import torch

from .config import cfg
from .core import *          # noqa: F401,F403  (the shared plumbing: _ptr, _stream, check, lib, Spikes, ...)


# ------------------------------------------------------------------------------------------------ transposition
import os as _os
_SMALL_PORTS = _os.environ.get("S2F_FANOUT_SMALL", "1") != "0"          # A/B switch of the two ports on small decoder tensors


class _TransposeLast2(torch.autograd.Function):
    """x [B, R, C] -> [B, C, R], contiguous (the adjoint is the same kernel the other way round).  -> (x^T, pass-through of x or an
    empty stand-in): the pass-through serves a second reader of x, whose gradient the adjoint sums (s2f_transpose_last2_add)."""

    @staticmethod
    def forward(ctx, x, skip):
        _need_cuda(x)
        x_in = x
        x = x.contiguous()
        B, R, C = x.shape
        y = torch.empty(B, C, R, dtype=torch.float32, device=x.device)
        check(lib.s2f_transpose_last2(_ptr(x), _ptr(y), B, R, C, _stream()), "s2f_transpose_last2")
        ctx.set_materialize_grads(False)
        if skip:
            return y, x_in
        aux = x.new_empty(0)
        ctx.mark_non_differentiable(aux)
        return y, aux

    @staticmethod
    def backward(ctx, gy, gskip):
        if gy is None:
            return gskip, None
        gy = gy.contiguous()
        B, C, R = gy.shape
        gx = torch.empty(B, R, C, dtype=torch.float32, device=gy.device)
        if gskip is not None:
            gskip = gskip.contiguous()
        check(lib.s2f_transpose_last2_add(_ptr(gy), _ptr(gskip), _ptr(gx), B, C, R, _stream()), "s2f_transpose_last2_add")
        return gx, None


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
    if n > 1 and cfg.FANOUT_PORTS and _SMALL_PORTS and x.is_cuda and x.dtype == torch.float32 and x.requires_grad and torch.is_grad_enabled():
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
    if skip and cfg.FANOUT_PORTS and _SMALL_PORTS and x.is_cuda:
        y, through = _TransposeLast2.apply(x.reshape(-1, R, C), True)
        return y.view(*lead, C, R), through.view(x.shape)
    y = _TransposeLast2.apply(x.reshape(-1, R, C), False)[0].view(*lead, C, R)
    return (y, x) if skip else y


# ------------------------------------------------------------------------------------------------ reductions / fills (csrc/glue.hip)
def channel_sum(x):
    """x [N, C, L] fp32 -> [C] = x.sum((0, 2)) on s2f_channel_sum (partials stored, added in order: bit-repeatable); ATen for rows
    that are no whole 16-byte groups."""
    N, C, L = x.shape
    if not (x.is_cuda and x.dtype == torch.float32 and L % 4 == 0 and x.numel() > 0 and C < 65536):
        return x.sum((0, 2))
    x = x.contiguous()
    ws = torch.empty(C * int(lib.s2f_channel_sum_slices(N, C, L)), dtype=torch.float32, device=x.device)
    out = torch.empty(C, dtype=torch.float32, device=x.device)
    check(lib.s2f_channel_sum(_ptr(x), N, C, L, _ptr(ws), _ptr(out), 0, _stream()), "s2f_channel_sum")
    return out


def sum_lead(x):
    """x [T, ...] fp32 -> x.sum(0) on s2f_sum_lead"""
    T = x.shape[0]
    M = x.numel() // max(T, 1)
    if not (x.is_cuda and x.dtype == torch.float32 and M % 4 == 0 and x.numel() > 0):
        return x.sum(0)
    x = x.contiguous()
    out = torch.empty(x.shape[1:], dtype=torch.float32, device=x.device)
    check(lib.s2f_sum_lead(_ptr(x), T, M, _ptr(out), _stream()), "s2f_sum_lead")
    return out


def _dense_flat(x):
    """x as a flat view of the memory it covers when its elements are a permutation of one dense block (any permuted view of a
    contiguous tensor), else None"""
    if x.numel() == 0:
        return None
    dims = sorted((st, sz) for st, sz in zip(x.stride(), x.shape) if sz > 1)
    run = 1
    for st, sz in dims:
        if st != run:
            return None
        run *= sz
    return x.as_strided((x.numel(),), (1,))


class _MeanAll(torch.autograd.Function):
    """x.mean() over a whole tensor (the benchmark's headline loss terms).  Forward: s2f_sum_all over the memory x covers (a permuted
    view sums to the same value).  Backward: the constant g / n written ONCE, by s2f_fill, with x's own strides -- the gradient of
    the permuted logits view is then a plain tensor in the contraction's layout and the consumer's .contiguous() is a no-op.  (torch's
    formula materialises expand(g) / n in the view's layout and the consumer copies it into its own: two passes over 367 MB at C2.)"""

    @staticmethod
    def forward(ctx, x):
        flat = _dense_flat(x) if (x.is_cuda and x.dtype == torch.float32) else None
        ctx.meta = (x.shape, x.stride(), flat is not None)
        if flat is None or flat.data_ptr() % 16 != 0:
            ctx.meta = (x.shape, x.stride(), False)
            return x.mean()
        n = flat.numel()
        part = torch.empty(int(lib.s2f_sum_all_parts(n)), dtype=torch.float32, device=x.device)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        check(lib.s2f_sum_all(_ptr(flat), n, 1.0 / n, _ptr(part), _ptr(out), _stream()), "s2f_sum_all")
        return out

    @staticmethod
    def backward(ctx, g):
        shape, stride, ours = ctx.meta
        n = 1
        for d in shape:
            n *= d
        if not ours:
            return (g / n).expand(shape)
        gx = torch.empty_strided(shape, stride, dtype=torch.float32, device=g.device)
        check(lib.s2f_fill(_ptr(gx), n, _ptr(g.contiguous()), 1.0 / n, _stream()), "s2f_fill")
        return gx


def mean_all(x):
    return _MeanAll.apply(x)


# ------------------------------------------------------------------------------------------------ 2x bilinear up-sampling
class _Up2x(torch.autograd.Function):
    """-> (up-sampled map, pass-through of x or an empty stand-in): the pass-through serves a second reader of x; the gradient it
    sends back is summed inside the adjoint kernel (s2f_upsample2x_bwd_add) instead of by an add of the autograd engine."""

    @staticmethod
    def forward(ctx, x, skip):
        _need_cuda(x)
        x_in = x
        x = x.contiguous()
        N, C, h, w = x.shape
        y = torch.empty(N, C, 2 * h, 2 * w, dtype=torch.float32, device=x.device)
        check(lib.s2f_upsample2x_fwd(_ptr(x), _ptr(y), N * C, h, w, _stream()), "s2f_upsample2x_fwd")
        ctx.shape = (N, C, h, w)
        ctx.set_materialize_grads(False)
        if skip:
            return y, x_in
        aux = x.new_empty(0)
        ctx.mark_non_differentiable(aux)
        return y, aux

    @staticmethod
    def backward(ctx, gy, gskip):
        N, C, h, w = ctx.shape
        if gy is None:
            return gskip, None
        gy = gy.contiguous()
        if gskip is not None:
            gskip = gskip.contiguous()
        gx = torch.empty(N, C, h, w, dtype=torch.float32, device=gy.device)
        check(lib.s2f_upsample2x_bwd_add(_ptr(gy), _ptr(gskip), _ptr(gx), N * C, h, w, _stream()), "s2f_upsample2x_bwd_add")
        return gx, None


class _Resize(torch.autograd.Function):
    """F.interpolate(x, size, mode='bilinear') for any sizes on s2f_resize_fwd; backward: the gather adjoint s2f_resize_bwd_add
    (no atomics: bit-repeatable).  -> (y, pass-through of x or an empty stand-in), the pass-through as in _Up2x: the gradient of a
    second reader of x is summed inside the adjoint kernel."""

    @staticmethod
    def forward(ctx, x, size, align_corners, skip):
        _need_cuda(x)
        x_in = x
        x = x.contiguous()
        N, C, h, w = x.shape
        H, W = size
        y = torch.empty(N, C, H, W, dtype=torch.float32, device=x.device)
        flags = lib_flags(align_corners)
        check(lib.s2f_resize_fwd(_ptr(x), _ptr(y), N * C, h * w, w, 0, 0, h, w, H, W, flags, _stream()), "s2f_resize_fwd")
        ctx.meta = (N, C, h, w, H, W, flags)
        ctx.set_materialize_grads(False)
        if skip:
            return y, x_in
        aux = x.new_empty(0)
        ctx.mark_non_differentiable(aux)
        return y, aux

    @staticmethod
    def backward(ctx, gy, gskip):
        N, C, h, w, H, W, flags = ctx.meta
        if gy is None:
            return gskip, None, None, None
        gy = gy.contiguous()
        if gskip is not None:
            gskip = gskip.contiguous()
        gx = torch.empty(N, C, h, w, dtype=torch.float32, device=gy.device)
        check(lib.s2f_resize_bwd_add(_ptr(gy), _ptr(gskip), _ptr(gx), N * C, h, w, H, W, flags, _stream()), "s2f_resize_bwd_add")
        return gx, None, None, None


RESIZE_ALIGN_CORNERS, RESIZE_SIGMOID, RESIZE_FLIP_H, RESIZE_FLIP_V = 1, 2, 4, 8       # include/s2f.h S2F_RESIZE_*


def lib_flags(align_corners=False, sigmoid=False, flip=None):
    """the S2F_RESIZE_* flags word; flip: None | 'horizontal' | 'vertical'"""
    return ((RESIZE_ALIGN_CORNERS if align_corners else 0) | (RESIZE_SIGMOID if sigmoid else 0)
            | (RESIZE_FLIP_H if flip == "horizontal" else 0) | (RESIZE_FLIP_V if flip == "vertical" else 0))


def _general_ok(x):
    return cfg.GENERAL_RESIZE and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.numel() > 0


def resize_bilinear(x, size, align_corners=False, sigmoid=False, skip=False):
    """F.interpolate(x [N, C, h, w], size, mode='bilinear', align_corners) (.sigmoid() after it with `sigmoid`) on the general
    kernel s2f_resize_fwd, any sizes; differentiable (s2f_resize_bwd_add) unless `sigmoid`, which is for inference only.
    `skip`: -> (y, x') as upsample_bilinear's."""
    H, W = (int(v) for v in size)
    if sigmoid:
        assert not skip and not (torch.is_grad_enabled() and x.requires_grad), "the fused sigmoid has no adjoint"
        _need_cuda(x)
        x = x.contiguous()
        N, C, h, w = x.shape
        y = torch.empty(N, C, H, W, dtype=torch.float32, device=x.device)
        check(lib.s2f_resize_fwd(_ptr(x), _ptr(y), N * C, h * w, w, 0, 0, h, w, H, W, lib_flags(align_corners, True), _stream()),
              "s2f_resize_fwd")
        return y
    if skip:
        if cfg.FANOUT_PORTS:
            return _Resize.apply(x, (H, W), bool(align_corners), True)
        return _Resize.apply(x, (H, W), bool(align_corners), False)[0], x
    return _Resize.apply(x, (H, W), bool(align_corners), False)[0]


def upsample_bilinear(x, size, sigmoid=False, skip=False):
    """F.interpolate(x, size, mode='bilinear', align_corners=False); the exact-2x even-width case runs the 2x kernels, every other
    fp32 CUDA [N, C, h, w] map the general resize (s2f_resize_fwd / s2f_resize_bwd_add).  `sigmoid`: followed by .sigmoid() --
    inside the same pass where no gradient is wanted (the inference post-processing).
    `skip`: -> (y, x') with x' = x for a second reader of x, whose gradient the adjoint kernel then sums (cfg.FANOUT_PORTS; x' is x
    itself where that does not apply)."""
    h, w = x.shape[-2:]
    two_x = tuple(size) == (2 * h, 2 * w) and w % 2 == 0
    if skip:
        if cfg.FANOUT_PORTS and two_x and x.dim() == 4 and x.is_cuda and not sigmoid:
            return _Up2x.apply(x, True)
        if not two_x and not sigmoid and _general_ok(x):
            return resize_bilinear(x, size, skip=True)
        return upsample_bilinear(x, size, sigmoid), x
    if two_x:
        if sigmoid and w % 4 == 0 and x.dim() == 4 and not (torch.is_grad_enabled() and x.requires_grad):
            _need_cuda(x)
            x = x.contiguous()
            N, C = x.shape[:2]
            y = torch.empty(N, C, 2 * h, 2 * w, dtype=torch.float32, device=x.device)
            check(lib.s2f_upsample2x_sigmoid_fwd(_ptr(x), _ptr(y), N * C, h, w, _stream()), "s2f_upsample2x_sigmoid_fwd")
            return y
        y = _Up2x.apply(x, False)[0]
        return y.sigmoid() if sigmoid else y
    if _general_ok(x):
        if sigmoid and not (torch.is_grad_enabled() and x.requires_grad):
            return resize_bilinear(x, size, sigmoid=True)
        y = resize_bilinear(x, size)
        return y.sigmoid() if sigmoid else y
    fallback("upsample_bilinear", f"{(h, w)} -> {tuple(size)}")
    y = torch.nn.functional.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False)
    return y.sigmoid() if sigmoid else y


# ------------------------------------------------------------------------------------------------ inference post-processing
def _window(x, crop):
    """x [K, Hp, Wp] (a plane-contiguous map) and crop = (top, bottom, left, right) -> (plane stride, row stride, row0, col0, h, w)"""
    Hp, Wp = x.shape[-2:]
    top, bottom, left, right = (int(v) for v in (crop or (0, 0, 0, 0)))
    assert x.stride(-1) == 1 and x.stride(-2) == Wp and x.stride(0) == Hp * Wp, "a contiguous [K, H, W] map"
    return Hp * Wp, Wp, top, left, Hp - top - bottom, Wp - left - right


def resize_window(x, size, crop=None, flip=None, align_corners=False, sigmoid=False):
    """x [K, Hp, Wp] fp32 CUDA -> [K, H, W]: the window x[:, top:Hp-bottom, left:Wp-right] (crop = (top, bottom, left, right)),
    flipped (None | 'horizontal' | 'vertical'), bilinearly resized to `size` (then sigmoid) -- one s2f_resize_fwd pass, no copy of
    the window (EncoderDecoder.postprocess_result)."""
    _need_cuda(x)
    x = x.contiguous()
    ps, ld, r0, c0, h, w = _window(x, crop)
    H, W = (int(v) for v in size)
    y = torch.empty(x.shape[0], H, W, dtype=torch.float32, device=x.device)
    check(lib.s2f_resize_fwd(_ptr(x), _ptr(y), x.shape[0], ps, ld, r0, c0, h, w, H, W, lib_flags(align_corners, sigmoid, flip),
                             _stream()), "s2f_resize_fwd")
    return y


def seg_argmax(x, threshold=0.3, sigmoid=False, float_out=False):
    """x [K, H, W] fp32 CUDA -> [1, H, W]: K > 1 the int64 arg-max over K (torch.argmax: first maximum, NaN wins); K == 1
    (sigmoid(x) if `sigmoid` else x) > threshold as int64 or, with float_out, as float 0 / 1 (s2f_seg_argmax)."""
    _need_cuda(x)
    x = x.contiguous()
    K, H, W = x.shape
    f = float_out and K == 1
    out = torch.empty(1, H, W, dtype=torch.float32 if f else torch.int64, device=x.device)
    check(lib.s2f_seg_argmax(_ptr(x), None if f else _ptr(out), _ptr(out) if f else None, K, H * W, int(sigmoid), float(threshold),
                             _stream()), "s2f_seg_argmax")
    return out


def seg_label(x, size, crop=None, flip=None, align_corners=False, threshold=0.3):
    """x [K, Hp, Wp] fp32 CUDA -> the label map [1, H, W] of its window resized to `size`: int64 arg-max for K > 1, float 0 / 1
    (sigmoid > threshold) for K == 1 -- the bits of seg_argmax(resize_window(x, size, crop, flip, align_corners, sigmoid=K == 1),
    threshold, float_out=True) in ONE launch with no [K, H, W] intermediate (s2f_seg_label)."""
    _need_cuda(x)
    x = x.contiguous()
    ps, ld, r0, c0, h, w = _window(x, crop)
    K = x.shape[0]
    H, W = (int(v) for v in size)
    f = K == 1
    out = torch.empty(1, H, W, dtype=torch.float32 if f else torch.int64, device=x.device)
    check(lib.s2f_seg_label(_ptr(x), None if f else _ptr(out), _ptr(out) if f else None, K, ps, ld, r0, c0, h, w, H, W,
                            lib_flags(align_corners, False, flip), float(threshold), _stream()), "s2f_seg_label")
    return out


def tta_accumulate(acc, x, first, crop=None, flip=None, align_corners=False, pre_sigmoid=False):
    """acc [K, H, W] (first ? = : +=) softmax over K of x's window (crop / flip / resize as resize_window) -- K == 1: sigmoid,
    after a first one with pre_sigmoid (s2f_tta_accumulate; mmseg seg_tta.py:29-34)"""
    _need_cuda(x, acc)
    x = x.contiguous()
    assert acc.is_contiguous() and acc.dtype == torch.float32 and acc.shape[0] == x.shape[0]
    ps, ld, r0, c0, h, w = _window(x, crop)
    K, H, W = acc.shape
    check(lib.s2f_tta_accumulate(_ptr(x), _ptr(acc), K, ps, ld, r0, c0, h, w, H, W, lib_flags(align_corners, pre_sigmoid, flip),
                                 int(bool(first)), _stream()), "s2f_tta_accumulate")
    return acc


def tta_finish(acc, n_views, threshold=0.3):
    """acc [K, H, W] /= n_views in place; -> the int64 arg-max [1, H, W] (K > 1) or the float 0 / 1 map acc > threshold (K == 1),
    as seg_tta.py:35-40 (s2f_tta_finish)"""
    _need_cuda(acc)
    assert acc.is_contiguous() and acc.dtype == torch.float32
    K, H, W = acc.shape
    out = torch.empty(1, H, W, dtype=torch.float32 if K == 1 else torch.int64, device=acc.device)
    f = K == 1
    check(lib.s2f_tta_finish(_ptr(acc), None if f else _ptr(out), _ptr(out) if f else None, K, H * W, int(n_views), float(threshold),
                             _stream()), "s2f_tta_finish")
    return out


def _pair(v):
    a, b = v
    return int(a), int(b)


def slide_grid(H, W, crop, stride):
    """-> (ny, nx, eh, ew): the window grid of sliding-window inference for an [H, W] picture (include/s2f.h "sliding-window
    inference"; mmseg encoder_decoder.py:262-273): ny x nx windows of eh x ew = min(crop, size) pixels, window i of an axis starting
    at min(i * stride, size - extent).  Host arithmetic."""
    H, W = int(H), int(W)
    (ch, cw), (sh, sw) = _pair(crop), _pair(stride)
    if min(H, W, ch, cw, sh, sw) <= 0:
        raise ValueError(f"slide_grid: sizes, crop and stride are positive, got {(H, W)}, {(ch, cw)}, {(sh, sw)}")
    return max(H - ch + sh - 1, 0) // sh + 1, max(W - cw + sw - 1, 0) // sw + 1, min(ch, H), min(cw, W)


def slide_windows(inputs, crop, stride, w0, n):
    """inputs [B, C, H, W] fp32 CUDA contiguous -> [n, B, C, eh, ew]: windows w0 .. w0 + n - 1 of slide_grid (row-major), window-major,
    in one launch (s2f_slide_windows).  There is no other route: a CPU tensor raises."""
    _need_cuda(inputs)
    assert inputs.dtype == torch.float32 and inputs.dim() == 4 and inputs.is_contiguous(), "a contiguous fp32 [B, C, H, W] input"
    B, C, H, W = inputs.shape
    ny, nx, eh, ew = slide_grid(H, W, crop, stride)
    out = torch.empty(int(n), B, C, eh, ew, dtype=torch.float32, device=inputs.device)
    check(lib.s2f_slide_windows(_ptr(inputs), _ptr(out), B, C, H, W, *_pair(crop), *_pair(stride), int(w0), int(n), _stream()),
          "s2f_slide_windows")
    return out


def slide_accumulate(preds, logits, crop, stride, w0):
    """preds [B, K, H, W] <- the merge of logits [n, B, K, eh, ew], the logits of windows w0 .. w0 + n - 1 (s2f_slide_accumulate): per
    covered pixel the windows are added in increasing index -- from +0.0 when the group holds the pixel's first window, else from
    the stored value -- and divided by the pixel's coverage count when it holds the last.  Groups go in increasing w0; preds may
    start uninitialised; after the last group it is mmseg's slide_inference result, bit for bit.  Both fp32 CUDA contiguous."""
    _need_cuda(preds, logits)
    assert preds.dtype == torch.float32 and preds.dim() == 4 and preds.is_contiguous(), "a contiguous fp32 [B, K, H, W] map"
    B, K, H, W = preds.shape
    ny, nx, eh, ew = slide_grid(H, W, crop, stride)
    assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.device == preds.device, "contiguous fp32 logits on preds' device"
    n = logits.numel() // max(B * K * eh * ew, 1)
    assert n > 0 and logits.numel() == n * B * K * eh * ew and tuple(logits.shape[-2:]) == (eh, ew), \
        f"logits {tuple(logits.shape)} are not [n, {B}, {K}, {eh}, {ew}]"
    check(lib.s2f_slide_accumulate(_ptr(logits), _ptr(preds), B, K, H, W, *_pair(crop), *_pair(stride), int(w0), n, _stream()),
          "s2f_slide_accumulate")
    return preds


# ------------------------------------------------------------------------------------------------ training augmentation, test-time views
AUG_CANDIDATES = 11                  # include/s2f.h S2F_AUG_CANDIDATES
AUG_MAX_CROP = 4096                  # include/s2f.h S2F_AUG_MAX_CROP
AUG_PARAM_BYTES, VIEW_PARAM_BYTES = lib.s2f_aug_param_bytes(), lib.s2f_view_param_bytes()
# include/s2f.h S2fAugParams and S2fViewParams, field for field (augment.py writes the tables)
PARAM_DTYPE = _np.dtype([
    ("img_off", "<i8"), ("seg_off", "<i8"), ("h0", "<i4"), ("w0", "<i4"), ("H", "<i4"), ("W", "<i4"),
    ("crop_y", "<i4", (AUG_CANDIDATES,)), ("crop_x", "<i4", (AUG_CANDIDATES,)), ("flip", "<i4"),
    ("bright_on", "<i4"), ("mode", "<i4"), ("contrast_on", "<i4"), ("sat_on", "<i4"), ("hue_on", "<i4"), ("hue_delta", "<i4"),
    ("bright_beta", "<f4"), ("contrast_alpha", "<f4"), ("sat_alpha", "<f4")])
VIEW_PARAM_DTYPE = _np.dtype([("img_off", "<i8"), ("out_off", "<i8"), ("h0", "<i4"), ("w0", "<i4"), ("H", "<i4"), ("W", "<i4"),
                              ("Hp", "<i4"), ("Wp", "<i4"), ("flip", "<i4"), ("reserved", "<i4")])
assert PARAM_DTYPE.itemsize == AUG_PARAM_BYTES, "PARAM_DTYPE does not mirror S2fAugParams"
assert VIEW_PARAM_DTYPE.itemsize == VIEW_PARAM_BYTES, "VIEW_PARAM_DTYPE does not mirror S2fViewParams"


def _aug_cuda(*ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("spike2former_amd ops run on the GPU only (HIP kernels); got a CPU tensor")


def _mean_std(mean, std):
    """SegDataPreProcessor's mean and std (both or neither: no normalisation) -> two lists of three floats"""
    if (mean is None) != (std is None):
        raise ValueError("mean and std go together")
    m = [float(v) for v in mean] if mean is not None else [0.0] * 3
    s = [float(v) for v in std] if std is not None else [1.0] * 3
    if len(m) != 3 or len(s) != 3:
        raise ValueError("mean and std have three values")
    return m, s


def _byte_buffer(t, what="data"):
    if not (t.dtype == torch.uint8 and t.dim() == 1 and t.is_contiguous()):
        raise ValueError(f"{what}: one contiguous uint8 byte buffer")


def _staged_table(t, entry_bytes, least=1):
    """a table as staged in device memory: whole entries of entry_bytes, at least `least`, as one uint8 buffer -> their number"""
    _byte_buffer(t, "the parameter table")
    if t.numel() % entry_bytes or t.numel() < least * entry_bytes:
        raise ValueError(f"the parameter table: {least} or more entries of {entry_bytes} bytes, got {t.numel()} bytes")
    _aug_cuda(t)
    return t.numel() // entry_bytes


def aug_crop_stats(data, params, flags, crop_size, ignore_index=255, reduce_zero_label=False, cat_max_ratio=0.75):
    """flags int32 [B, 11] <- RandomCrop.crop_bbox's test of every candidate crop window of the nearest-resized annotations
    (s2f_aug_crop_stats).  data: the batch's packed uint8 pictures and annotations; params: the B-entry table (S2fAugParams) as
    bytes; both CUDA.  There is no other route: a CPU tensor raises."""
    _byte_buffer(data)
    B = _staged_table(params, AUG_PARAM_BYTES)
    _aug_cuda(data, flags)
    assert flags.dtype == torch.int32 and flags.is_contiguous() and tuple(flags.shape) == (B, AUG_CANDIDATES)
    Hc, Wc = (int(v) for v in crop_size)
    check(lib.s2f_aug_crop_stats(_ptr(data), data.numel(), _ptr(params), B, Hc, Wc, int(ignore_index), int(bool(reduce_zero_label)),
                                 float(cat_max_ratio), _ptr(flags), _stream()), "s2f_aug_crop_stats")
    return flags


def aug_apply(data, params, flags, inputs, seg, mean=None, std=None, bgr_to_rgb=False, pad_val=0.0, seg_pad_val=255,
              reduce_zero_label=False):
    """inputs fp32 [B, 3, Hc, Wc] and seg uint8 [B, Hc, Wc] <- resize, chosen crop, flip, photometric distortion, channel swap,
    normalisation and padding of every picture of the batch in one launch that writes every element once (s2f_aug_apply).
    flags: what aug_crop_stats wrote, or None (candidate 0).  There is no other route: a CPU tensor raises."""
    _byte_buffer(data)
    m, s = _mean_std(mean, std)
    B = _staged_table(params, AUG_PARAM_BYTES)
    _aug_cuda(data, inputs, seg)
    assert inputs.dtype == torch.float32 and inputs.is_contiguous() and inputs.dim() == 4 and inputs.shape[:2] == (B, 3)
    Hc, Wc = (int(v) for v in inputs.shape[-2:])
    assert seg.dtype == torch.uint8 and seg.is_contiguous() and tuple(seg.shape) == (B, Hc, Wc)
    if flags is not None:
        _aug_cuda(flags)
        assert flags.dtype == torch.int32 and flags.is_contiguous() and tuple(flags.shape) == (B, AUG_CANDIDATES)
    check(lib.s2f_aug_apply(_ptr(data), data.numel(), _ptr(params), _ptr(flags), B, Hc, Wc, *m, *s, int(bool(bgr_to_rgb)),
                            float(pad_val), int(seg_pad_val), int(bool(reduce_zero_label)), _ptr(inputs), _ptr(seg), _stream()),
          "s2f_aug_apply")
    return inputs, seg


def check_view_table(table, data_bytes, out_elems):
    """The rules of s2f_test_views on a table the host wrote, before it is launched on: every picture inside data, every block
    inside out, 0 < H <= Hp <= AUG_MAX_CROP (W alike), out_off a multiple of 4, the blocks disjoint.  ValueError names the entry."""
    table = _np.asarray(table)
    if table.dtype != VIEW_PARAM_DTYPE or table.ndim != 1 or not 0 < len(table) <= 65535:
        raise ValueError(f"table: 1 .. 65535 entries of VIEW_PARAM_DTYPE, got {table.dtype} {table.shape}")
    spans = []
    for v, p in enumerate(table):
        img_off, out_off, h0, w0, H, W, Hp, Wp = (int(p[k]) for k in ("img_off", "out_off", "h0", "w0", "H", "W", "Hp", "Wp"))
        if h0 <= 0 or w0 <= 0 or h0 * w0 >= 2 ** 31:
            raise ValueError(f"view table entry {v}: bad source size {h0} x {w0}")
        if img_off < 0 or img_off + 3 * h0 * w0 > data_bytes:
            raise ValueError(f"view table entry {v}: the source picture (bytes {img_off} .. {img_off + 3 * h0 * w0}) leaves data "
                             f"({data_bytes} bytes)")
        if not (0 < H <= Hp <= AUG_MAX_CROP and 0 < W <= Wp <= AUG_MAX_CROP):
            raise ValueError(f"view table entry {v}: resized {H} x {W}, padded {Hp} x {Wp}: need 0 < H <= Hp <= {AUG_MAX_CROP} and "
                             f"0 < W <= Wp <= {AUG_MAX_CROP}")
        if out_off % 4:
            raise ValueError(f"view table entry {v}: out_off {out_off} is not a multiple of 4")
        if out_off < 0 or out_off + 3 * Hp * Wp > out_elems:
            raise ValueError(f"view table entry {v}: the block (elements {out_off} .. {out_off + 3 * Hp * Wp}) leaves out "
                             f"({out_elems} elements)")
        spans.append((out_off, out_off + 3 * Hp * Wp, v))
    spans.sort()
    for (_, end, a), (beg, _, b) in zip(spans, spans[1:]):
        if beg < end:
            raise ValueError(f"view table entries {a} and {b}: the blocks overlap")
    return table


def test_views(data, table, out, mean=None, std=None, bgr_to_rgb=False, pad_val=0.0, table_dev=None):
    """Every view of a test iteration in ONE launch (s2f_test_views): per table entry the keep-ratio bilinear resize of a uint8 BGR
    picture of `data` (aug_apply's resize: the kernels call one sampler), the horizontal flip, the channel swap, (x - mean) / std and
    the padding with pad_val, into the entry's [3, Hp, Wp] block of the packed fp32 buffer `out`; elements between the blocks are not
    touched.  table: a numpy array of VIEW_PARAM_DTYPE -- the host wrote it, so check_view_table validates EVERY entry here, before
    any launch (ValueError); table_dev: its staged copy in device memory as uint8 (None: copied here).  There is no other route: a
    CPU tensor raises."""
    _byte_buffer(data)
    if not (out.dtype == torch.float32 and out.dim() == 1 and out.is_contiguous()):
        raise ValueError("out: one contiguous fp32 buffer")
    table = check_view_table(table, data.numel(), out.numel())
    m, s = _mean_std(mean, std)
    _aug_cuda(data, out)
    V = len(table)
    if table_dev is None:
        table_dev = torch.from_numpy(_np.ascontiguousarray(table).view(_np.uint8).copy()).to(data.device)
    _staged_table(table_dev, VIEW_PARAM_BYTES, V)
    check(lib.s2f_test_views(_ptr(data), data.numel(), _ptr(table_dev), V, int(table["Hp"].max()), int(table["Wp"].max()), *m, *s,
                             int(bool(bgr_to_rgb)), float(pad_val), _ptr(out), out.numel(), _stream()), "s2f_test_views")
    return out


test_views.__test__ = False          # (an op, not a test: pytest collects `test_*` names imported into a test module)


# ------------------------------------------------------------------------------------------------ evaluation
SEG_HIST_MAX_CLASSES = 2048          # include/s2f.h S2F_SEG_HIST_MAX_CLASSES
_SEG_PRED_CODES = {torch.int64: 0, torch.float32: 1}
_SEG_LABEL_CODES = {torch.uint8: 0, torch.int64: 1}


def _seg_hist_torch(pred, label, totals, ignore_index, reduce_zero_label):
    """the semantics of s2f_seg_hist in exact integer torch arithmetic (CPU tensors; CUDA tensors the kernel does not take)"""
    K = totals.shape[1]
    lab = label.to(torch.int64)
    if reduce_zero_label:
        lab = torch.where((lab == 0) | (lab == 255), torch.full_like(lab, 255), lab - 1)
    none = torch.full_like(lab, -1)
    if pred.is_floating_point():
        ok = (pred >= 0) & (pred < K) & (pred == pred.trunc())
        pc = torch.where(ok, torch.where(ok, pred, torch.zeros_like(pred)).to(torch.int64), none)
    else:
        pred = pred.to(torch.int64)
        pc = torch.where((pred >= 0) & (pred < K), pred, none)
    lc = torch.where((lab >= 0) & (lab < K), lab, none)
    part = lab != ignore_index
    pc, lc = pc[part], lc[part]
    totals[0] += torch.bincount(pc[(pc == lc) & (pc >= 0)], minlength=K)
    totals[1] += torch.bincount(pc[pc >= 0], minlength=K)
    totals[2] += torch.bincount(lc[lc >= 0], minlength=K)
    return totals


def seg_hist(pred, label, totals, ignore_index=255, reduce_zero_label=False):
    """totals int64 [3, K] += {intersection, prediction areas, label areas} of ONE image over the pixels with label != ignore_index
    (s2f_seg_hist; IoUMetric.intersect_and_union, mmseg iou_metric.py:164-205, as integer class histograms).  pred [H, W] or [1, H, W],
    int64 or float32 0 / 1; label of the same shape -- or stored transposed ([W, H], iou_metric.py:187-190: read by strides, not
    copied) -- uint8 or int64; `reduce_zero_label` maps a raw annotation on the fly (0 -> 255, 255 -> 255, else - 1).  CUDA tensors
    run the kernel; CPU tensors the same arithmetic in torch (the package's CPU implementation of this op)."""
    pred = pred[0] if pred.dim() == 3 and pred.shape[0] == 1 else pred
    label = label[0] if label.dim() == 3 and label.shape[0] == 1 else label
    assert pred.dim() == 2 and label.dim() == 2, "one [H, W] (or [1, H, W]) prediction and label map"
    if label.shape[0] != pred.shape[0] and label.shape[0] == pred.shape[1]:
        label = label.t()
    assert label.shape == pred.shape, f"label {tuple(label.shape)} does not fit the prediction {tuple(pred.shape)}"
    assert totals.dtype == torch.int64 and totals.dim() == 2 and totals.shape[0] == 3 and totals.is_contiguous()
    assert pred.device == label.device == totals.device, "pred, label and totals on one device"
    H, W = pred.shape
    K = totals.shape[1]
    if not pred.is_cuda:
        return _seg_hist_torch(pred, label, totals, int(ignore_index), bool(reduce_zero_label))
    if (pred.dtype not in _SEG_PRED_CODES or label.dtype not in _SEG_LABEL_CODES or not 0 < K <= SEG_HIST_MAX_CLASSES
            or not 0 < H * W < 2 ** 31 - 8 or abs(int(ignore_index)) >= 2 ** 31):
        fallback("seg_hist", f"pred {pred.dtype}, label {label.dtype}, K {K}, {H} x {W}")
        return _seg_hist_torch(pred, label, totals, int(ignore_index), bool(reduce_zero_label))
    pred = pred.contiguous()
    check(lib.s2f_seg_hist(_ptr(pred), _SEG_PRED_CODES[pred.dtype], _ptr(label), _SEG_LABEL_CODES[label.dtype], label.stride(0),
                           label.stride(1), W, H * W, K, int(ignore_index), int(bool(reduce_zero_label)), _ptr(totals), _stream()),
          "s2f_seg_hist")
    return totals


SEG_CONF_LDS_BYTES = 131072          # include/s2f.h S2F_SEG_CONF_LDS_BYTES: [K][K] 32-bit counters per workgroup up to K = 181
_SEG_CONF_GLOBAL = 2                 # include/s2f.h S2F_SEG_CONF_GLOBAL


def _seg_confusion_torch(pred, label, matrix, ignore_index, reduce_zero_label):
    """the semantics of s2f_seg_confusion in exact integer torch arithmetic (CPU tensors; CUDA tensors the kernel does not take)"""
    K = matrix.shape[0]
    lab = label.to(torch.int64)
    if reduce_zero_label:
        lab = torch.where((lab == 0) | (lab == 255), torch.full_like(lab, 255), lab - 1)
    if pred.is_floating_point():
        ok = (pred >= 0) & (pred < K) & (pred == pred.trunc())
        pc = torch.where(ok, pred, torch.zeros_like(pred)).to(torch.int64)
    else:
        pc = pred.to(torch.int64)
        ok = (pc >= 0) & (pc < K)
    ok = ok & (lab != ignore_index) & (lab >= 0) & (lab < K)
    matrix += torch.bincount(lab[ok] * K + pc[ok], minlength=K * K).view(K, K)
    return matrix


def seg_confusion(pred, label, matrix, ignore_index=255, reduce_zero_label=False, route=None):
    """matrix int64 [K, K] += the class-pair counts of ONE image, row = label, column = prediction (s2f_seg_confusion; the reference's
    tools/analysis_tools/confusion_matrix.py:46-65 with IoUMetric's ignore_index rule, which that function lacks).  A pixel counts
    iff its (reduce_zero_label-mapped) label != ignore_index and is a class and its prediction is a class; pred / label shapes,
    dtypes and the transposed label as seg_hist.  route: None -- the kernel chooses between its per-workgroup LDS table and global
    atomics by K -- or "global" to force the latter (both give the same matrix).  CUDA tensors run the kernel; CPU tensors the same
    arithmetic in torch (the package's CPU implementation of this op)."""
    assert route in (None, "global"), f"route {route!r}: None or 'global'"
    pred = pred[0] if pred.dim() == 3 and pred.shape[0] == 1 else pred
    label = label[0] if label.dim() == 3 and label.shape[0] == 1 else label
    assert pred.dim() == 2 and label.dim() == 2, "one [H, W] (or [1, H, W]) prediction and label map"
    if label.shape[0] != pred.shape[0] and label.shape[0] == pred.shape[1]:
        label = label.t()
    assert label.shape == pred.shape, f"label {tuple(label.shape)} does not fit the prediction {tuple(pred.shape)}"
    assert (matrix.dtype == torch.int64 and matrix.dim() == 2 and matrix.shape[0] == matrix.shape[1] and matrix.is_contiguous()), \
        "matrix: one contiguous int64 [K, K]"
    assert pred.device == label.device == matrix.device, "pred, label and matrix on one device"
    H, W = pred.shape
    K = matrix.shape[0]
    if not pred.is_cuda:
        return _seg_confusion_torch(pred, label, matrix, int(ignore_index), bool(reduce_zero_label))
    if (pred.dtype not in _SEG_PRED_CODES or label.dtype not in _SEG_LABEL_CODES or not 0 < K <= SEG_HIST_MAX_CLASSES
            or not 0 < H * W < 2 ** 31 - 8 or abs(int(ignore_index)) >= 2 ** 31):
        fallback("seg_confusion", f"pred {pred.dtype}, label {label.dtype}, K {K}, {H} x {W}")
        return _seg_confusion_torch(pred, label, matrix, int(ignore_index), bool(reduce_zero_label))
    pred = pred.contiguous()
    flags = int(bool(reduce_zero_label)) | (_SEG_CONF_GLOBAL if route == "global" else 0)
    check(lib.s2f_seg_confusion(_ptr(pred), _SEG_PRED_CODES[pred.dtype], _ptr(label), _SEG_LABEL_CODES[label.dtype], label.stride(0),
                                label.stride(1), W, H * W, K, int(ignore_index), flags, _ptr(matrix), _stream()),
          "s2f_seg_confusion")
    return matrix


# ------------------------------------------------------------------------------------------------ operand census
CENSUS_FIELDS = 8                    # include/s2f.h S2F_CENSUS_FIELDS
_CENSUS_DTYPES = {torch.float32: 0, torch.bfloat16: 1}          # S2F_CENSUS_F32 / S2F_CENSUS_BF16


def _operand_census_torch(x, row, D):
    """the semantics of s2f_operand_census in exact integer torch arithmetic (CPU tensors)"""
    xf = x.reshape(-1).to(torch.float32)          # (bf16 -> fp32 is exact)
    n = xf.numel()
    mag = xf.view(torch.int32) & 0x7fffffff
    p = xf * torch.tensor(D, dtype=torch.float32)          # ONE fp32 multiply by D converted to fp32
    finite = mag < 0x7f800000
    subnormal = (mag != 0) & (mag < 0x00800000)
    on = finite & ~subnormal & (p >= 0) & (p <= 65535) & (p == p.trunc())
    level = torch.where(on, p, torch.zeros_like(p)).to(torch.int64)
    row[0] += n
    row[1] += level.sum()
    row[2] += (mag != 0).sum()
    row[3] += (~on).sum()
    if n:
        row[4] = torch.maximum(row[4], level.max())
    row[5] += (~finite).sum()
    row[6] += 1
    return row


def operand_census(x, row, D):
    """row int64 [8] += the census of one operand (s2f_operand_census, include/s2f.h "operand census"): {elements, sum of the integer
    levels x * D, non-zero elements, elements off the level grid, max level (a running maximum), non-finite elements, calls, 0}.
    x: a tensor or an ops.Spikes (then its stored data: bf16 or fp32), fp32 or bf16, any shape -- a non-contiguous one is copied; row:
    one row of the caller's table (a contiguous slice) on x's device; D: the level grid, an integer >= 1.  CUDA tensors run the kernel,
    one launch; CPU tensors the same arithmetic in torch (the package's CPU implementation of this op, no fall-back site)."""
    x = x.data if isinstance(x, Spikes) else x
    D = int(D)
    if x.dtype not in _CENSUS_DTYPES:
        raise TypeError(f"operand_census: an operand is fp32 or bf16; got {x.dtype}")
    if D < 1:
        raise ValueError(f"operand_census: D {D} below 1")
    if row.dtype != torch.int64 or tuple(row.shape) != (CENSUS_FIELDS,) or not row.is_contiguous():
        raise ValueError(f"operand_census: row is a contiguous int64 [{CENSUS_FIELDS}]")
    if row.device != x.device:
        raise RuntimeError(f"operand_census: the operand on {x.device}, the row on {row.device}")
    x = x.detach()
    if not x.is_cuda:
        return _operand_census_torch(x, row, D)
    x = x.contiguous()
    # (an empty tensor has no address; the entry point wants a non-null one and reads nothing of it at n == 0)
    check(lib.s2f_operand_census(_ptr(x) if x.numel() else _ptr(row), _CENSUS_DTYPES[x.dtype], x.numel(), D, _ptr(row), _stream()),
          "s2f_operand_census")
    return row


# ------------------------------------------------------------------------------------------------ visualisation
_SEG_DRAW_BGR = 4                    # include/s2f.h S2F_SEG_DRAW_BGR


def _seg_class_numpy(m, K, reduce_zero_label=False):
    """a label map as numpy -> int64 class indices, -1 where the value is no class (the rules of s2f_seg_hist / s2f_seg_draw)"""
    if m.dtype.kind == "f":
        with _np.errstate(invalid="ignore"):
            ok = (m >= 0) & (m < K) & (m == _np.trunc(m))
        return _np.where(ok, _np.where(ok, m, 0).astype(_np.int64), -1)
    m = m.astype(_np.int64)
    if reduce_zero_label:
        m = _np.where((m == 0) | (m == 255), 255, m - 1)
    return _np.where((m >= 0) & (m < K), m, -1)


def _seg_draw_numpy(image, palette, gt, pred, alpha, bgr, reduce_zero_label, out):
    """the semantics of s2f_seg_draw in numpy float64, one rounding per operation (CPU tensors)"""
    img, pal = image.numpy(), palette.numpy()
    K = pal.shape[0]
    kept = (img[..., ::-1] if bgr else img).astype(_np.float64) * (1.0 - alpha)
    W = img.shape[1]
    for q, (m, rzl) in enumerate((m, rzl) for m, rzl in ((gt, reduce_zero_label), (pred, False)) if m is not None):
        cls = _seg_class_numpy(m.numpy(), K, rzl)
        colour = _np.where((cls >= 0)[..., None], pal[_np.clip(cls, 0, K - 1)], 0).astype(_np.float64)
        out[:, q * W:(q + 1) * W] = torch.from_numpy((kept + colour * alpha).astype(_np.uint8))
    return out


def seg_draw(image, palette, gt=None, pred=None, alpha=0.8, bgr=False, reduce_zero_label=False, out=None):
    """-> uint8 [H, P W, 3] RGB: the class colours of the P given maps blended into `image`, the ground truth left of the prediction
    (s2f_seg_draw; SegLocalVisualizer._draw_sem_seg and add_datasample's concatenation, mmseg local_visualizer.py:79-118, as one
    launch).  image uint8 [H, W, 3], RGB or (`bgr`) BGR; palette uint8 [K, 3] RGB on the image's device; gt [H, W] or [1, H, W], uint8
    or int64, `reduce_zero_label` maps it as a raw annotation first; pred alike, int64 or float32.  Every byte is
    uint8(fl64(v * (1 - alpha)) + fl64(c * alpha)), c the palette entry of the pixel's class or 0 where its value is no class (a
    negative label, too: a stated deviation).  CUDA tensors run the kernel; CPU tensors the same arithmetic in numpy (the package's
    CPU implementation of this op).  A tensor on another device than the image raises; a non-contiguous one is copied."""
    maps = []
    for m, what, dtypes in ((gt, "gt", _SEG_LABEL_CODES), (pred, "pred", _SEG_PRED_CODES)):
        if m is not None:
            m = m[0] if m.dim() == 3 and m.shape[0] == 1 else m
            if m.dtype not in dtypes:
                raise TypeError(f"seg_draw: {what} is {m.dtype}, not one of {[str(d) for d in dtypes]}")
            if m.dim() != 2 or tuple(m.shape) != tuple(image.shape[:2]):
                raise ValueError(f"seg_draw: {what} {tuple(m.shape)} does not fit the picture {tuple(image.shape)}")
            m = m.contiguous()
        maps.append(m)
    gt, pred = maps
    if gt is None and pred is None:
        raise ValueError("seg_draw: neither a ground-truth map nor a prediction to draw")
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3 or image.numel() == 0:
        raise ValueError("seg_draw: image is uint8 [H, W, 3]")
    if palette.dtype != torch.uint8 or palette.dim() != 2 or palette.shape[1] != 3:
        raise ValueError("seg_draw: palette is uint8 [K, 3]")
    H, W, K, P = image.shape[0], image.shape[1], palette.shape[0], sum(m is not None for m in maps)
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"seg_draw: alpha {alpha} outside 0 .. 1")
    if not 0 < K <= SEG_HIST_MAX_CLASSES or not H * W < 2 ** 31 - 8:
        raise ValueError(f"seg_draw: {K} classes (1 .. {SEG_HIST_MAX_CLASSES}) on {H} x {W} pixels (fewer than 2^31 - 8)")
    if out is None:
        out = torch.empty(H, P * W, 3, dtype=torch.uint8, device=image.device)
    if out.dtype != torch.uint8 or tuple(out.shape) != (H, P * W, 3) or not out.is_contiguous():
        raise ValueError(f"seg_draw: out is one contiguous uint8 [{H}, {P * W}, 3]")
    for t in (palette, gt, pred, out):
        if t is not None and t.device != image.device:
            raise RuntimeError(f"seg_draw: a tensor on {t.device}, the image on {image.device}")
    image, palette = image.contiguous(), palette.contiguous()
    if not image.is_cuda:
        return _seg_draw_numpy(image, palette, gt, pred, alpha, bool(bgr), bool(reduce_zero_label), out)
    flags = (_SEG_DRAW_BGR if bgr else 0) | int(bool(reduce_zero_label))
    check(lib.s2f_seg_draw(_ptr(image), _ptr(gt), _SEG_LABEL_CODES[gt.dtype] if gt is not None else 0, _ptr(pred),
                           _SEG_PRED_CODES[pred.dtype] if pred is not None else 0, _ptr(palette), K, alpha, flags, H, W, _ptr(out),
                           _stream()), "s2f_seg_draw")
    return out


# ------------------------------------------------------------------------------------------------ mask losses (row f1)
class _MaskLossSums(torch.autograd.Function):
    """sums[p] = {sum s t, sum s, sum t, sum focal} over the 2x up-sampled logits of matched prediction p against its binary
    target (s2f.h s2f_mask_loss_fwd/bwd); nothing of size [P, 2h, 2w] exists forward, one such buffer backward."""

    @staticmethod
    def forward(ctx, pred, tgt, gt_index, alpha, gamma):
        _need_cuda(pred)
        pred = pred.contiguous()
        tgt = tgt.contiguous()
        P, h, w = pred.shape
        assert tgt.dtype == torch.uint8 and tgt.shape[1:] == (2 * h, 2 * w) and gt_index.dtype == torch.int64
        sums = torch.empty(P, 4, dtype=torch.float32, device=pred.device)
        check(lib.s2f_mask_loss_fwd(_ptr(pred), _ptr(tgt), _ptr(gt_index), _ptr(sums), P, h, w, alpha, gamma, _stream()),
              "s2f_mask_loss_fwd")
        ctx.save_for_backward(pred, tgt, gt_index)
        ctx.cfg = (alpha, gamma)
        return sums

    @staticmethod
    def backward(ctx, g):
        pred, tgt, gt_index = ctx.saved_tensors
        P, h, w = pred.shape
        g = g.contiguous()
        gup = torch.empty(P, 2 * h, 2 * w, dtype=torch.float32, device=pred.device)
        check(lib.s2f_mask_loss_bwd(_ptr(pred), _ptr(tgt), _ptr(gt_index), _ptr(g), _ptr(gup), P, h, w, *ctx.cfg, _stream()),
              "s2f_mask_loss_bwd")
        gp = torch.empty_like(pred)
        check(lib.s2f_upsample2x_bwd(_ptr(gup), _ptr(gp), P, h, w, _stream()), "s2f_upsample2x_bwd")
        return gp, None, None, None, None


def mask_loss_sums(pred, tgt_u8, gt_index, alpha, gamma):
    """pred [P, h, w] fp32 logits, tgt_u8 [G, 2h, 2w] uint8 0/1, gt_index [P] int64 -> [P, 4]"""
    return _MaskLossSums.apply(pred, tgt_u8, gt_index, float(alpha), float(gamma))


def mask_cost_bins(pred, seg_small, K, alpha, gamma, eps):
    """pred [B, R, hw] fp32 logits, seg_small [B, hw] uint8 label map -> [B, R, 2K + 2]: per class id the segmented sums of
    (pos - neg) and of s, then sum neg and sum s over all pixels (s2f.h s2f_mask_cost_bins; match_cost.py:289-297, :361-371)."""
    _need_cuda(pred)
    pred, seg_small = pred.contiguous(), seg_small.contiguous()
    B, R, hw = pred.shape
    assert seg_small.dtype == torch.uint8 and seg_small.shape == (B, hw) and pred.dtype == torch.float32
    out = torch.empty(B, R, 2 * K + 2, dtype=torch.float32, device=pred.device)
    check(lib.s2f_mask_cost_bins(_ptr(pred), _ptr(seg_small), _ptr(out), B, R, hw, K, alpha, gamma, eps, _stream()),
          "s2f_mask_cost_bins")
    return out


LSA_MAX_QUERIES, LSA_MAX_CLASSES = 256, 254          # include/s2f.h S2F_LSA_MAX_QUERIES / S2F_LSA_MAX_CLASSES


def lsa_tables(cost, count_full, K, out=None, tile_l2=False):
    """The Hungarian assignment of the semantic-map loss on the device (s2f.h s2f_lsa_tables): cost [L, B, Q, K] fp32 and
    count_full [B, 256] fp32 as MaskFormerLoss.costs_all_classes returns them -> (tgt_labels [L, B, Q] int64, row_class [B, L*Q]
    int32, num_masks [L] fp32, status [1] int32) -- the three tables of MaskFormerLoss.match_tables plus a status word (bit 0: a
    label in K..254 is present, bit 1: a non-finite cost in a present column; num_masks is NaN then).  `out`: those four tensors
    to write into (static buffers of a captured step); every element is written.  No autograd; nothing synchronises.
    `tile_l2` (measurement only, tools/probe_lsa.py): re-read the costs from L2 instead of keeping the fp64 tile in LDS."""
    if not (cost.is_cuda and count_full.is_cuda):
        raise RuntimeError("ops.lsa_tables runs on the GPU only (HIP kernel, no host fall-back); got a CPU tensor -- "
                           "the host route is MaskFormerLoss.match_tables (assign='host')")
    if cost.dtype != torch.float32 or count_full.dtype != torch.float32:
        raise RuntimeError(f"ops.lsa_tables takes fp32 costs and counts; got {cost.dtype}, {count_full.dtype}")
    if cost.dim() != 4 or cost.shape[3] != K:
        raise ValueError(f"cost [L, B, Q, K = {K}], got {tuple(cost.shape)}")
    L, B, Q = cost.shape[:3]
    if tuple(count_full.shape) != (B, 256) or count_full.device != cost.device:
        raise ValueError(f"count_full [B = {B}, 256] on {cost.device}, got {tuple(count_full.shape)} on {count_full.device}")
    cost, count_full = cost.detach().contiguous(), count_full.detach().contiguous()
    dev = cost.device
    if out is None:
        out = (torch.empty(L, B, Q, dtype=torch.int64, device=dev), torch.empty(B, L * Q, dtype=torch.int32, device=dev),
               torch.empty(L, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    tgt, rows, num_masks, status = out
    for t, shape, dtype in ((tgt, (L, B, Q), torch.int64), (rows, (B, L * Q), torch.int32), (num_masks, (L,), torch.float32),
                            (status, (1,), torch.int32)):
        if not (t.device == dev and tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()):
            raise ValueError(f"out: a contiguous {dtype} tensor of shape {shape} on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    args = (_ptr(cost), _ptr(count_full), _ptr(tgt), _ptr(rows), _ptr(num_masks), _ptr(status), L, B, Q, int(K))
    if tile_l2:
        check(lib.s2f_lsa_tables_ex(*args, 1, _stream()), "s2f_lsa_tables_ex")          # S2F_LSA_TILE_L2
    else:
        check(lib.s2f_lsa_tables(*args, _stream()), "s2f_lsa_tables")
    return tgt, rows, num_masks, status


class _MaskLossSeg(torch.autograd.Function):
    """sums[(b, r)] = {sum s t, sum s, sum t, sum focal} of the 2x up-sampled logits pred[b, r] against  seg[b] == row_class[b, r]
    (rows with row_class < 0: zeros, zero gradient); s2f.h s2f_mask_loss_seg_fwd/bwd."""

    @staticmethod
    def forward(ctx, pred, seg, row_class, alpha, gamma):
        _need_cuda(pred)
        pred = pred.contiguous()
        B, R, h, w = pred.shape
        assert seg.dtype == torch.uint8 and seg.shape == (B, 2 * h, 2 * w) and seg.is_contiguous()
        assert row_class.dtype == torch.int32 and row_class.numel() == B * R and row_class.is_contiguous()
        sums = torch.empty(B * R, 4, dtype=torch.float32, device=pred.device)
        part = torch.empty(int(lib.s2f_mask_loss_seg_partials(B, R, h, w)), dtype=torch.float32, device=pred.device)
        check(lib.s2f_mask_loss_seg_fwd(_ptr(pred), _ptr(seg), _ptr(row_class), _ptr(sums), _ptr(part), B, R, h, w, alpha, gamma,
                                        _stream()), "s2f_mask_loss_seg_fwd")
        ctx.save_for_backward(pred, seg, row_class)
        ctx.cfg = (alpha, gamma)
        return sums

    @staticmethod
    def backward(ctx, g):
        pred, seg, row_class = ctx.saved_tensors
        B, R, h, w = pred.shape
        gp = torch.empty_like(pred)
        check(lib.s2f_mask_loss_seg_bwd(_ptr(pred), _ptr(seg), _ptr(row_class), _ptr(g.contiguous()), _ptr(gp), B, R, h, w, *ctx.cfg,
                                        _stream()), "s2f_mask_loss_seg_bwd")
        return gp, None, None, None, None


def mask_loss_seg(pred, seg_u8, row_class, alpha, gamma):
    """pred [B, R, h, w] fp32 logits, seg_u8 [B, 2h, 2w] uint8 label map, row_class [B * R] int32 -> sums [B * R, 4]"""
    return _MaskLossSeg.apply(pred, seg_u8, row_class, float(alpha), float(gamma))



__all__ = [n for n in dir() if not n.startswith('__')]
