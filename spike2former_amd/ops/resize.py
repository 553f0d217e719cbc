"""Differentiable bilinear resizing: the exact-2x kernels (csrc/upsample.hip) and the general one with its gather adjoint (csrc/resize.hip)."""
import math

import torch

from .config import cfg
from .core import *          # noqa: F401,F403  (the shared plumbing: _ptr, _stream, check, lib, Spikes, ...)

RESIZE_ALIGN_CORNERS, RESIZE_SIGMOID, RESIZE_FLIP_H, RESIZE_FLIP_V = 1, 2, 4, 8       # include/s2f.h S2F_RESIZE_*


def lib_flags(align_corners=False, sigmoid=False, flip=None):
    """the S2F_RESIZE_* flags word; flip: None | 'horizontal' | 'vertical'"""
    return ((RESIZE_ALIGN_CORNERS if align_corners else 0) | (RESIZE_SIGMOID if sigmoid else 0)
            | (RESIZE_FLIP_H if flip == "horizontal" else 0) | (RESIZE_FLIP_V if flip == "vertical" else 0))


def _resize_fwd(x, lead, window, size, flags):
    """-> y [*lead, H, W] fp32: per plane of the plane-contiguous map x its window = (plane stride, row stride, row0, col0, h, w),
    resized to size = (H, W) as `flags` say -- the one launch site of s2f_resize_fwd, which reads the window in place"""
    y = torch.empty(*lead, *size, dtype=torch.float32, device=x.device)
    check(lib.s2f_resize_fwd(_ptr(x), _ptr(y), math.prod(lead), *window, *size, flags, _stream()), "s2f_resize_fwd")
    return y


# ------------------------------------------------------------------------------------------------ 2x bilinear up-sampling
def _up2x_fwd(x, sigmoid=False):
    N, C, h, w = x.shape
    y = torch.empty(N, C, 2 * h, 2 * w, dtype=torch.float32, device=x.device)
    name = "s2f_upsample2x_sigmoid_fwd" if sigmoid else "s2f_upsample2x_fwd"          # (one signature)
    check(getattr(lib, name)(_ptr(x), _ptr(y), N * C, h, w, _stream()), name)
    return y


def _up2x_bwd_add(gy, gskip, gx):
    N, C, h, w = gx.shape
    check(lib.s2f_upsample2x_bwd_add(_ptr(gy), _ptr(gskip), _ptr(gx), N * C, h, w, _stream()), "s2f_upsample2x_bwd_add")


_Up2x = _pass_through_function(
    "_Up2x",
    """-> (up-sampled map, pass-through of x or an empty stand-in): the pass-through serves a second reader of x; the gradient it
    sends back is summed inside the adjoint kernel (s2f_upsample2x_bwd_add) instead of by an add of the autograd engine.""",
    _up2x_fwd, _up2x_bwd_add)


def _general_fwd(x, size, flags):
    N, C, h, w = x.shape          # (contiguous: the window is every whole plane)
    return _resize_fwd(x, (N, C), (h * w, w, 0, 0, h, w), size, flags)


def _general_bwd_add(gy, gskip, gx, size, flags):
    N, C, h, w = gx.shape
    check(lib.s2f_resize_bwd_add(_ptr(gy), _ptr(gskip), _ptr(gx), N * C, h, w, *size, flags, _stream()), "s2f_resize_bwd_add")


_Resize = _pass_through_function(
    "_Resize",
    """F.interpolate(x, size, mode='bilinear') for any sizes on s2f_resize_fwd; backward: the gather adjoint s2f_resize_bwd_add
    (no atomics: bit-repeatable).  -> (y, pass-through of x or an empty stand-in), the pass-through as in _Up2x: the gradient of a
    second reader of x is summed inside the adjoint kernel.""",
    _general_fwd, _general_bwd_add)


def _general_ok(x):
    return cfg.GENERAL_RESIZE and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.numel() > 0


def resize_bilinear(x, size, align_corners=False, sigmoid=False, skip=False):
    """F.interpolate(x [N, C, h, w], size, mode='bilinear', align_corners) (.sigmoid() after it with `sigmoid`) on the general
    kernel s2f_resize_fwd, any sizes; differentiable (s2f_resize_bwd_add) unless `sigmoid`, which is for inference only.
    `skip`: -> (y, x') as upsample_bilinear's."""
    H, W = (int(v) for v in size)
    size = (H, W)
    if sigmoid:
        assert not skip and not (torch.is_grad_enabled() and x.requires_grad), "the fused sigmoid has no adjoint"
        _need_cuda(x)
        return _general_fwd(x.contiguous(), size, lib_flags(align_corners, True))
    port = bool(skip and cfg.FANOUT_PORTS)
    y, through = _Resize.apply(x, port, size, lib_flags(align_corners))
    return (y, through if port else x) if skip else y


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
            return _up2x_fwd(x.contiguous(), sigmoid=True)
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


__all__ = [n for n in dir() if not n.startswith('__')]
