"""Inference post-processing on csrc/resize.hip (window resize, arg-max, label maps, test-time augmentation) and sliding-window
inference on csrc/slide.hip."""
import torch

from .core import *          # noqa: F401,F403  (the shared plumbing: _ptr, _stream, check, lib, Spikes, ...)
from .resize import _resize_fwd, lib_flags


def _window(x, crop):
    """x [K, Hp, Wp] fp32 CUDA and crop = (top, bottom, left, right) -> (x as a plane-contiguous map, its window as the entry points
    take it: plane stride, row stride, row0, col0, h, w)"""
    _need_cuda(x)
    x = x.contiguous()
    Hp, Wp = x.shape[-2:]
    top, bottom, left, right = (int(v) for v in (crop or (0, 0, 0, 0)))
    assert x.stride(-1) == 1 and x.stride(-2) == Wp and x.stride(0) == Hp * Wp, "a contiguous [K, H, W] map"
    return x, (Hp * Wp, Wp, top, left, Hp - top - bottom, Wp - left - right)


def _label_out(K, H, W, device, float_out=True):
    """-> (out, ptrs): the label map [1, H, W] an entry point writes -- int64 class indices, or float 0 / 1 for K == 1 with float_out --
    and its address as the entry points' (int64 output, float output) argument pair, the other one null"""
    f = float_out and K == 1
    out = torch.empty(1, H, W, dtype=torch.float32 if f else torch.int64, device=device)
    return out, ((None, _ptr(out)) if f else (_ptr(out), None))


def resize_window(x, size, crop=None, flip=None, align_corners=False, sigmoid=False):
    """x [K, Hp, Wp] fp32 CUDA -> [K, H, W]: the window x[:, top:Hp-bottom, left:Wp-right] (crop = (top, bottom, left, right)),
    flipped (None | 'horizontal' | 'vertical'), bilinearly resized to `size` (then sigmoid) -- one s2f_resize_fwd pass, no copy of
    the window (EncoderDecoder.postprocess_result)."""
    x, window = _window(x, crop)
    H, W = (int(v) for v in size)
    return _resize_fwd(x, x.shape[:1], window, (H, W), lib_flags(align_corners, sigmoid, flip))


def seg_argmax(x, threshold=0.3, sigmoid=False, float_out=False):
    """x [K, H, W] fp32 CUDA -> [1, H, W]: K > 1 the int64 arg-max over K (torch.argmax: first maximum, NaN wins); K == 1
    (sigmoid(x) if `sigmoid` else x) > threshold as int64 or, with float_out, as float 0 / 1 (s2f_seg_argmax)."""
    _need_cuda(x)
    x = x.contiguous()
    K, H, W = x.shape
    out, ptrs = _label_out(K, H, W, x.device, float_out)
    check(lib.s2f_seg_argmax(_ptr(x), *ptrs, K, H * W, int(sigmoid), float(threshold), _stream()), "s2f_seg_argmax")
    return out


def seg_label(x, size, crop=None, flip=None, align_corners=False, threshold=0.3):
    """x [K, Hp, Wp] fp32 CUDA -> the label map [1, H, W] of its window resized to `size`: int64 arg-max for K > 1, float 0 / 1
    (sigmoid > threshold) for K == 1 -- the bits of seg_argmax(resize_window(x, size, crop, flip, align_corners, sigmoid=K == 1),
    threshold, float_out=True) in ONE launch with no [K, H, W] intermediate (s2f_seg_label)."""
    x, window = _window(x, crop)
    K = x.shape[0]
    H, W = (int(v) for v in size)
    out, ptrs = _label_out(K, H, W, x.device)
    check(lib.s2f_seg_label(_ptr(x), *ptrs, K, *window, H, W, lib_flags(align_corners, False, flip), float(threshold), _stream()),
          "s2f_seg_label")
    return out


def tta_accumulate(acc, x, first, crop=None, flip=None, align_corners=False, pre_sigmoid=False):
    """acc [K, H, W] (first ? = : +=) softmax over K of x's window (crop / flip / resize as resize_window) -- K == 1: sigmoid,
    after a first one with pre_sigmoid (s2f_tta_accumulate; mmseg seg_tta.py:29-34)"""
    x, window = _window(x, crop)
    _need_cuda(acc)
    assert acc.is_contiguous() and acc.dtype == torch.float32 and acc.shape[0] == x.shape[0]
    K, H, W = acc.shape
    check(lib.s2f_tta_accumulate(_ptr(x), _ptr(acc), K, *window, H, W, lib_flags(align_corners, pre_sigmoid, flip),
                                 int(bool(first)), _stream()), "s2f_tta_accumulate")
    return acc


def tta_finish(acc, n_views, threshold=0.3):
    """acc [K, H, W] /= n_views in place; -> the int64 arg-max [1, H, W] (K > 1) or the float 0 / 1 map acc > threshold (K == 1),
    as seg_tta.py:35-40 (s2f_tta_finish)"""
    _need_cuda(acc)
    assert acc.is_contiguous() and acc.dtype == torch.float32
    K, H, W = acc.shape
    out, ptrs = _label_out(K, H, W, acc.device)
    check(lib.s2f_tta_finish(_ptr(acc), *ptrs, K, H * W, int(n_views), float(threshold), _stream()), "s2f_tta_finish")
    return out


# ------------------------------------------------------------------------------------------------ sliding-window inference
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


__all__ = [n for n in dir() if not n.startswith('__')]
