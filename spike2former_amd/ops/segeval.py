"""The evaluation ops: class and class-pair histograms (csrc/segmetric.hip), the drawing of label maps (csrc/segdraw.hip), each with
its CPU implementation."""
import numpy as _np
import torch

from .core import *          # noqa: F401,F403  (the shared plumbing: _ptr, _stream, check, lib, Spikes, ...)

SEG_HIST_MAX_CLASSES = 2048          # include/s2f.h S2F_SEG_HIST_MAX_CLASSES
SEG_CONF_LDS_BYTES = 131072          # include/s2f.h S2F_SEG_CONF_LDS_BYTES: [K][K] 32-bit counters per workgroup up to K = 181
_SEG_CONF_GLOBAL = 2                 # include/s2f.h S2F_SEG_CONF_GLOBAL
_SEG_DRAW_BGR = 4                    # include/s2f.h S2F_SEG_DRAW_BGR
_SEG_PRED_CODES = {torch.int64: 0, torch.float32: 1}
_SEG_LABEL_CODES = {torch.uint8: 0, torch.int64: 1}


def _seg_squeeze(m):
    """one map, [H, W] or [1, H, W] -> [H, W]"""
    return m[0] if m.dim() == 3 and m.shape[0] == 1 else m


def _seg_size_ok(K, H, W):
    """what the kernels take: K classes in the table, 32-bit pixel indices with room for the last 8-pixel group"""
    return 0 < K <= SEG_HIST_MAX_CLASSES and 0 < H * W < 2 ** 31 - 8


def _seg_maps(site, pred, label, K, acc, what, ignore_index):
    """The prediction / label map contract of the histogram op `site`, whose int64 accumulator `acc` (named `what`) holds K classes:
    -> (pred [H, W], label [H, W] -- one stored transposed ([W, H]) as the view that reads it by strides --, args).  args: the leading
    arguments of the entry point (pred, dtype code, label, dtype code, its two strides, W, H W, K, ignore_index), pred then contiguous,
    or None where the kernel does not take the maps: CPU tensors, or other dtypes and sizes than its own (the fall-back site)."""
    pred, label = _seg_squeeze(pred), _seg_squeeze(label)
    assert pred.dim() == 2 and label.dim() == 2, "one [H, W] (or [1, H, W]) prediction and label map"
    if label.shape[0] != pred.shape[0] and label.shape[0] == pred.shape[1]:
        label = label.t()
    assert label.shape == pred.shape, f"label {tuple(label.shape)} does not fit the prediction {tuple(pred.shape)}"
    assert pred.device == label.device == acc.device, f"pred, label and {what} on one device"
    H, W = pred.shape
    if not pred.is_cuda:
        return pred, label, None
    if not (pred.dtype in _SEG_PRED_CODES and label.dtype in _SEG_LABEL_CODES and _seg_size_ok(K, H, W)
            and abs(int(ignore_index)) < 2 ** 31):
        fallback(site, f"pred {pred.dtype}, label {label.dtype}, K {K}, {H} x {W}")
        return pred, label, None
    pred = pred.contiguous()
    return pred, label, (_ptr(pred), _SEG_PRED_CODES[pred.dtype], _ptr(label), _SEG_LABEL_CODES[label.dtype], label.stride(0),
                         label.stride(1), W, H * W, K, int(ignore_index))


def _seg_class(v, K, reduce_zero_label=False):
    """A prediction or label map -> (cls, v'): v' the values the ignore_index test reads -- an integer map as int64 after
    `reduce_zero_label` (0 -> 255, 255 -> 255, else - 1), a float map as it is -- and cls their int64 class indices, -1 where the
    value is no class: an integer outside [0, K), a float that differs from its truncation or lies outside [0, K).  The kernels' rule
    (s2f_seg_hist, s2f_seg_confusion, s2f_seg_draw), stated once for the CPU implementations, in exact integer torch arithmetic."""
    none = torch.full_like(v, -1, dtype=torch.int64)
    if v.is_floating_point():
        ok = (v >= 0) & (v < K) & (v == v.trunc())
        return torch.where(ok, torch.where(ok, v, torch.zeros_like(v)).to(torch.int64), none), v
    v = v.to(torch.int64)
    if reduce_zero_label:
        v = torch.where((v == 0) | (v == 255), torch.full_like(v, 255), v - 1)
    return torch.where((v >= 0) & (v < K), v, none), v


# ------------------------------------------------------------------------------------------------ evaluation
def _seg_hist_torch(pred, label, totals, ignore_index, reduce_zero_label):
    """the semantics of s2f_seg_hist in exact integer torch arithmetic (CPU tensors; CUDA tensors the kernel does not take)"""
    K = totals.shape[1]
    pc, _ = _seg_class(pred, K)
    lc, lab = _seg_class(label.to(torch.int64), K, reduce_zero_label)
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
    assert totals.dtype == torch.int64 and totals.dim() == 2 and totals.shape[0] == 3 and totals.is_contiguous()
    pred, label, args = _seg_maps("seg_hist", pred, label, totals.shape[1], totals, "totals", ignore_index)
    if args is None:
        return _seg_hist_torch(pred, label, totals, int(ignore_index), bool(reduce_zero_label))
    check(lib.s2f_seg_hist(*args, int(bool(reduce_zero_label)), _ptr(totals), _stream()), "s2f_seg_hist")
    return totals


def _seg_confusion_torch(pred, label, matrix, ignore_index, reduce_zero_label):
    """the semantics of s2f_seg_confusion in exact integer torch arithmetic (CPU tensors; CUDA tensors the kernel does not take)"""
    K = matrix.shape[0]
    pc, _ = _seg_class(pred, K)
    lc, lab = _seg_class(label.to(torch.int64), K, reduce_zero_label)
    ok = (pc >= 0) & (lab != ignore_index) & (lc >= 0)
    matrix += torch.bincount(lc[ok] * K + pc[ok], minlength=K * K).view(K, K)
    return matrix


def seg_confusion(pred, label, matrix, ignore_index=255, reduce_zero_label=False, route=None):
    """matrix int64 [K, K] += the class-pair counts of ONE image, row = label, column = prediction (s2f_seg_confusion; the reference's
    tools/analysis_tools/confusion_matrix.py:46-65 with IoUMetric's ignore_index rule, which that function lacks).  A pixel counts
    iff its (reduce_zero_label-mapped) label != ignore_index and is a class and its prediction is a class; pred / label shapes,
    dtypes and the transposed label as seg_hist.  route: None -- the kernel chooses between its per-workgroup LDS table and global
    atomics by K -- or "global" to force the latter (both give the same matrix).  CUDA tensors run the kernel; CPU tensors the same
    arithmetic in torch (the package's CPU implementation of this op)."""
    assert route in (None, "global"), f"route {route!r}: None or 'global'"
    assert (matrix.dtype == torch.int64 and matrix.dim() == 2 and matrix.shape[0] == matrix.shape[1] and matrix.is_contiguous()), \
        "matrix: one contiguous int64 [K, K]"
    pred, label, args = _seg_maps("seg_confusion", pred, label, matrix.shape[0], matrix, "matrix", ignore_index)
    if args is None:
        return _seg_confusion_torch(pred, label, matrix, int(ignore_index), bool(reduce_zero_label))
    flags = int(bool(reduce_zero_label)) | (_SEG_CONF_GLOBAL if route == "global" else 0)
    check(lib.s2f_seg_confusion(*args, flags, _ptr(matrix), _stream()), "s2f_seg_confusion")
    return matrix


# ------------------------------------------------------------------------------------------------ visualisation
def _seg_draw_numpy(image, palette, gt, pred, alpha, bgr, reduce_zero_label, out):
    """the semantics of s2f_seg_draw in numpy float64, one rounding per operation (CPU tensors)"""
    img, pal = image.numpy(), palette.numpy()
    K = pal.shape[0]
    kept = (img[..., ::-1] if bgr else img).astype(_np.float64) * (1.0 - alpha)
    W = img.shape[1]
    for q, (m, rzl) in enumerate((m, rzl) for m, rzl in ((gt, reduce_zero_label), (pred, False)) if m is not None):
        cls = _seg_class(m, K, rzl)[0].numpy()
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
            m = _seg_squeeze(m)
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
    if not _seg_size_ok(K, H, W):
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


__all__ = [n for n in dir() if not n.startswith('__')]
