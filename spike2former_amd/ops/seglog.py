"""The segmentation log's row (csrc/seglog.hip): `seg_log_append`, the areas of intersect_and_union between the step's own
prediction at the mask resolution and the sub-sampled label map, per class and scored decoder layer, into a ring on the device.  HIP
only -- the score is a kernel of the captured step; CPU tensors raise (the numpy restatement is tests/seglog_ref.py)."""
import ctypes

import torch

from .core import _ptr, _stream, check, lib

SEG_LOG_MAX_LAYERS = 32          # include/s2f.h S2F_SEG_LOG_MAX_LAYERS
SEG_LOG_MAX_CLASSES = 254          # 255 is the ignored label


def seg_log_tiles(h, w):
    """the workgroups of s2f_seg_log_partials per (scored layer, image) of an h x w mask map: `partials` holds L' * B * tiles slices"""
    tile = int(lib.s2f_seg_log_tile_pixels())
    return (int(h) * int(w) + tile - 1) // tile


def seg_log_append(pred, cls, seg_u8, layers, partials, ring, streak, head, patience):
    """One row of train-crop areas (s2f_seg_log_partials -> s2f_seg_log_rows).  pred fp32 [B, L*Q, h*w]: the head's own mask buffer
    (logits); cls fp32 [L, B, Q, K+1]: the class scores (logits, the void column last); seg_u8 uint8 [B, 2h, 2w] with 255 = ignored,
    read with stride 2; layers: the scored decoder layers, a sequence of L' ints in 0 .. L-1 (host values: checked before the launch
    and baked into it); partials int32 [L' * B * seg_log_tiles(h, w), 3, K] (workspace); ring int64 [window, L', 3, K]; streak int32
    [K]; head int64 [4], the head of devring.py.  Row head[0] % window <- per scored layer {intersect, pred, label}[K], the areas of
    IoUMetric.intersect_and_union between pred = argmax_k sum_q softmax(cls)[q, k] * sigmoid(pred)[q, p] and seg_u8[:, ::2, ::2] over the
    batch (include/s2f.h "segmentation log"); the streaks count the rows in a row in which a class was labelled and not once hit by the
    LAST scored layer, the first to reach `patience` is latched in head[1]; head[0] += 1.  Two launches on the current stream, no
    synchronisation, capturable; pred, cls and seg_u8 are only read.  HIP only: CPU tensors raise."""
    if pred.dtype != torch.float32 or pred.dim() != 3 or not pred.is_contiguous():
        raise ValueError("seg_log_append: pred is a contiguous fp32 [B, L*Q, h*w]")
    if cls.dtype != torch.float32 or cls.dim() != 4 or not cls.is_contiguous():
        raise ValueError("seg_log_append: cls is a contiguous fp32 [L, B, Q, K+1]")
    L, B, Q, K = cls.shape[0], cls.shape[1], cls.shape[2], cls.shape[3] - 1
    if seg_u8.dtype != torch.uint8 or seg_u8.dim() != 3 or seg_u8.shape[0] != B or not seg_u8.is_contiguous():
        raise ValueError(f"seg_log_append: seg_u8 is a contiguous uint8 [{B}, 2h, 2w]")
    H, W = seg_u8.shape[1:]
    h, w = H // 2, W // 2
    if H % 2 or W % 2 or tuple(pred.shape) != (B, L * Q, h * w):
        raise ValueError(f"seg_log_append: pred {tuple(pred.shape)} is not [{B}, {L} * {Q}, h*w] at half the {H} x {W} label maps")
    if not 1 <= K <= SEG_LOG_MAX_CLASSES or w % 2 or (h * w) % 4:
        raise ValueError(f"seg_log_append: {K} classes (1 .. {SEG_LOG_MAX_CLASSES}) on a {h} x {w} mask map (w even, h*w a multiple of 4)")
    layers = [int(i) for i in layers]
    n = len(layers)
    if not 1 <= n <= SEG_LOG_MAX_LAYERS or any(not 0 <= i < L for i in layers):
        raise ValueError(f"seg_log_append: layers {layers}: 1 .. {SEG_LOG_MAX_LAYERS} of them, each in 0 .. {L - 1}")
    per_layer = B * seg_log_tiles(h, w)
    if partials.dtype != torch.int32 or tuple(partials.shape) != (n * per_layer, 3, K) or not partials.is_contiguous():
        raise ValueError(f"seg_log_append: partials is a contiguous int32 [{n * per_layer}, 3, {K}]")
    if ring.dtype != torch.int64 or ring.dim() != 4 or tuple(ring.shape[1:]) != (n, 3, K) or not ring.is_contiguous():
        raise ValueError(f"seg_log_append: ring is a contiguous int64 [window, {n}, 3, {K}]")
    if streak.dtype != torch.int32 or tuple(streak.shape) != (K,) or not streak.is_contiguous():
        raise ValueError(f"seg_log_append: streak is a contiguous int32 [{K}]")
    if head.dtype != torch.int64 or tuple(head.shape) != (4,) or not head.is_contiguous():
        raise ValueError("seg_log_append: head is a contiguous int64 [4]")
    if any(t.device != pred.device for t in (cls, seg_u8, partials, ring, streak, head)):
        raise RuntimeError("seg_log_append: every tensor lives on one device")
    window, patience = ring.shape[0], int(patience)
    if window < 1 or patience < 1:
        raise ValueError(f"seg_log_append: a ring of {window} rows, patience {patience}: each is at least 1")
    if not pred.is_cuda:
        raise RuntimeError("seg_log_append: the segmentation log is two HIP launches of the captured step; there is no CPU route")
    s = _stream()
    table = (ctypes.c_int32 * n)(*layers)
    check(lib.s2f_seg_log_partials(_ptr(pred), _ptr(cls), _ptr(seg_u8), ctypes.cast(table, ctypes.c_void_p), n, L, B, Q, K, h, w,
                                   _ptr(partials), s), "s2f_seg_log_partials")
    check(lib.s2f_seg_log_rows(_ptr(partials), n, per_layer, K, _ptr(ring), window, _ptr(streak), patience, _ptr(head), s),
          "s2f_seg_log_rows")
    return ring


__all__ = ["SEG_LOG_MAX_LAYERS", "SEG_LOG_MAX_CLASSES", "seg_log_tiles", "seg_log_append"]
