"""The device-side data pipelines of csrc/augment.hip: the training augmentation and the views of a test iteration."""
import numpy as _np
import torch

from .core import *          # noqa: F401,F403  (the shared plumbing: _ptr, _stream, check, lib, Spikes, ...)

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
    _need_cuda(t, fp32=False)
    return t.numel() // entry_bytes


def aug_crop_stats(data, params, flags, crop_size, ignore_index=255, reduce_zero_label=False, cat_max_ratio=0.75):
    """flags int32 [B, 11] <- RandomCrop.crop_bbox's test of every candidate crop window of the nearest-resized annotations
    (s2f_aug_crop_stats).  data: the batch's packed uint8 pictures and annotations; params: the B-entry table (S2fAugParams) as
    bytes; both CUDA.  There is no other route: a CPU tensor raises."""
    _byte_buffer(data)
    B = _staged_table(params, AUG_PARAM_BYTES)
    _need_cuda(data, flags, fp32=False)
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
    _need_cuda(data, inputs, seg, flags, fp32=False)
    assert inputs.dtype == torch.float32 and inputs.is_contiguous() and inputs.dim() == 4 and inputs.shape[:2] == (B, 3)
    Hc, Wc = (int(v) for v in inputs.shape[-2:])
    assert seg.dtype == torch.uint8 and seg.is_contiguous() and tuple(seg.shape) == (B, Hc, Wc)
    if flags is not None:
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
    _need_cuda(data, out, fp32=False)
    V = len(table)
    if table_dev is None:
        table_dev = torch.from_numpy(_np.ascontiguousarray(table).view(_np.uint8).copy()).to(data.device)
    _staged_table(table_dev, VIEW_PARAM_BYTES, V)
    check(lib.s2f_test_views(_ptr(data), data.numel(), _ptr(table_dev), V, int(table["Hp"].max()), int(table["Wp"].max()), *m, *s,
                             int(bool(bgr_to_rgb)), float(pad_val), _ptr(out), out.numel(), _stream()), "s2f_test_views")
    return out


test_views.__test__ = False          # (an op, not a test: pytest collects `test_*` names imported into a test module)


__all__ = [n for n in dir() if not n.startswith('__')]
