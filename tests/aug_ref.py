"""numpy restatement of the device-side training augmentation (spike2former_amd/csrc/augment.hip, spike2former_amd/augment.py) --
a test helper, no conftest.  Written from the reference's mmseg/datasets/transforms/transforms.py for the order of the stages,
the probabilities, `PhotoMetricDistortion.convert` and `RandomCrop.crop_bbox`'s rule, from mmcv's `rescale_size` for the geometry,
and from the formulas of include/s2f.h for the two pieces the reference hands to OpenCV (the bilinear resize and the 8-bit HSV
conversions).  Every float operation is ONE operation of `dtype` on arrays of `dtype` (float32 by default: what the kernel does,
operation for operation; float64: the same chain in double precision, for measuring how far fp32 round-off can move a grey level).

A parameter record `p` is anything indexable by the field names of S2fAugParams (a row of TrainAugment.PARAM_DTYPE or a dict)."""
import numpy as np

CANDIDATES = 11


# ------------------------------------------------------------------------------------------------ geometry (mmcv rescale_size)
def resized_size(h0, w0, scale, ratio):
    """RandomResize(scale, ratio_range, keep_ratio=True) at the drawn `ratio` -> (H, W)"""
    long_edge, short_edge = max(int(scale[0] * ratio), int(scale[1] * ratio)), min(int(scale[0] * ratio), int(scale[1] * ratio))
    f = min(long_edge / max(h0, w0), short_edge / min(h0, w0))
    return int(h0 * f + 0.5), int(w0 * f + 0.5)


def margins(H, W, crop_size):
    return max(H - crop_size[0], 0), max(W - crop_size[1], 0)


# ------------------------------------------------------------------------------------------------ annotation
def reduce_zero_label(seg):
    """LoadAnnotations(reduce_zero_label=True): 0 -> 255, 255 -> 255, l -> l - 1"""
    s = seg.astype(np.int64)
    return np.where((s == 0) | (s == 255), 255, s - 1).astype(np.uint8)


def nearest_resize(seg, H, W):
    h0, w0 = seg.shape
    sy = (np.arange(H, dtype=np.int64) * h0) // H
    sx = (np.arange(W, dtype=np.int64) * w0) // W
    return seg[sy[:, None], sx[None, :]]


def crop_passes(window, ignore_index=255, cat_max_ratio=0.75):
    """transforms.py:283-286"""
    labels, cnt = np.unique(window, return_counts=True)
    cnt = cnt[labels != ignore_index]
    return bool(len(cnt) > 1 and np.max(cnt) / np.sum(cnt) < cat_max_ratio)


def choose_candidate(seg_resized, origins, crop_size, ignore_index=255, cat_max_ratio=0.75):
    """the reference's retry loop on pre-drawn origins: the first passing one of candidates 0 .. 9, else candidate 10; -> (index,
    [pass flag of every candidate])"""
    flags = [crop_passes(seg_resized[y:y + crop_size[0], x:x + crop_size[1]], ignore_index, cat_max_ratio) for y, x in origins]
    if cat_max_ratio >= 1.0:
        return 0, flags
    for i in range(CANDIDATES - 1):
        if flags[i]:
            return i, flags
    return CANDIDATES - 1, flags


# ------------------------------------------------------------------------------------------------ bilinear resize
def _taps(n_in, n_out, dtype):
    f = dtype
    scale = f(n_in) / f(n_out)
    src = scale * (np.arange(n_out).astype(f) + f(0.5)) - f(0.5)
    src = np.where(src < 0, f(0), src).astype(f)
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, (src - i0.astype(f)).astype(f)


def bilinear_float(img, H, W, dtype=np.float32):
    """img [h0, w0, C] uint8 -> [H, W, C] `dtype`: half-pixel centres, no antialias (ATen upsample_bilinear2d, align_corners=False)"""
    f = dtype
    y0, y1, ly = _taps(img.shape[0], H, f)
    x0, x1, lx = _taps(img.shape[1], W, f)
    a = img.astype(f)
    ly, lx = ly[:, None, None], lx[None, :, None]
    one = f(1)
    top = (one - lx) * a[y0][:, x0] + lx * a[y0][:, x1]
    bot = (one - lx) * a[y1][:, x0] + lx * a[y1][:, x1]
    out = (one - ly) * top + ly * bot
    assert out.dtype == f
    return out


def bilinear_u8(img, H, W, dtype=np.float32):
    return np.rint(bilinear_float(img, H, W, dtype)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ photometric distortion
def convert(img, alpha, beta, dtype=np.float32):
    """transforms.py:636-638: fp32(img) * alpha + beta, clipped to 0 .. 255, truncated"""
    f = dtype
    v = img.astype(f) * f(alpha) + f(beta)
    return np.clip(v, f(0), f(255)).astype(np.uint8)


def bgr2hsv(img, dtype=np.float32):
    """[..., 3] uint8 BGR -> [..., 3] uint8 HSV: V = max, S = 255 (V - min) / V, hue by 60-degree sectors (V == R, then G, then B)
    halved into 0 .. 179 with 180 wrapped to 0, each rounded to nearest"""
    f = dtype
    b, g, r = (img[..., c].astype(np.int64) for c in range(3))
    v = np.maximum(b, np.maximum(g, r))
    mn = np.minimum(b, np.minimum(g, r))
    diff = (v - mn).astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(v == 0, f(0), np.rint(f(255) * diff / v.astype(f)))
        hr = f(60) * (g - b).astype(f) / diff
        hg = f(120) + f(60) * (b - r).astype(f) / diff
        hb = f(240) + f(60) * (r - g).astype(f) / diff
    h = np.where(v == mn, f(0), np.where(v == r, hr, np.where(v == g, hg, hb))).astype(f)
    h = np.where(h < 0, h + f(360), h).astype(f)
    h = np.rint(h * f(0.5)).astype(np.int64)
    h = np.where(h >= 180, h - 180, h)
    return np.stack([h, s.astype(np.int64), v], axis=-1).astype(np.uint8)


def hsv2bgr(hsv, dtype=np.float32):
    """the standard sector inverse on the 0 .. 255 scale, each value rounded to nearest"""
    f = dtype
    h, s, v = (hsv[..., c].astype(np.int64) for c in range(3))
    vf, sf = v.astype(f), s.astype(f) / f(255)
    hh = h.astype(f) / f(30)
    i = np.minimum(hh.astype(np.int64), 5)
    fr = (hh - hh.astype(np.int64).astype(f)).astype(f)
    one = f(1)
    p = np.rint(vf * (one - sf)).astype(np.int64)
    q = np.rint(vf * (one - sf * fr)).astype(np.int64)
    t = np.rint(vf * (one - sf * (one - fr))).astype(np.int64)
    r = np.choose(i, [v, q, p, p, t, v])
    g = np.choose(i, [t, v, v, q, p, p])
    b = np.choose(i, [p, p, t, v, v, q])
    return np.stack([b, g, r], axis=-1).astype(np.uint8)


def photometric(img, p, dtype=np.float32):
    """transforms.py:716-734 with the draws of `p`: brightness, contrast here if mode == 1, saturation, hue, contrast otherwise"""
    if p["bright_on"]:
        img = convert(img, 1, p["bright_beta"], dtype)
    if p["mode"] == 1 and p["contrast_on"]:
        img = convert(img, p["contrast_alpha"], 0, dtype)
    if p["sat_on"]:
        hsv = bgr2hsv(img, dtype)
        hsv[..., 1] = convert(hsv[..., 1], p["sat_alpha"], 0, dtype)
        img = hsv2bgr(hsv, dtype)
    if p["hue_on"]:
        hsv = bgr2hsv(img, dtype)
        hsv[..., 0] = ((hsv[..., 0].astype(int) + int(p["hue_delta"])) % 180).astype(np.uint8)
        img = hsv2bgr(hsv, dtype)
    if p["mode"] != 1 and p["contrast_on"]:
        img = convert(img, p["contrast_alpha"], 0, dtype)
    return img


# ------------------------------------------------------------------------------------------------ the whole pipeline
def pipeline(img, seg, p, crop_size, mean=None, std=None, bgr_to_rgb=False, pad_val=0, seg_pad_val=255, reduce_zero=False,
             ignore_index=255, cat_max_ratio=0.75, dtype=np.float32):
    """One image.  img [h0, w0, 3] uint8 BGR, seg [h0, w0] uint8, `p` its parameter record ->
    dict(inputs [3, Hc, Wc] float32, seg [Hc, Wc] uint8, levels [hv, wv, 3] uint8 (the picture before the normalisation),
         choice (the chosen candidate), flags (every candidate's pass flag))"""
    Hc, Wc = crop_size
    H, W = int(p["H"]), int(p["W"])
    if reduce_zero:
        seg = reduce_zero_label(seg)
    img_r = bilinear_u8(img, H, W, dtype)
    seg_r = nearest_resize(seg, H, W)
    origins = [(int(y), int(x)) for y, x in zip(p["crop_y"], p["crop_x"])]
    choice, flags = choose_candidate(seg_r, origins, crop_size, ignore_index, cat_max_ratio)
    y0, x0 = origins[choice]
    img_c, seg_c = img_r[y0:y0 + Hc, x0:x0 + Wc], seg_r[y0:y0 + Hc, x0:x0 + Wc]
    if p["flip"]:
        img_c, seg_c = img_c[:, ::-1], seg_c[:, ::-1]
    levels = photometric(np.ascontiguousarray(img_c), p, dtype)
    x = levels[..., ::-1] if bgr_to_rgb else levels
    x = x.astype(np.float32).transpose(2, 0, 1)
    if mean is not None:
        x = (x - np.asarray(mean, np.float32).reshape(3, 1, 1)) / np.asarray(std, np.float32).reshape(3, 1, 1)
    hv, wv = seg_c.shape
    inputs = np.full((3, Hc, Wc), pad_val, np.float32)
    inputs[:, :hv, :wv] = x
    seg_out = np.full((Hc, Wc), seg_pad_val, np.uint8)
    seg_out[:hv, :wv] = seg_c
    return dict(inputs=inputs, seg=seg_out, levels=levels, choice=choice, flags=flags)


def batch(images, segs, params, crop_size, **kw):
    """-> inputs [B, 3, Hc, Wc] float32, seg [B, Hc, Wc] uint8, [choice per image]"""
    outs = [pipeline(i, s, p, crop_size, **kw) for i, s, p in zip(images, segs, params)]
    return np.stack([o["inputs"] for o in outs]), np.stack([o["seg"] for o in outs]), [o["choice"] for o in outs]
