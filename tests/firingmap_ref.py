"""The two kernels of csrc/firingmap.hip restated in numpy int64 (include/s2f.h "firing maps") -- and nothing else.  Every test of the
firing maps compares integers or bytes against these two functions."""
import numpy as np


def _fp32_bits(x):
    """x: a numpy float32 array, or uint16 holding bf16 bit patterns -> (uint32 bits, the float32 values)"""
    if x.dtype == np.uint16:
        bits = x.astype(np.uint32) << 16
        return bits, bits.view(np.float32)
    assert x.dtype == np.float32
    x = np.ascontiguousarray(x)
    return x.view(np.uint32), x


def firing_map(x, B, D, stats=None, assign=False):
    """x: [TB, C, P] float32 (or uint16 = bf16 bits); -> int64 [B, 4, P].  stats: the planes before the call (None: zeros)."""
    TB, C, P = x.shape
    assert TB % B == 0
    bits, val = _fp32_bits(x)
    mag = bits & np.uint32(0x7fffffff)
    with np.errstate(all="ignore"):
        p = val * np.float32(D)          # ONE fp32 multiply
        finite = mag < 0x7f800000
        subnormal = (mag != 0) & (mag < 0x00800000)
        on = finite & ~subnormal & (p >= 0) & (p <= 65535) & (p == np.trunc(p))
        level = np.where(on, p, np.float32(0)).astype(np.int64)
    new = np.zeros((B, 4, P), np.int64)
    shape = (TB // B, B, C, P)          # row n = t B + b belongs to image b
    new[:, 0] = level.reshape(shape).sum((0, 2))
    new[:, 1] = (mag != 0).reshape(shape).sum((0, 2))
    new[:, 2] = level.reshape(shape).max((0, 2)) if P else 0
    new[:, 3] = (~on).reshape(shape).sum((0, 2))
    if stats is None or assign:
        return new
    out = np.asarray(stats, np.int64) + new
    out[:, 2] = np.maximum(np.asarray(stats, np.int64)[:, 2], new[:, 2])
    return out


def _axis(big, small):
    z = np.arange(big, dtype=np.int64)
    nz = np.maximum(0, (2 * z + 1) * small - big)
    z0 = nz // (2 * big)
    f = ((nz - z0 * 2 * big) * 256) // (2 * big)
    return z0, np.minimum(z0 + 1, small - 1), f


def firing_index(plane, full, H, W):
    """plane: int [h, w] -> int64 [H, W], the colour-table row of every output pixel"""
    s = np.maximum(0, np.asarray(plane, np.int64))
    y0, y1, fy = _axis(H, s.shape[0])
    x0, x1, fx = _axis(W, s.shape[1])
    fy, fx = fy[:, None], fx[None, :]
    v = (256 - fy) * ((256 - fx) * s[y0][:, x0] + fx * s[y0][:, x1]) + fy * ((256 - fx) * s[y1][:, x0] + fx * s[y1][:, x1])
    return np.minimum(255, (255 * v + 32768 * int(full)) // (65536 * int(full)))


def firing_draw(image, plane, full, lut, a8, bgr=False):
    """image: uint8 [H, W, 3]; plane: int [h, w]; lut: uint8 [256, 3]; a8 in 0 .. 256 -> uint8 [H, W, 3] RGB"""
    H, W = image.shape[:2]
    col = np.asarray(lut, np.int64)[firing_index(plane, full, H, W)]
    img = np.asarray(image, np.int64)
    if bgr:
        img = img[:, :, ::-1]
    return ((img * (256 - a8) + col * a8 + 128) >> 8).astype(np.uint8)
