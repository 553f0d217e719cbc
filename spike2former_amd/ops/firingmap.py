"""The firing maps of one neuron output and their drawing (csrc/firingmap.hip), each with its CPU implementation."""
import math

import torch

from .core import *          # noqa: F401,F403  (the shared plumbing: _ptr, _stream, check, lib, Spikes, ...)
from .census import _CENSUS_DTYPES
from .segeval import _SEG_DRAW_BGR

FIRING_MAP_ASSIGN = 1                # include/s2f.h S2F_FIRING_MAP_ASSIGN
FIRING_MAP_PLANES = 4                # level sum, non-zero, max level, off grid
FIRING_MAP_MAX_LEVEL = 65535         # the largest level one element adds to plane 0


def firing_map_sum_ok(planes, passes=1):
    """whether `passes` passes over `planes` = (TB / B) C planes per image keep plane 0 inside int32: the entry point's bound for one
    pass, the host's for the passes it accumulates"""
    return int(planes) * int(passes) * FIRING_MAP_MAX_LEVEL < 2 ** 31


def _firing_map_torch(x, TB, B, C, P, D, stats, assign):
    """the semantics of s2f_firing_map in exact integer torch arithmetic (CPU tensors)"""
    xf = x.reshape(TB // B, B, C, P).to(torch.float32)          # (bf16 -> fp32 is exact); row n = t B + b belongs to image b
    mag = xf.view(torch.int32) & 0x7fffffff
    p = xf * torch.tensor(D, dtype=torch.float32)          # ONE fp32 multiply by D converted to fp32
    finite = mag < 0x7f800000
    subnormal = (mag != 0) & (mag < 0x00800000)
    on = finite & ~subnormal & (p >= 0) & (p <= 65535) & (p == p.trunc())
    level = torch.where(on, p, torch.zeros_like(p)).to(torch.int64)
    new = torch.stack([level.sum((0, 2)), (mag != 0).sum((0, 2)), level.amax((0, 2)), (~on).sum((0, 2))], 1).to(torch.int32)
    flat = stats.view(B, FIRING_MAP_PLANES, P)
    if assign:
        flat.copy_(new)
    else:
        new[:, 2] = torch.maximum(flat[:, 2], new[:, 2])
        new[:, (0, 1, 3)] += flat[:, (0, 1, 3)]
        flat.copy_(new)
    return stats


def firing_map(x, B, D, stats, assign=False):
    """stats int32 [B, 4, *map] (+)= the firing maps of one neuron output (s2f_firing_map, include/s2f.h "firing maps"): per image and
    pixel, over the time steps and channels, {sum of the integer levels x * D, non-zero elements, max level (a running maximum),
    elements off the level grid}.  x: a tensor or an ops.Spikes (then its stored data), fp32 or bf16, CONTIGUOUS, t-major: its
    trailing dimensions are the map's (stats.shape[2:]: (h, w) or one N), the one in front of them the channels, everything before
    them T B rows of which row n belongs to image n % B.  `assign`: the planes are written instead of added to (the first pass
    after a clear needs no clear launch).  CUDA tensors run the kernel, one launch; CPU tensors the same arithmetic in torch (the
    package's CPU implementation of this op, no fall-back site)."""
    x = x.data if isinstance(x, Spikes) else x
    B, D = int(B), int(D)
    if x.dtype not in _CENSUS_DTYPES:
        raise TypeError(f"firing_map: a neuron output is fp32 or bf16; got {x.dtype}")
    if D < 1 or B < 1:
        raise ValueError(f"firing_map: D {D} and B {B} are at least 1")
    if (stats.dtype != torch.int32 or stats.dim() < 3 or tuple(stats.shape[:2]) != (B, FIRING_MAP_PLANES)
            or not stats.is_contiguous()):
        raise ValueError(f"firing_map: stats is a contiguous int32 [{B}, {FIRING_MAP_PLANES}, *map]; got {stats.dtype} "
                         f"{tuple(stats.shape)}")
    space = tuple(stats.shape[2:])
    if x.dim() < len(space) + 2 or tuple(x.shape[x.dim() - len(space):]) != space:
        raise ValueError(f"firing_map: x {tuple(x.shape)} does not end in a channel dimension and the map {space}")
    if not x.is_contiguous():
        raise ValueError("firing_map: x is not contiguous")
    lead = x.dim() - len(space) - 1
    TB, C, P = math.prod(x.shape[:lead]), x.shape[lead], math.prod(space)
    if TB < 1 or C < 1 or TB % B:
        raise ValueError(f"firing_map: {TB} leading rows of {C} channels for {B} images")
    if not firing_map_sum_ok(TB // B * C):
        raise ValueError(f"firing_map: {TB // B * C} planes per image: their level sum may pass 2^31")
    if stats.device != x.device:
        raise RuntimeError(f"firing_map: the output on {x.device}, the maps on {stats.device}")
    x = x.detach()
    if not x.is_cuda:
        return _firing_map_torch(x, TB, B, C, P, D, stats, bool(assign))
    if P:
        check(lib.s2f_firing_map(_ptr(x), _CENSUS_DTYPES[x.dtype], TB, B, C, P, D, _ptr(stats), FIRING_MAP_ASSIGN if assign else 0,
                                 _stream()), "s2f_firing_map")
    return stats


def _firing_axis(big, small):
    """per output coordinate of an axis of `big` samples over a plane axis of `small`: (z0, z1, f) as int64 tensors"""
    z = torch.arange(big, dtype=torch.int64)
    nz = ((2 * z + 1) * small - big).clamp_(min=0)
    z0 = nz // (2 * big)
    f = ((nz - z0 * 2 * big) * 256) // (2 * big)
    return z0, (z0 + 1).clamp_(max=small - 1), f


def _firing_draw_torch(image, plane, full, lut, a8, bgr, out):
    """the semantics of s2f_firing_draw in exact integer torch arithmetic (CPU tensors)"""
    H, W = image.shape[:2]
    s = plane.to(torch.int64).clamp_(min=0)
    y0, y1, fy = _firing_axis(H, plane.shape[0])
    x0, x1, fx = _firing_axis(W, plane.shape[1])
    fy, fx = fy[:, None], fx[None, :]
    top = (256 - fx) * s[y0][:, x0] + fx * s[y0][:, x1]
    bottom = (256 - fx) * s[y1][:, x0] + fx * s[y1][:, x1]
    v = (256 - fy) * top + fy * bottom
    idx = ((255 * v + 32768 * full) // (65536 * full)).clamp_(max=255)
    col = lut.to(torch.int64)[idx]          # [H, W, 3]
    img = image.to(torch.int64)
    if bgr:
        img = img.flip(2)
    out.copy_(((img * (256 - a8) + col * a8 + 128) >> 8).to(torch.uint8))
    return out


def firing_draw(image, plane, full, lut, alpha, bgr=False, out=None):
    """-> uint8 [H, W, 3] RGB: one int32 plane [h, w] resampled to the picture's size, looked up in the colour table lut (uint8
    [256, 3] RGB; `full` and above is its last row) and blended into `image` (uint8 [H, W, 3], RGB or (`bgr`) BGR) with weight
    a8 / 256, a8 = floor(alpha * 256 + 0.5) -- s2f_firing_draw, include/s2f.h "firing maps": integer arithmetic throughout, one
    definition of every byte.  `out`: a uint8 [H, W, 3] tensor or VIEW whose pixels are 3 bytes apart and whose rows are at least 3 W
    bytes apart (a tile of a larger panel); allocated when None.  CUDA tensors run the kernel, one launch; CPU tensors the same
    arithmetic in torch (the package's CPU implementation of this op)."""
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3 or image.numel() == 0:
        raise ValueError("firing_draw: image is uint8 [H, W, 3]")
    if plane.dtype != torch.int32 or plane.dim() != 2 or plane.numel() == 0:
        raise ValueError("firing_draw: plane is int32 [h, w]")
    if lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
        raise ValueError("firing_draw: lut is uint8 [256, 3]")
    H, W = image.shape[:2]
    full, alpha = int(full), float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"firing_draw: alpha {alpha} outside 0 .. 1")
    if not 1 <= full <= 2 ** 40:
        raise ValueError(f"firing_draw: full {full} outside 1 .. 2^40")
    if not (H * W < 2 ** 31 - 8 and plane.numel() < 2 ** 31):
        raise ValueError(f"firing_draw: {H} x {W} pixels or a plane of {plane.numel()} elements: below 2^31 each")
    a8 = int(math.floor(alpha * 256 + 0.5))
    if out is None:
        out = torch.empty(H, W, 3, dtype=torch.uint8, device=image.device)
    if (out.dtype != torch.uint8 or tuple(out.shape) != (H, W, 3) or out.stride(2) != 1 or out.stride(1) != 3
            or (H > 1 and out.stride(0) < 3 * W)):
        raise ValueError(f"firing_draw: out is uint8 [{H}, {W}, 3] with pixels 3 bytes and rows at least {3 * W} bytes apart")
    for t in (plane, lut, out):
        if t.device != image.device:
            raise RuntimeError(f"firing_draw: a tensor on {t.device}, the image on {image.device}")
    image, plane, lut = image.contiguous(), plane.contiguous(), lut.contiguous()
    if not image.is_cuda:
        return _firing_draw_torch(image, plane, full, lut, a8, bool(bgr), out)
    check(lib.s2f_firing_draw(_ptr(image), _ptr(plane), plane.shape[0], plane.shape[1], full, _ptr(lut), a8, _SEG_DRAW_BGR if bgr else 0,
                              H, W, _ptr(out), out.stride(0) if H > 1 else 3 * W, _stream()), "s2f_firing_draw")
    return out


__all__ = [n for n in dir() if not n.startswith('__')]
