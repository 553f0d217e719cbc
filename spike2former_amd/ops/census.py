"""The operand census of one tensor (csrc/opcensus.hip) and its CPU implementation."""
import torch

from .core import *          # noqa: F401,F403  (the shared plumbing: _ptr, _stream, check, lib, Spikes, ...)

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


__all__ = [n for n in dir() if not n.startswith('__')]
