"""The two launches of the weight average (csrc/ema.hip): `ema_update`, every parameter of a pointer table copied into or averaged
towards its slot of one flat fp32 buffer, and `ema_swap`, parameters and slots exchanged bit for bit.  The tables are
`train.FlatAdamW`'s (`slots` / `chunks`): the kernels read the parameters through the pointers baked into `slots`.  CPU tensors run
the same semantics in torch (as `state_copy` does), so that ema.WeightEMA and the hooks of runner.py can be driven without a GPU;
tests/ema_ref.py restates both in numpy."""
import torch

from .core import _ptr, _stream, check, lib


def _tables(what, slots, chunks, ema):
    if slots.dtype != torch.int64 or slots.dim() != 2 or slots.shape[1] != 3 or not slots.is_contiguous():
        raise ValueError(f"{what}: slots is a contiguous int64 [n, 3]")
    if chunks.dtype != torch.int32 or chunks.dim() != 2 or chunks.shape[1] != 2 or not chunks.is_contiguous() or chunks.shape[0] < 1:
        raise ValueError(f"{what}: chunks is a contiguous int32 [nchunks >= 1, 2]")
    if ema.dtype != torch.float32 or ema.dim() != 1 or not ema.is_contiguous():
        raise ValueError(f"{what}: ema is one contiguous fp32 buffer")
    if slots.device != ema.device or chunks.device != ema.device:
        raise RuntimeError(f"{what}: tables on {slots.device} / {chunks.device}, ema on {ema.device}")


def _cpu_pairs(what, slots, ema, params):
    """the CPU route's (parameter as flat fp32, its slot of ema) pairs"""
    if params is None:
        raise RuntimeError(f"{what}: the CPU route reads the parameters themselves (params=...), not the table's pointers")
    params = list(params)
    if len(params) != slots.shape[0]:
        raise ValueError(f"{what}: {len(params)} parameters for a table of {slots.shape[0]} slots")
    out = []
    for p, (_, off, n) in zip(params, slots.tolist()):
        if p.dtype != torch.float32 or p.numel() != n or not p.is_contiguous() or off + n > ema.numel():
            raise ValueError(f"{what}: the table does not describe these parameters")
        out.append((p.detach().reshape(-1), ema[off:off + n]))
    return out


def ema_update(slots, chunks, ema, state, table, begin=0, interval=1, partials=None, params=None):
    """One update of the average (s2f_ema_update), behind s2f_adamw_step: with t = state[4] (the optimizer's count of this update,
    from 1) and c = t - max(begin, 1): c <= 0 copies the parameters into `ema` bit for bit, a c that `interval` does not divide
    touches nothing, any other c averages, e += table[min(c, len(table) - 1)] * (p - e) in three separately rounded fp32 operations
    (a NaN result is the quiet NaN 0x7fc00000).  slots int64 [n, 3], chunks int32 [nchunks, 2]: FlatAdamW's; ema: fp32, the layout of
    the moments; state: fp32 [>= 5]; table: fp32 [>= 1] momenta; partials: None or fp64 [nchunks, 2] <- per chunk {sum (p - e)^2, sum
    e^2} after the update.  One launch on the current stream, no synchronisation, capturable.  `params`: the parameters of the
    table in its order -- read by the CPU route only (the kernel reads the pointers baked into `slots`)."""
    _tables("ema_update", slots, chunks, ema)
    if state.dtype != torch.float32 or state.dim() != 1 or state.numel() < 5 or not state.is_contiguous():
        raise ValueError("ema_update: state is a contiguous fp32 [>= 5]")
    if table.dtype != torch.float32 or table.dim() != 1 or table.numel() < 1 or not table.is_contiguous():
        raise ValueError("ema_update: table is a contiguous fp32 [>= 1]")
    if partials is not None and (partials.dtype != torch.float64 or tuple(partials.shape) != (chunks.shape[0], 2)
                                 or not partials.is_contiguous()):
        raise ValueError(f"ema_update: partials is a contiguous fp64 [{chunks.shape[0]}, 2]")
    if any(t is not None and t.device != ema.device for t in (state, table, partials)):
        raise RuntimeError("ema_update: every tensor lives on the ema buffer's device")
    begin, interval = int(begin), int(interval)
    if begin < 0 or interval < 1:
        raise ValueError(f"ema_update: begin {begin} below 0 or interval {interval} below 1")
    if not ema.is_cuda:
        c = int(state[4]) - max(begin, 1)
        if c > 0 and c % interval:
            return ema
        m = None if c <= 0 else table[min(c, table.numel() - 1)]
        rows = []
        chunk = int(lib.s2f_adamw_chunk_elems())
        for p, e in _cpu_pairs("ema_update", slots, ema, params):
            if m is None:
                e.view(torch.int32).copy_(p.view(torch.int32))
            else:
                r = e + m * (p - e)          # three tensor operations: each rounds to fp32 on its own
                e.copy_(torch.where(torch.isnan(r), torch.tensor(0x7FC00000, dtype=torch.int32).view(torch.float32), r))
            for s in range(0, p.numel(), chunk):
                pd, ed = p[s:s + chunk].double(), e[s:s + chunk].double()
                rows.append((float(((pd - ed) ** 2).sum()), float((ed ** 2).sum())))
        if partials is not None:
            partials.copy_(torch.tensor(rows, dtype=torch.float64).reshape(-1, 2))
        return ema
    check(lib.s2f_ema_update(_ptr(slots), _ptr(chunks), chunks.shape[0], _ptr(ema), _ptr(state), _ptr(table), table.numel(), begin,
                             interval, None if partials is None else _ptr(partials), _stream()), "s2f_ema_update")
    return ema


def ema_swap(slots, chunks, ema, params=None):
    """Every parameter of the table <-> its slot of `ema` (s2f_ema_swap): bits, no arithmetic; twice is the identity.  The caller
    bumps the parameters' version counters (FlatAdamW.mark_updated).  One launch on the current stream; capturable.  `params`: as
    in `ema_update`."""
    _tables("ema_swap", slots, chunks, ema)
    if not ema.is_cuda:
        for p, e in _cpu_pairs("ema_swap", slots, ema, params):
            pb, eb = p.view(torch.int32), e.view(torch.int32)
            keep = pb.clone()
            pb.copy_(eb)
            eb.copy_(keep)
        return ema
    check(lib.s2f_ema_swap(_ptr(slots), _ptr(chunks), chunks.shape[0], _ptr(ema), _stream()), "s2f_ema_swap")
    return ema


__all__ = ["ema_update", "ema_swap"]
