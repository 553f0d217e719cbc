"""The weight-conversion cache.  Every matrix-core product multiplies by a converted copy of its fp32 weight: a bf16 hi / mid / lo
SPLIT [3, Mpad, Kpad], or a bf16 PACK (s2f.h "pipelined GEMMs": blocks of [3 terms][64 rows][32 k], the LDS image of the LDS-DMA
kernels of csrc/pgemm.hip -- the forward spike GEMMs on s2f_pgemm_nn_bf16, and every fp32 x fp32 product, the input gradients of the
1x1 convolutions and the forward products of the convolutions whose input is no spike map, on s2f_pgemm_dx_f32: 6 bf16 passes = fp32
accuracy).  Seven layouts (`_LAYOUTS`), one conversion routine (`_convert`), one cached copy per weight and layout.

A captured training step bakes the buffers' addresses into its hipGraph, ops.resplit_all redoes every conversion from the live
weights in two launches over device job tables, and an eager step after an optimiser update converts again.  Four rules keep those
three in step:
  * owner, not address: an entry belongs to a tensor OBJECT (weak reference, `_owner`); key, shape, owner and version make a hit;
  * convert into the same buffer: a stale entry of the same weight is converted INTO again (`_convert`);
  * tables replaced, never mutated: a job table tensor is not written again once built (`_Table`, `_store` only invalidates);
  * trust only inside a capture after the recorded resplit_all: then, and only then, a moved version is adopted without a launch
    (`step_begins`, `_convert`)."""
import types
import typing
import weakref

import torch

from .config import cfg
from .core import _ptr, _stream, check, lib


class Job(typing.NamedTuple):
    """What the _multi kernels need to redo one conversion from the live weight (resplit_all).  Only the address is kept (a tensor
    would keep a freed model's weights allocated); it is used only while the owner is alive and its storage still covers it."""
    src: int
    mode: int
    cdim: int
    M: int
    K: int


class Entry(typing.NamedTuple):
    version: int                    # None: forgotten (forget_versions) -- the next use converts again
    out: torch.Tensor
    shape: tuple
    owner: weakref.ref
    job: Job                        # None: the source was not contiguous -- converted through a copy, left out of resplit_all
    kind: str                       # "split" | "pack": which job table


class _Table(typing.NamedTuple):
    """Job table of resplit_all, one per conversion kernel.  A table tensor is REPLACED, never written again, once built: a
    captured graph keeps reading the tensor it recorded (graph.py holds references to the tables and buffers of its capture)."""
    rows: torch.Tensor = None
    njobs: int = 0
    blocks: int = 0


# The module's state, one object (ops/__init__.py copies module names by value).  entries: (layout tag, address, numel) -> Entry;
# keys: the entries the tables `split` / `pack` were built for, None: to be rebuilt;  trust: set by step_begins() inside a capture --
# every registered conversion was just redone from the live weights
conversions = types.SimpleNamespace(entries={}, keys=None, split=_Table(), pack=_Table(), trust=False)


def _up(n, m):
    return (n + m - 1) // m * m


def _plain(R, C):
    return R, C, 0, (R, C)


def _tap_major(Mw, C, _kh, _kw):    # [M, (ky, kx, c)]: what the implicit 3x3 kernels contract over
    return Mw, 9 * C, C, (Mw, C)


def _flipped_t(Mw, C, _kh, _kw):    # [C, (ky, kx, m)], Wt[c][(ky, kx), m] = weight[m][c][2 - ky][2 - kx]: the transposed convolution
    return C, 9 * Mw, Mw, (Mw, C)


# The seven layouts: key tag -> (mode, dims, matrix, mpad).
#   mode   : the source layout as s2f_pack_bf16x3 and the two _multi kernels name it
#   dims   : (*weight.shape) -> (M, K, cdim, the entry's `shape`)
#   matrix : splits only -- the [M, K] matrix as an ATen view / copy for the eager launch: s2f_split_bf16x3 takes no mode, only the
#            _multi kernel reads the 3x3 layouts directly.  None: a pack (buffer of s2f_pack_elems(M, K) elements)
#   mpad   : a split buffer is [3, Mpad, Kpad] with Mpad a multiple of this (128: what s2f_conv3x3_general needs), Kpad of 32
_LAYOUTS = {
    "split": (0, _plain, lambda w: w, 64),
    "split_tap": (1, _tap_major, lambda w: w.permute(0, 2, 3, 1).flatten(1), 64),
    "split_flip": (2, _flipped_t, lambda w: w.flip(2, 3).permute(1, 2, 3, 0).flatten(1), 128),
    "pack": (0, _plain, None, 0),
    "pack_t": (3, lambda R, C: (C, R, 0, (C, R)), None, 0),
    "pack_tap": (1, _tap_major, None, 0),
    "pack_flip": (2, _flipped_t, None, 0),
}


def _owner(t):
    """The long-lived tensor object a cached conversion belongs to: the parameter a view was taken from (or the first twin of a
    zero-copy concatenation).  The cache keeps a weak reference to it -- an address is not an identity: once a model is
    freed, another model's weight of the same shape lands on the same address with the same version counter."""
    o = getattr(t, "_s2f_owner", None)
    if o is not None:
        return o
    return t._base if t._base is not None else t


def _store(key, entry):
    entries = conversions.entries
    if len(entries) > 4096:                            # dead entries of freed models
        for k in [k for k, e in entries.items() if e.owner() is None]:
            del entries[k]
    old = entries.get(key)
    entries[key] = entry
    if old is None or old.out is not entry.out or old.job != entry.job:
        conversions.keys = None                        # a new destination: the job tables must be rebuilt (never mutated)


def _convert(w, tag):
    """version -> lookup -> destination -> launch -> store, for every layout.  Re-converted when the weight is modified in place
    (optimiser step, load_state_dict) -- tracked through the tensor version counter; weights must not be mutated through `.data`
    (its own version counter).  Inside a captured step the conversions are redone by resplit_all()."""
    mode, dims, matrix, mpad = _LAYOUTS[tag]
    M, K, cdim, shape = dims(*w.shape)
    key = (tag, w.data_ptr(), M * K)          # (M * K = w.numel())
    # a zero-copy concatenation of sibling parameters (cat_params) is a fresh tensor every call: it carries the sum of the
    # parameters' version counters instead of its own
    version = getattr(w, "_s2f_version", w._version)
    owner = _owner(w)
    old = conversions.entries.get(key)
    mine = old is not None and old.shape == shape and old.owner() is owner          # (never the address alone)
    if mine and old.version == version:
        return old.out
    if mine and conversions.trust and old.job is not None and torch.cuda.is_current_stream_capturing():
        conversions.entries[key] = old._replace(version=version)
        return old.out
    split = matrix is not None
    out_shape = (3, _up(M, mpad), _up(K, 32)) if split else (int(lib.s2f_pack_elems(M, K)),)
    # the destination: the buffer of a stale entry of the same weight is converted INTO again -- a captured hipGraph (and the job
    # tables of resplit_all) hold its address, a fresh allocation would leave them writing into freed memory -- otherwise a new one
    reuse = mine and old.out.device == w.device and tuple(old.out.shape) == out_shape
    out = old.out if reuse else torch.empty(out_shape, dtype=torch.int16, device=w.device)
    src = w.detach()
    job = Job(src.data_ptr(), mode, cdim, M, K) if src.is_contiguous() else None          # (a copy below is no source for resplit_all)
    mat = (matrix(src) if split else src).contiguous()
    if split:
        check(lib.s2f_split_bf16x3(_ptr(mat), _ptr(out), M, K, out_shape[1], out_shape[2], _stream()), "s2f_split_bf16x3")
    else:
        check(lib.s2f_pack_bf16x3(_ptr(mat), _ptr(out), M, K, mode, cdim, _stream()), "s2f_pack_bf16x3")
    _store(key, Entry(version, out, shape, weakref.ref(owner), job, "split" if split else "pack"))
    return out


def split_weight(w2d):
    """fp32 [M, K] -> cached bf16 [3, Mpad, Kpad] (hi, mid, lo)."""
    return _convert(w2d, "split")


def split_weight_conv3(weight):
    """[M, C, 3, 3] -> cached bf16 split of the TAP-MAJOR matrix [M, (ky, kx, c)] that the implicit 3x3 kernels contract over."""
    return _convert(weight, "split_tap")


def split_weight_tconv3(weight):
    """[M, C, 3, 3] -> cached bf16 split of the transposed-convolution matrix [C, (ky, kx, m)] with flipped taps
    (Wt[c][(ky, kx), m] = weight[m][c][2 - ky][2 - kx]), rows padded to a multiple of 128 for s2f_conv3x3_general."""
    return _convert(weight, "split_flip")


def pack_weight(w2d, transposed=False):
    """fp32 [M, K] -> the cached bf16 PACK of it, or of its transpose (`transposed`: the pack of w2d^T, the A operand of the forward
    product of a convolution whose input is a general fp32 tensor).  The pack of W serves its forward product (s2f_pgemm_nn_bf16)
    AND the input gradient W^T dY (s2f_pgemm_dx_f32)."""
    return _convert(w2d, "pack_t" if transposed else "pack")


def pack_weight_conv3(weight, transposed=False):
    """[M, C, 3, 3] -> the cached PACK (see pack_weight) of the TAP-MAJOR matrix [M, (ky, kx, c)] the implicit 3x3 kernels contract
    over (s2f_pgemm_conv3x3_bf16), or -- `transposed` -- of the transposed-convolution matrix [C, (ky, kx, m)] with flipped taps:
    the A operand of the input gradient (s2f_pgemm_conv3x3_f32)."""
    return _convert(weight, "pack_flip" if transposed else "pack_tap")


def conversion_state():
    """What a captured step must keep alive: the job tables resplit_all launched with and every cached conversion buffer."""
    return (conversions.split.rows, conversions.pack.rows, [e.out for e in conversions.entries.values()])


def clear_conversions():
    """Forget every cached conversion (tests): the next use converts into a fresh buffer, the next resplit_all builds new tables."""
    conversions.entries.clear()
    conversions.keys = None


def _table(entries, device):
    """The job rows of one _multi kernel (include/s2f.h); `first`: the job's first workgroup in the launch."""
    rows, first = [], 0
    for e in entries:
        j, dst, word = e.job, e.out.data_ptr(), e.job.mode | (e.job.cdim << 8)
        if e.kind == "pack":
            rows.append([j.src, dst, j.M, j.K, word, first, 0, 0])
            first += (_up(j.M, 64) // 64) * (_up(j.K, 32) // 32) * 2
        else:
            _, Mpad, Kpad = e.out.shape
            rows.append([j.src, dst, j.M, j.K, Mpad, Kpad, word, first])
            first += (Mpad * Kpad + 1023) // 1024
    return _Table(torch.tensor(rows, dtype=torch.int64).to(device) if rows else None, len(rows), first)


def resplit_all(device, build=True):
    """Redo EVERY cached weight conversion (bf16 hi/mid/lo splits and packs) from the live fp32 weights: one launch per
    conversion kernel (s2f_split_bf16x3_multi, s2f_pack_bf16x3_multi).  A training step owes this after each optimiser update;
    a captured step (graph.GraphedStep) records it, so every replay multiplies by the current weights -- without it the graph
    would replay the bf16 terms of capture time while its backward reads the live fp32 weights.  -> number of weights
    converted; -1 when the job tables would have to be (re)built and `build` is False (they are uploaded from the host, which
    a stream capture does not allow: GraphedStep calls this once before capturing)."""
    def covered(e):
        o = e.owner()
        if o is None or e.job is None or e.out.device != device:
            return False
        st = o.untyped_storage()
        return st.data_ptr() <= e.job.src and e.job.src + 4 * e.job.M * e.job.K <= st.data_ptr() + st.nbytes()
    S = conversions
    live = {k: e for k, e in S.entries.items() if covered(e)}
    if not live:
        return 0
    built = S.split.rows if S.split.rows is not None else S.pack.rows
    if S.keys != tuple(live) or built is None or built.device != device:
        if not build:
            return -1
        S.keys = tuple(live)
        S.split, S.pack = (_table([e for e in live.values() if e.kind == kind], device) for kind in ("split", "pack"))
    if S.split.njobs:
        check(lib.s2f_split_bf16x3_multi(_ptr(S.split.rows), S.split.njobs, S.split.blocks, _stream()), "s2f_split_bf16x3_multi")
    if S.pack.njobs:
        check(lib.s2f_pack_bf16x3_multi(_ptr(S.pack.rows), S.pack.njobs, S.pack.blocks, _stream()), "s2f_pack_bf16x3_multi")
    return len(live)


def forget_versions():
    """Every cached weight converts again at its next use, by its own launch, INTO its buffer."""
    for k, e in conversions.entries.items():
        conversions.entries[k] = e._replace(version=None)


def step_begins(device):
    """core.begin_step: a step that is being captured into a hipGraph re-converts every weight first (two launches, recorded in
    the graph): the replays then read the live fp32 weights instead of the bf16 terms of capture time."""
    conversions.trust = False
    if device is not None and torch.cuda.is_current_stream_capturing() and cfg.RESPLIT_IN_GRAPH:
        n = resplit_all(device, build=False)
        if n > 0:
            conversions.trust = True
        elif n < 0:
            # no job table for the current set of weights: each weight is re-converted by its own launch inside this capture
            # (correct, ~180 launches more per replay)
            forget_versions()

