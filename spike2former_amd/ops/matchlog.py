"""The match log's row (csrc/matchlog.hip): `match_log_append`, what the Hungarian assignment did in one replay -- matched pairs, their
cost, how many are also the cheapest of their class, how many changed hands since the layer before, whether matched queries classify
their target, how many unmatched ones claim an object, which queries were used -- into a ring on the device.  HIP only -- the figures
are kernels of the captured step; CPU tensors raise (the numpy restatement is tests/matchlog_ref.py)."""
import torch

from .core import _ptr, _stream, check, lib
from .maskloss import LSA_MAX_CLASSES, LSA_MAX_QUERIES

MATCH_LOG_MAX_LAYERS = 16          # include/s2f.h S2F_MATCH_LOG_MAX_LAYERS
MATCH_LOG_FIELDS = ("matched", "cost", "greedy", "moved", "cls_hit", "unmatched_obj")          # S2F_MATCH_LOG_FIELDS of them


def match_log_row_words(L, Q):
    """the 8-byte words of one row: int64 [L, 6], then usage int32 [Q] padded to whole words"""
    return len(MATCH_LOG_FIELDS) * int(L) + (int(Q) + 1) // 2


def match_log_append(cost, cls, row_class, partials, usage, ring, idle, head, patience):
    """One row of the assignment's figures (s2f_match_log_partials -> s2f_match_log_rows).  cost fp32 [L, B, Q, K] as
    MaskFormerLoss.costs_all_classes returns it, cls fp32 [L, B, Q, K+1] (logits, the void column last), row_class int32 [B, L*Q] as
    ops.lsa_tables / MaskFormerLoss.match_tables write it (a value outside 0 .. K-1: unmatched); partials int64 [L, B, 6] and usage
    int32 [B, Q] (workspace); ring int64 [window, match_log_row_words(L, Q)]; idle int32 [Q]; head int64 [4], the head of devring.py.
    Row head[0] % window <- per layer MATCH_LOG_FIELDS summed over the images (include/s2f.h "match log": `cost` is the bit pattern
    of an fp64 sum in a prescribed order) and per query the images in which the LAST layer matched it; idle counts the rows in a row a
    query was matched in none, the first to reach `patience` is latched in head[1]; head[0] += 1.  Two launches on the current stream,
    no synchronisation, capturable; cost, cls and row_class are only read.  HIP only: CPU tensors raise."""
    for name, t in (("cost", cost), ("cls", cls)):
        if t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous():
            raise ValueError(f"match_log_append: {name} is a contiguous fp32 [L, B, Q, K{'+1' if name == 'cls' else ''}]")
    L, B, Q, K = cost.shape
    if tuple(cls.shape) != (L, B, Q, K + 1):
        raise ValueError(f"match_log_append: cls {tuple(cls.shape)} beside cost {tuple(cost.shape)}: [{L}, {B}, {Q}, {K + 1}] expected")
    if not (1 <= L <= MATCH_LOG_MAX_LAYERS and 1 <= B <= 65535 and 1 <= Q <= LSA_MAX_QUERIES and 1 <= K <= LSA_MAX_CLASSES):
        raise ValueError(f"match_log_append: L {L} (1 .. {MATCH_LOG_MAX_LAYERS}), B {B} (1 .. 65535), Q {Q} (1 .. {LSA_MAX_QUERIES}), "
                         f"K {K} (1 .. {LSA_MAX_CLASSES})")
    words = match_log_row_words(L, Q)
    for name, t, dtype, shape in (("row_class", row_class, torch.int32, (B, L * Q)), ("partials", partials, torch.int64, (L, B, 6)),
                                  ("usage", usage, torch.int32, (B, Q)), ("idle", idle, torch.int32, (Q,)),
                                  ("head", head, torch.int64, (4,))):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"match_log_append: {name} is a contiguous {dtype} {list(shape)}, got {t.dtype} {list(t.shape)}")
    if ring.dtype != torch.int64 or ring.dim() != 2 or ring.shape[1] != words or not ring.is_contiguous():
        raise ValueError(f"match_log_append: ring is a contiguous int64 [window, {words}]")
    if any(t.device != cost.device for t in (cls, row_class, partials, usage, ring, idle, head)):
        raise RuntimeError("match_log_append: every tensor lives on one device")
    window, patience = ring.shape[0], int(patience)
    if window < 1 or patience < 1:
        raise ValueError(f"match_log_append: a ring of {window} rows, patience {patience}: each is at least 1")
    if not cost.is_cuda:
        raise RuntimeError("match_log_append: the match log is two HIP launches of the captured step; there is no CPU route")
    s = _stream()
    check(lib.s2f_match_log_partials(_ptr(cost), _ptr(cls), _ptr(row_class), L, B, Q, K, _ptr(partials), _ptr(usage), s),
          "s2f_match_log_partials")
    check(lib.s2f_match_log_rows(_ptr(partials), _ptr(usage), L, B, Q, _ptr(ring), window, _ptr(idle), patience, _ptr(head), s),
          "s2f_match_log_rows")
    return ring


__all__ = ["MATCH_LOG_MAX_LAYERS", "MATCH_LOG_FIELDS", "match_log_row_words", "match_log_append"]
