"""What the Hungarian assignment did in EVERY iteration, from inside the step: the one part of a MaskFormer-style trainer that had no
figure at all.

With `GraphedHungarianStep(assign="device")` the assignment is a kernel of the step (csrc/lsa.hip) and its tables never reach the
host.  `MatchLog` is two read-only launches behind it (csrc/matchlog.hip) into a ring, and one copy per log line:

    step = GraphedHungarianStep(..., assign="device", log=TrainLog(window=50), match_log=MatchLog(window=50, patience=500))
    ...
    read = step.match_log.read(); read.rows[-1]; read.first_idle

Per decoder layer, summed over the images of the batch (ops.MATCH_LOG_FIELDS; the rule in full: include/s2f.h "match log"):
`matched` pairs and their `cost` (an fp64 sum in a prescribed order, kept as its bit pattern: `MatchLog.costs`), the pairs whose
query is also the first arg-min of its class's cost column (`greedy`), the pairs whose class belonged to another query, or to none,
in the layer before (`moved`), the pairs whose query's first arg-max over the K+1 class logits is its target (`cls_hit`: DETR's
class_error is 100 - 100 * cls_hit / matched), and the unmatched queries whose arg-max is not the void column (`unmatched_obj`).
Per query: the images in which the LAST layer matched it (`usage`), and how many rows in a row it was matched in none (`idle`).
None of these has a counterpart in the reference, whose head logs losses only.  At world size > 1 every rank logs its own images
and rank 0's figures are the ones written; with `accumulative_counts=k` a row is an iteration (a micro-batch); the ring and the
streaks are in no checkpoint (a resumed run starts them afresh)."""
import collections

import numpy as np
import torch

from . import ops
from .devring import DeviceRing, latch, unwrap

FIELDS = ops.MATCH_LOG_FIELDS
MATCHED, COST, GREEDY, MOVED, CLS_HIT, UNMATCHED_OBJ = range(len(FIELDS))


class MatchRead(collections.namedtuple("MatchRead", "rows usage count idle first_idle")):
    """What `MatchLog.read()` returns.  rows: int64 [n, L, 6], the fields of ops.MATCH_LOG_FIELDS per decoder layer of the rows
    appended since the last read (at most the ring's window of them), oldest first -- `cost` as the bits of a double
    (`MatchLog.costs(rows)`); usage: int32 [n, Q], the images in which the last layer matched each query; count: rows appended so far;
    idle: int32 [Q], the rows in a row each query has now been matched in no image of the last layer; first_idle: (row, query) of the
    first query whose streak reached the log's patience, or None."""
    __slots__ = ()


class MatchLog(DeviceRing):
    """A devring.DeviceRing of the last `window` iterations' figures (int64 [window, 6L + ceil(Q/2)]: [L, 6] fields, then usage int32
    [Q]; state words: the idle streaks, int32 [Q]; head[1] latches the first query that `patience` iterations in a row were matched
    in no image of the last layer).  `bind(L, B, Q, K)` allocates for the step's shapes (GraphedHungarianStep does, after its shape
    probe); `append(cost, cls, row_class)` is two launches (ops.match_log_append), capturable."""
    HEAD, prefix = (0, -1), "match"

    def __init__(self, window=64, patience=500, device=None):
        if window < 1 or patience < 1:
            raise ValueError(f"MatchLog: window {window} and patience {patience} are at least 1")
        self.window, self.patience = int(window), int(patience)
        self._device = device
        self.shape = None          # until bind()

    def bind(self, L, B, Q, K, device=None):
        """the allocation for a decoder of L layers, batches of B images, Q queries and K classes: head, streaks, ring and the
        workspace of the first launch.  Everything starts afresh.  Not under capture."""
        L, B, Q, K = (int(v) for v in (L, B, Q, K))
        if not (1 <= L <= ops.MATCH_LOG_MAX_LAYERS and 1 <= B <= 65535 and 1 <= Q <= ops.LSA_MAX_QUERIES and 1 <= K <= ops.LSA_MAX_CLASSES):
            raise ValueError(f"MatchLog: L {L} (1 .. {ops.MATCH_LOG_MAX_LAYERS}), B {B} (1 .. 65535), Q {Q} (1 .. {ops.LSA_MAX_QUERIES}), "
                             f"K {K} (1 .. {ops.LSA_MAX_CLASSES})")
        if device is None:
            device = self._device if self._device is not None else ("cuda" if torch.cuda.is_available() else "cpu")
        self.shape = (L, B, Q, K)
        self.pad, self.words = (Q + 1) // 2, ops.match_log_row_words(L, Q)          # (idle, usage: padded to whole words)
        state, ring = self._allocate(self.pad, self.window * self.words, device)
        self.idle, self.ring = state.view(torch.int32)[:Q], ring.view(self.window, self.words)
        self.partials = torch.zeros(L, B, len(FIELDS), dtype=torch.int64, device=self.device)
        self.usage = torch.zeros(B, Q, dtype=torch.int32, device=self.device)
        self.clear()
        return self

    def _bound(self):
        if self.shape is None:
            raise RuntimeError("MatchLog: bind(L, B, Q, K) first (GraphedHungarianStep(match_log=...) does)")

    def clear(self):
        """ring, streaks and head as new.  Not under capture."""
        self._bound()
        super().clear()
        self.head[2:].zero_()
        self.idle.zero_()
        self._last = 0

    def rebase(self, start, unit=1):
        self._bound()
        super().rebase(start, unit)

    def append(self, cost, cls, row_class):
        """one row: TWO launches on the current stream, capturable.  cost [L, B, Q, K] (MaskFormerLoss.costs_all_classes: what the
        assignment read), cls [L, B, Q, K+1] (the head's class scores, detached here), row_class int32 [B, L*Q] (the assignment's
        table)."""
        self._bound()
        L, B, Q, K = self.shape
        if tuple(cost.shape) != (L, B, Q, K) or tuple(cls.shape) != (L, B, Q, K + 1):
            raise ValueError(f"MatchLog.append: cost {tuple(cost.shape)}, cls {tuple(cls.shape)}; bound to {(L, B, Q, K)} and "
                             f"{(L, B, Q, K + 1)}")
        ops.match_log_append(cost.detach().float().contiguous(), cls.detach().float().contiguous(), row_class, self.partials,
                             self.usage, self.ring, self.idle, self.head, self.patience)

    @staticmethod
    def costs(rows):
        """rows int64 [..., 6] -> the `cost` field as the doubles it holds, [...]"""
        return np.ascontiguousarray(rows[..., COST]).view(np.float64)

    def read(self, consume=True):
        """-> MatchRead over the rows since the last read.  One `fetch()`.  `consume=False`: the next read sees these rows again."""
        self._bound()
        words = self.fetch()
        L, _, Q, _ = self.shape
        n, count = len(FIELDS) * L, int(words[0])
        ring = unwrap(words[4 + self.pad:].reshape(self.window, self.words), count, self.window, self._last)
        rows = np.ascontiguousarray(ring[:, :n]).reshape(-1, L, len(FIELDS))
        usage = np.ascontiguousarray(ring[:, n:]).view(np.int32)[:, :Q]
        idle = words[4:4 + self.pad].copy().view(np.int32)[:Q]
        if consume:
            self._last = count
        return MatchRead(rows, usage, count, idle, latch(words[1], range(Q)))

    @staticmethod
    def _figures(t, cost, k):
        """the totals int64 [6] of one layer over k rows and their cost -> {name: figure}; a figure whose denominator is 0 is left out"""
        matched = int(t[MATCHED])
        out = {}
        if matched > 0:
            out["class_error"] = 100.0 - 100.0 * int(t[CLS_HIT]) / matched
        out["matched"] = matched / k
        if matched > 0:
            out["cost"] = float(cost) / matched
            out["greedy_share"] = int(t[GREEDY]) / matched
            out["moved_share"] = int(t[MOVED]) / matched
        out["false_pos"] = int(t[UNMATCHED_OBJ]) / k
        return out

    def report(self, n, since, iteration_of=int):
        """runner.LoggerHook's share of the log line of iteration `n`, over the rows since the last read -> (keys for the line and
        scalars.json, the line of match.jsonl or None, a warning or None).  Keys, of the LAST decoder layer: `match/class_error` =
        100 - 100 * cls_hit / matched (DETR's), `match/matched` (pairs per iteration), `match/cost` (per matched pair),
        `match/greedy_share`, `match/moved_share` (of the matched pairs), `match/false_pos` (unmatched queries per iteration whose
        arg-max is an object), `match/queries_used` (queries matched at least once in these rows), `match/idle_max` (the longest
        current streak).  A key whose denominator is 0 is left out.  match.jsonl: the same figures for every layer and the usage
        summed over the rows, under the iteration of the last row.  Warning: the latched query and the iteration its streak reached
        `patience`."""
        read = self.read()
        k = len(read.rows)
        keys, items, warning = {}, None, None
        if k > 0:
            total = read.rows.sum(0)          # int64 [L, 6]  (the cost column: summed below, as doubles)
            cost = self.costs(read.rows).sum(0)          # fp64 [L]
            layers = [self._figures(t, c, k) for t, c in zip(total, cost)]
            used = read.usage.sum(0, dtype=np.int64)
            keys = {f"match/{name}": v for name, v in layers[-1].items()}
            keys["match/queries_used"] = int((used > 0).sum())
            keys["match/idle_max"] = int(read.idle.max())
            items = dict(iter=iteration_of(self.base + read.count), rows=k, layers=layers, usage=[int(u) for u in used])
        if read.first_idle is not None:
            row, q = read.first_idle
            warning = (f"query {q} has been matched in no image of the last decoder layer for {self.patience} iterations in a row, "
                       f"up to iteration {iteration_of(self.base + row + 1)}")
        return keys, items, warning
