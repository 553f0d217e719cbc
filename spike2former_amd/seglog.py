"""Train-crop accuracy and mIoU of EVERY iteration, from inside the step: whether the model segments what it is trained on.

mmseg's BaseDecodeHead logs `decode.acc_seg` with every loss; the reference's MaskFormerHead logs losses only, and the loop's own
validation mIoU arrives every `val_interval` iterations.  Set beside it, the figure of the training crops separates "not learning"
from "not generalising".  The captured step already holds what the score needs on the device -- the decoder's class scores and mask
logits, and the label map -- so `SegLog` is two launches at the end of the step (csrc/seglog.hip) into a ring, and one copy per log
line:

    step = GraphedHungarianStep(..., log=TrainLog(window=50), seg_log=SegLog(150, window=50))
    ...
    read = step.seg_log.read(); read.areas[-1]; read.first_missed

The prediction is MaskFormerHead.predict's -- softmax over the classes without the void column, sigmoid of the masks, their product
summed over the queries, the arg-max -- with ONE stated deviation: predict up-samples the masks to the picture first, the log scores
at the MASK resolution against the labels the matching costs see (seg[:, ::2, ::2]).  A training diagnostic, not the validation
metric.  At world size > 1 every rank scores its own crops and rank 0's figures are the ones written (the rule runner.LoggerHook
states for every ring); with `accumulative_counts=k` a row is an iteration (a micro-batch).  Not logged: a confusion matrix of the
crops; the ring and the streaks are in no checkpoint (a resumed run starts them afresh)."""
import collections

import numpy as np
import torch

from . import ops
from .devring import DeviceRing, latch, unwrap
from .metrics import IoUMetric


class SegRead(collections.namedtuple("SegRead", "areas count streak first_missed")):
    """What `SegLog.read()` returns.  areas: int64 [rows, L', 3, K] = {intersect, pred, label} per scored layer and class, the rows
    appended since the last read (at most the ring's window of them), oldest first; count: rows appended so far; streak: int32 [K],
    the rows in a row each class has now been labelled without one correctly predicted pixel (the last scored layer's); first_missed:
    (row, class index) of the first class whose streak reached the log's patience, or None."""
    __slots__ = ()


class SegLog(DeviceRing):
    """A devring.DeviceRing of the last `window` iterations' areas (int64 [window, L', 3, K]; state words: the streaks, int32 [K];
    head[1] latches the first class that was labelled `patience` iterations in a row without a correctly predicted pixel).
    layers: "last" scores the last decoder layer (L' = 1), "all" every layer (L' = L; the streaks and the latch follow the last one),
    or a list of layer indices; classes: names for the report.  `bind(L, B, Q, h, w)` allocates for the step's shapes
    (GraphedHungarianStep does, after its shape probe); `append(cls, masks, seg_u8)` is two launches (ops.seg_log_append), capturable."""
    HEAD, prefix = (0, -1), "seg"

    def __init__(self, num_classes, window=64, patience=500, layers="last", classes=None, device=None):
        if window < 1 or patience < 1:
            raise ValueError(f"SegLog: window {window} and patience {patience} are at least 1")
        if not 1 <= int(num_classes) <= ops.SEG_LOG_MAX_CLASSES:
            raise ValueError(f"SegLog: {num_classes} classes outside 1 .. {ops.SEG_LOG_MAX_CLASSES} (255 is the ignored label)")
        if not (layers in ("last", "all") if isinstance(layers, str) else len(list(layers)) >= 1):
            raise ValueError(f"SegLog: layers is 'last', 'all' or a list of layer indices, got {layers!r}")
        self.K, self.window, self.patience = int(num_classes), int(window), int(patience)
        self.layers_spec = layers if isinstance(layers, str) else [int(i) for i in layers]
        self.classes = [str(c) for c in classes] if classes is not None else None
        if self.classes is not None and len(self.classes) != self.K:
            raise ValueError(f"SegLog: {len(self.classes)} class names for {self.K} classes")
        self._device = device
        self.layers = self.shape = None          # until bind()

    def bind(self, L, B, Q, h, w, device=None):
        """the scored layers of a decoder of L layers, and the allocation for batches of B images, Q queries and h x w mask maps:
        head, streaks, ring and the workspace of the first launch.  Everything starts afresh.  Not under capture."""
        L, B, Q, h, w = (int(v) for v in (L, B, Q, h, w))
        spec = self.layers_spec
        layers = [L - 1] if spec == "last" else list(range(L)) if spec == "all" else [i + L if i < 0 else i for i in spec]
        if not 1 <= len(layers) <= ops.SEG_LOG_MAX_LAYERS or any(not 0 <= i < L for i in layers):
            raise ValueError(f"SegLog: layers {layers} of a decoder of {L}: 1 .. {ops.SEG_LOG_MAX_LAYERS} of them, each in 0 .. {L - 1}")
        if B < 1 or Q < 1 or w % 2 or (h * w) % 4 or h < 1 or w < 1:
            raise ValueError(f"SegLog: B {B}, Q {Q} are at least 1; a {h} x {w} mask map needs w even and h*w a multiple of 4")
        if device is None:
            device = self._device if self._device is not None else ("cuda" if torch.cuda.is_available() else "cpu")
        self.layers, self.shape, n, K = layers, (L, B, Q, h, w), len(layers), self.K
        self.pad = (K + 1) // 2          # (streak: padded to whole words)
        state, ring = self._allocate(self.pad, self.window * n * 3 * K, device)
        self.streak, self.ring = state.view(torch.int32)[:K], ring.view(self.window, n, 3, K)
        self.partials = torch.zeros(n * B * ops.seg_log_tiles(h, w), 3, K, dtype=torch.int32, device=self.device)
        self.clear()
        return self

    def _bound(self):
        if self.layers is None:
            raise RuntimeError("SegLog: bind(L, B, Q, h, w) first (GraphedHungarianStep(seg_log=...) does)")

    def clear(self):
        """ring, streaks and head as new.  Not under capture."""
        self._bound()
        super().clear()
        self.head[2:].zero_()
        self.streak.zero_()
        self._last = 0

    def rebase(self, start, unit=1):
        self._bound()
        super().rebase(start, unit)

    def append(self, cls, masks, seg_u8):
        """one row: TWO launches on the current stream, capturable.  cls [L, B, Q, K+1], masks [L, B, Q, h, w] (a view of the head's
        [B, L*Q, h*w] buffer: MaskFormerHead's outputs, detached here), seg_u8 [B, 2h, 2w] (loss.MaskFormerLoss.seg_as_u8)."""
        self._bound()
        L, B, Q, h, w = self.shape
        if tuple(cls.shape) != (L, B, Q, self.K + 1) or tuple(masks.shape) != (L, B, Q, h, w):
            raise ValueError(f"SegLog.append: cls {tuple(cls.shape)}, masks {tuple(masks.shape)}; bound to {(L, B, Q, self.K + 1)} and "
                             f"{(L, B, Q, h, w)}")
        pred = masks.detach().permute(1, 0, 2, 3, 4).reshape(B, L * Q, h * w).float()          # a view of the head's buffer
        ops.seg_log_append(pred.contiguous(), cls.detach().float().contiguous(), seg_u8, self.layers, self.partials, self.ring,
                           self.streak, self.head, self.patience)

    def read(self, consume=True):
        """-> SegRead over the rows since the last read.  One `fetch()`.  `consume=False`: the next read sees these rows again."""
        self._bound()
        words = self.fetch()
        n, K, count = len(self.layers), self.K, int(words[0])
        areas = unwrap(words[4 + self.pad:].reshape(self.window, n, 3, K), count, self.window, self._last)
        streak = words[4:4 + self.pad].copy().view(np.int32)[:K]
        if consume:
            self._last = count
        return SegRead(areas, count, streak, latch(words[1], range(K)))

    def name(self, c):
        return self.classes[c] if self.classes is not None else str(c)

    def report(self, n, since, iteration_of=int):
        """runner.LoggerHook's share of the log line of iteration `n`, over the rows since the last read -> (keys for the line and
        scalars.json, the line of seg.jsonl or None, a warning or None).  The areas are summed over the rows and handed to
        IoUMetric.total_area_to_metrics.  Keys: `decode.acc_seg` = aAcc in percent (mmseg's name for it), `train/mIoU` and `train/mAcc`
        = round(nanmean * 100, 2) over the classes labelled in these rows, `train/classes` = how many those are; with more than one
        scored layer `decode.d{i}.acc_seg` of every earlier layer i.  seg.jsonl: per labelled class {IoU, Acc, pixels}, under the
        iteration of the last row.  Warning: the latched class and the iteration its streak reached `patience`."""
        read = self.read()
        k = len(read.areas)
        keys, items, warning = {}, None, None
        if k > 0:
            total = read.areas.sum(0)          # int64 [L', 3, K]
            metrics = [IoUMetric.total_area_to_metrics(t[0], t[1] + t[2] - t[0], t[1], t[2]) for t in total]
            last, m = total[-1], metrics[-1]
            labelled = np.flatnonzero(last[2] > 0)
            if labelled.size:
                keys["decode.acc_seg"] = float(m["aAcc"] * 100)
                keys["train/mIoU"] = round(float(np.nanmean(m["IoU"][labelled])) * 100, 2)
                keys["train/mAcc"] = round(float(np.nanmean(m["Acc"][labelled])) * 100, 2)
            keys["train/classes"] = int(labelled.size)          # (0: every pixel of these rows was ignored; no figure to give)
            if labelled.size:
                for i, t, mi in zip(self.layers[:-1], total, metrics):
                    if t[2].sum() > 0:
                        keys[f"decode.d{i}.acc_seg"] = float(mi["aAcc"] * 100)
                items = dict(iter=iteration_of(self.base + read.count), rows=k,
                             classes={self.name(c): dict(IoU=float(m["IoU"][c]), Acc=float(m["Acc"][c]), pixels=int(last[2][c]))
                                      for c in labelled})
        if read.first_missed is not None:
            row, c = read.first_missed
            warning = (f"class {self.name(c)} has been labelled for {self.patience} iterations in a row without one correctly "
                       f"predicted pixel, up to iteration {iteration_of(self.base + row + 1)}")
        return keys, items, warning
