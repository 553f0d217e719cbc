"""Per-parameter gradient, weight and update norms of EVERY iteration, from inside the step: where the gradient goes.

A spiking network trained through a surrogate window fails tensor by tensor -- a block whose pre-activations leave the window gets an
exactly-zero gradient and never recovers; one exploding tensor under `clip_grad(max_norm=0.01)` scales every other update down; a
non-finite term starts in one tensor.  The usual way to see any of it is ~1 000 `.norm()` calls and a host stop per iteration, which
`train.FlatAdamW` and the captured step exist to avoid.  `GradLog` is two launches behind `s2f_adamw_step` (csrc/gradlog.hip: a
segmented reduction over the optimizer's flat buffers and its pointer table) into a ring on the device, and one copy per log line.

    optim = FlatAdamW(model, red, ..., grad_log=GradLog)          # or: optim.attach_grad_log(GradLog(optim, window=50))
    step = GraphedHungarianStep(..., optimizer=optim, log=TrainLog(window=50))     # the rows are captured with the update
    ...
    read = optim.grad_log.read(); read.grad_norm[-1]; read.first_stalled

Not logged: per-element histograms; the ring and the streaks are in no checkpoint (a resumed run starts them afresh)."""
import collections

import numpy as np
import torch

from . import ops
from .devring import DeviceRing, latch, unwrap


class GradRead(collections.namedtuple("GradRead", "names cols count streak first_stalled first_nonfinite")):
    """What `GradLog.read()` returns, over the rows appended since the last read (at most the ring's window of them, oldest first).
    names: the parameters, in the optimizer's order; cols: int64 [rows, n, 8], the rows as the kernels wrote them (include/s2f.h
    "gradient log": columns 0-3 are doubles by bit pattern); count: rows appended so far; streak: int32 [n, 2] = the rows in a row each
    parameter's gradient has now been {all zero, non-finite somewhere}; first_stalled: (row, name) of the first parameter whose
    gradient stayed all zero for the log's patience, or None; first_nonfinite: (row, name) of the first parameter with a non-finite
    gradient element, or None.  Every array below is float64 [rows, n] unless it says otherwise."""
    __slots__ = ()

    @classmethod
    def from_buffer(cls, buf, names, window, last=0):
        """buf: the log's allocation on the host, int64 [4 + n + window * n * 8] = head, streaks, ring; `last`: the row count at the
        previous read."""
        buf = np.asarray(buf, dtype=np.int64)
        n = len(names)
        count = int(buf[0])
        cols = unwrap(buf[4 + n:].reshape(window, n, 8), count, window, last)
        streak = buf[4:4 + n].copy().view(np.int32).reshape(n, 2)
        return cls(list(names), cols, count, streak, latch(buf[1], names), latch(buf[3], names))

    def _f(self, c):
        return np.ascontiguousarray(self.cols[:, :, c]).view(np.float64)

    @property
    def grad_sq(self):
        return self._f(0)

    @property
    def weight_sq(self):
        return self._f(1)

    @property
    def update_sq(self):
        return self._f(2)

    @property
    def grad_norm(self):
        return np.sqrt(self._f(0))

    @property
    def weight_norm(self):
        return np.sqrt(self._f(1))

    @property
    def update_ratio(self):
        """|u| / |p|: how far the Adam step (without the decay term) moved the tensor, relative to its size; 0 where |p| is 0"""
        p, u = self._f(1), self._f(2)
        return np.sqrt(np.divide(u, p, out=np.zeros_like(u), where=p > 0))

    @property
    def grad_max(self):
        return self._f(3)

    @property
    def numel(self):
        """int64 [rows, n]"""
        return self.cols[:, :, 7]

    @property
    def zero_share(self):
        """the share of elements whose gradient is exactly 0"""
        z, n = self.cols[:, :, 4].astype(np.float64), self.cols[:, :, 7].astype(np.float64)
        return np.divide(z, n, out=np.zeros_like(z), where=n > 0)

    @property
    def nonfinite(self):
        """int64 [rows, n, 2]: non-finite elements of {g, p or u}"""
        return self.cols[:, :, 5:7]

    @property
    def total_grad_norm(self):
        """float64 [rows]: the norm of the whole gradient, over its finite elements (FlatAdamW.grad_norm, summed another way)"""
        return np.sqrt(self._f(0).sum(1))


class GradLog(DeviceRing):
    """A devring.DeviceRing of the last `window` updates' per-parameter rows (int64 [window, n, 8]; state words: the streaks, int32
    [n, 2]; head[1] latches the first stalled parameter, head[3] the first non-finite gradient) over a `train.FlatAdamW`.  `append()`
    is two launches (ops.grad_log_append) that only read the optimizer's buffers and the parameters; `FlatAdamW.step()` calls it
    directly behind the update once the log is attached, so a row is added wherever `step()` runs: captured with the step at world
    size 1, eager behind the all-reduce at N > 1.  Without a log the step launches what it always did."""
    HEAD, prefix = (0, -1, 0, -1), "grad"

    def __init__(self, optimizer, window=64, patience=200):
        if window < 1 or patience < 1:
            raise ValueError(f"GradLog: window {window} and patience {patience} are at least 1")
        self.optimizer, self.window, self.patience = optimizer, int(window), int(patience)
        self.names = [g["name"] for g in optimizer.param_groups]
        n = self.n = len(self.names)
        if n < 1:
            raise ValueError("GradLog: the optimizer has no parameters")
        state, ring = self._allocate(n, self.window * n * 8, optimizer.slots.device)
        self.streak, self.ring = state.view(torch.int32).view(n, 2), ring.view(self.window, n, 8)
        self.rebuild()          # (-> clear(): `_last`, the row count at the last read, is 0)

    def rebuild(self):
        """the span table over the optimizer's CURRENT slot table (FlatAdamW.rebuild() re-lays the buffers and may reorder the
        parameters: rows and streaks of the old order mean nothing in the new one, so the log starts afresh).  Not under capture."""
        self._slots = self.optimizer.slots
        self.names = [g["name"] for g in self.optimizer.param_groups]
        if len(self.names) != self.n:
            raise RuntimeError(f"GradLog: built over {self.n} parameters, the optimizer now has {len(self.names)}")
        self.spans = ops.grad_log_table(self._slots)
        self.partials = torch.zeros(self.spans.shape[0], 8, dtype=torch.int64, device=self.device)
        self.clear()

    def clear(self):
        """ring, streaks and head as new.  Not under capture."""
        super().clear()
        self.streak.zero_()
        self._last = 0

    def append(self):
        """one row: TWO launches on the current stream, capturable.  Call it behind the optimizer's update (FlatAdamW.step does)."""
        opt = self.optimizer
        if opt.slots is not self._slots:
            self.rebuild()
        ops.grad_log_append(opt.slots, self.spans, opt.hyper, opt.state, opt.red.flat, opt.exp_avg, opt.exp_avg_sq, self.partials,
                            self.ring, self.streak, self.head, opt.eps, self.patience)

    def read(self, consume=True):
        """-> GradRead over the rows since the last read.  One `fetch()`.  `consume=False`: the next read sees these rows again."""
        read = GradRead.from_buffer(self.fetch(), self.names, self.window, self._last)
        if consume:
            self._last = read.count
        return read

    def report(self, n, since, iteration_of):
        """runner.LoggerHook's share of a log line, over the rows since the last read -> (keys for the line and scalars.json, the line
        of grad.jsonl or None, a warning or None).  Keys: the parameter with the lowest mean gradient norm, the one holding the largest
        share of sum g^2 (the one the clip is reacting to), the largest mean |u| / |p|, the share of gradient elements that are exactly
        0, the parameters whose gradient was all zero in the last row.  grad.jsonl: every parameter's figures, under the iteration
        of the last row (`iteration_of` a row number: the rows count updates).  Warning: the latched first stalled parameter."""
        read = self.read()
        k = len(read.cols)
        keys, items, warning = {}, None, None
        if k > 0:
            sq = read.grad_sq.sum(0)
            norm, ratio = read.grad_norm.mean(0), read.update_ratio.mean(0)
            low, top, far = int(np.argmin(norm)), int(np.argmax(sq)), int(np.argmax(ratio))
            elems = float(read.numel.sum())
            keys["grad/min"], keys["grad/min_name"] = float(norm[low]), read.names[low]
            keys["grad/max_share"], keys["grad/max_name"] = float(sq[top] / sq.sum()) if sq.sum() > 0 else 0.0, read.names[top]
            keys["grad/update_ratio_max"], keys["grad/update_ratio_max_name"] = float(ratio[far]), read.names[far]
            keys["grad/zero_share"] = float(read.cols[:, :, 4].sum()) / elems if elems else 0.0
            keys["grad/stalled"] = int((read.streak[:, 0] >= 1).sum())
            per = dict(grad_norm=norm, weight_norm=read.weight_norm.mean(0), update_ratio=ratio, grad_max=read.grad_max.max(0),
                       zero_share=read.zero_share.mean(0))
            items = dict(iter=iteration_of(self.base + read.count), rows=k,
                         **{key: {name: float(v) for name, v in zip(read.names, vals)} for key, vals in per.items()})
        if read.first_stalled is not None:
            row, name = read.first_stalled
            warning = (f"parameter {name} has had an all-zero gradient for {self.patience} iterations, up to iteration "
                       f"{iteration_of(self.base + row + 1)}")
        return keys, items, warning
