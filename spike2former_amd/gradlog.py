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
        k = max(0, min(count - last, window))
        ring = buf[4 + n:].reshape(window, n, 8)
        cols = np.stack([ring[(count - k + i) % window] for i in range(k)]) if k else np.zeros((0, n, 8), np.int64)
        streak = buf[4:4 + n].copy().view(np.int32).reshape(n, 2)

        def event(word):
            return None if word < 0 else (int(word >> 32), names[int(word & 0xffffffff)])
        return cls(list(names), cols.copy(), count, streak, event(int(buf[1])), event(int(buf[3])))

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


class GradLog:
    """A ring of the last `window` iterations' per-parameter rows on the device, over a `train.FlatAdamW`.  `append()` is two launches
    (ops.grad_log_append, capturable) that only read the optimizer's buffers and the parameters; `FlatAdamW.step()` calls it directly
    behind the update once the log is attached, so a row is added wherever `step()` runs: captured with the step at world size 1, eager
    behind the all-reduce at N > 1.  `read()` is one device-to-host copy.  Without a log the step launches what it always did."""

    def __init__(self, optimizer, window=64, patience=200):
        if window < 1 or patience < 1:
            raise ValueError(f"GradLog: window {window} and patience {patience} are at least 1")
        self.optimizer, self.window, self.patience = optimizer, int(window), int(patience)
        self.names = [g["name"] for g in optimizer.param_groups]
        n = self.n = len(self.names)
        if n < 1:
            raise ValueError("GradLog: the optimizer has no parameters")
        self.device = optimizer.slots.device
        # head (int64 [4]), the streaks (int32 [n, 2]: n whole words) and the ring in ONE allocation: read() is one copy
        self._buf = torch.zeros(4 + n + self.window * n * 8, dtype=torch.int64, device=self.device)
        self.head = self._buf[:4]
        self.streak = self._buf[4:4 + n].view(torch.int32).view(n, 2)
        self.ring = self._buf[4 + n:].view(self.window, n, 8)
        self._host = torch.zeros_like(self._buf, device="cpu")
        self._event = None
        if self.device.type == "cuda":
            self._host = self._host.pin_memory()
            self._event = torch.cuda.Event()
        self.base = 0          # the iterations that ran before row 0 (a resumed run)
        self._last = 0         # the row count at the last read
        self._slots = None
        self.rebuild()

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
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("GradLog.clear under capture")
        self._buf.zero_()
        self.head.copy_(torch.tensor([0, -1, 0, -1], dtype=torch.int64))
        self._last = 0

    def append(self):
        """one row: TWO launches on the current stream, capturable.  Call it behind the optimizer's update (FlatAdamW.step does)."""
        opt = self.optimizer
        if opt.slots is not self._slots:
            self.rebuild()
        ops.grad_log_append(opt.slots, self.spans, opt.hyper, opt.state, opt.red.flat, opt.exp_avg, opt.exp_avg_sq, self.partials,
                            self.ring, self.streak, self.head, opt.eps, self.patience)

    def read(self, consume=True):
        """-> GradRead over the rows since the last read.  One device-to-host copy on the current stream, and a wait for that copy.
        `consume=False`: the next read sees these rows again."""
        if self._event is not None:
            self._host.copy_(self._buf, non_blocking=True)
            self._event.record()
            self._event.synchronize()
        else:
            self._host.copy_(self._buf)
        read = GradRead.from_buffer(self._host.numpy(), self.names, self.window, self._last)
        if consume:
            self._last = read.count
        return read
