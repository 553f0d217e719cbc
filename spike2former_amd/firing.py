"""Firing-count instrumentation: the counterpart of tools/cal_firing_num.py:138-174, 203-225, 272-285.

The reference registers a forward hook on every Q_IFNode and accumulates mean(output * quant) / test_num per module
name.  Here each neuron's kernel launch adds {sum of integer counts, number of non-zero counts} into a 2-word device
counter (wave-level reduction inside s2f_lif_fwd), so recording costs no extra pass over the activations."""
import collections
import json
from collections import OrderedDict

import numpy as np
import torch

from . import ops
from .devring import DeviceRing, latch, unwrap
from .neuron import LIFNode, Q_IFNode


class FiringRecorder:
    def __init__(self, model, quant=8):
        self.model, self.quant = model, quant
        self.nodes = OrderedDict((n, m) for n, m in model.named_modules() if isinstance(m, Q_IFNode))
        self.table = OrderedDict()
        self.nonzero = OrderedDict()
        self.num_images = 0

    def __enter__(self):
        dev = next(self.model.parameters()).device
        for m in self.nodes.values():
            m.stats = ops.new_stats(dev)
            m.stats_elems = 0
        return self

    def __exit__(self, *exc):
        for m in self.nodes.values():
            m.stats = None
        return False

    def collect(self):
        """Call after each forward: folds this forward's counters into the running table (one D2H copy)."""
        names = [n for n, m in self.nodes.items() if m.stats_elems > 0]
        if not names:
            return
        st = torch.stack([ops.read_stats(self.nodes[n].stats) for n in names]).cpu()
        for i, n in enumerate(names):
            m = self.nodes[n]
            rate = float(st[i, 0]) / m.stats_elems * (self.quant / m.D)     # == mean(output * quant)
            self.table[n] = self.table.get(n, 0.0) + rate
            self.nonzero[n] = self.nonzero.get(n, 0.0) + float(st[i, 1]) / m.stats_elems
            m.stats.zero_()
            m.stats_elems = 0
        self.num_images += 1

    def result(self, test_num=None):
        k = test_num or max(self.num_images, 1)
        return {"t0": OrderedDict((n, v / k) for n, v in self.table.items())}

    def to_json(self, test_num=None):
        return json.dumps(self.result(test_num))

    def to_csv(self, path, test_num=None):
        """Same shape as the reference's fr_rate.csv: index = module name, one column 'T' (cal_firing_num.py:272-285)."""
        with open(path, "w") as f:
            f.write(",T\n")
            for n, v in self.result(test_num)["t0"].items():
                f.write(f"{n},{v}\n")


class FiringRead(collections.namedtuple("FiringRead", "names sums elems count silent first_dead scale")):
    """What `FiringLog.read()` returns.  names: the neurons, in `named_modules()` order; sums: int64 [rows, n, 2] = {sum of counts,
    non-zero counts} of the last min(count, window) rows, oldest first; elems: int64 [n], the elements each neuron fires over in
    one forward (0: not watched); count: rows appended so far; silent: int32 [n], the rows in a row each neuron has now been
    silent for (-1: not watched); first_dead: (row, name) of the first neuron whose streak reached the log's patience, or None;
    scale: quant / D per neuron."""
    __slots__ = ()

    def _per_elem(self, k):
        watched = self.elems > 0
        out = np.full(self.sums.shape[:2], np.nan)
        out[:, watched] = self.sums[:, watched, k] / self.elems[watched]
        return out

    def rates(self):
        """float64 [rows, n]: mean(output * quant) of every neuron in every row (cal_firing_num.py:140-160; FiringRecorder's
        number); NaN for a neuron that is not watched"""
        return self._per_elem(0) * self.scale

    def nonzero(self):
        """float64 [rows, n]: the share of elements with a non-zero count; NaN for a neuron that is not watched"""
        return self._per_elem(1)


class FiringLog(DeviceRing):
    """Firing counters of every neuron for EVERY iteration of a captured step, without a host stop: the counters of all neurons
    are slices of one allocation, `append()` is one launch (ops.firing_log_append) that adds each neuron's contention slots up,
    writes the pair into the next row of a devring.DeviceRing (int64 [window, n, 2]), clears the counters and keeps a streak of
    silent rows per neuron (the state words), latching in head[1] the first neuron that stayed silent for `patience` rows.

        firing = FiringLog(model, window=50)
        step = GraphedHungarianStep(..., firing=firing)        # attach, measure, append recorded as the step's last launch
    or around eager forwards (a validation loop):
        firing.attach(); firing.measure(lambda: model(x0)); firing.clear()
        for x in images: model(x); firing.append()
        read = firing.read(); firing.detach()

    Attached counters change which kernels run: the memoised, pre-fired and fused-neuron routes test `stats is None` and step aside,
    as they do for `FiringRecorder` (which stays the tool for an evaluation table in the reference's format)."""
    HEAD, prefix = (0, -1, 0, 0), "firing"

    def __init__(self, model, window=64, patience=200, quant=8, device=None):
        if window < 1 or patience < 1:
            raise ValueError(f"FiringLog: window {window} and patience {patience} are at least 1")
        self.model, self.window, self.patience, self.quant = model, int(window), int(patience), quant
        self.nodes = OrderedDict((n, m) for n, m in model.named_modules() if isinstance(m, (Q_IFNode, LIFNode)))
        if not self.nodes:
            raise ValueError("FiringLog: the model has no Q_IFNode or LIFNode")
        if device is None:
            p = next(model.parameters(), None)
            device = p.device if p is not None else "cpu"
        n = self.n = len(self.nodes)
        self.names = list(self.nodes)
        state, ring = self._allocate((n + 1) // 2, self.window * n * 2, device)          # (silent: padded to whole words)
        self.silent, self.ring = state.view(torch.int32)[:n], ring.view(self.window, n, 2)
        self.counters = torch.zeros(n, ops.STAT_SLOTS, 2, dtype=torch.int64, device=self.device)
        self.clear()
        self.elems = torch.zeros(n, dtype=torch.int64)          # (host) elements per neuron in one forward; 0: not watched
        self.scale = np.array([quant / m.D for m in self.nodes.values()], np.float64)
        self.attached = False

    # ------------------------------------------------------------------------------------------------ the neurons' counters
    def attach(self):
        """every neuron's `stats` <- its slice of the counters.  Raises when a neuron already counts into something (a live
        FiringRecorder, another FiringLog)."""
        if self.attached:
            return
        busy = [n for n, m in self.nodes.items() if m.stats is not None]
        if busy:
            raise RuntimeError(f"FiringLog.attach: {len(busy)} neurons already record firing (a live FiringRecorder or another "
                               f"FiringLog), first {busy[0]!r}")
        for i, m in enumerate(self.nodes.values()):
            m.stats = self.counters[i]
        self.attached = True

    def detach(self):
        if self.attached:
            for m in self.nodes.values():
                m.stats = None
        self.attached = False

    def measure(self, forward):
        """Run `forward()` once and take from it how many elements each neuron fires over (`elems`): a neuron the forward never
        runs is not watched (silent = -1), every other starts with a streak of 0.  Not under capture; what the forward counted
        stays in the counters until `clear()` or the next `append()`."""
        if not self.attached:
            raise RuntimeError("FiringLog.measure before attach")
        for m in self.nodes.values():
            m.stats_elems = 0
        forward()
        self.elems = torch.tensor([int(m.stats_elems) for m in self.nodes.values()], dtype=torch.int64)
        self.silent.copy_(torch.where(self.elems > 0, 0, -1).to(torch.int32))

    def clear(self):
        """counters, ring and head as new; the streaks of the watched neurons to 0.  Not under capture."""
        super().clear()
        self.counters.zero_()
        self.silent.clamp_(max=0)          # (-1 stays)

    # ------------------------------------------------------------------------------------------------ rows
    def append(self):
        """one row: ONE launch on the current stream, capturable"""
        ops.firing_log_append(self.counters, self.ring, self.silent, self.head, self.patience)

    def read(self):
        """-> FiringRead.  One `fetch()`."""
        words = self.fetch()
        n, pad, count = self.n, (self.n + 1) // 2, int(words[0])
        sums = unwrap(words[4 + pad:].reshape(self.window, n, 2), count, self.window)
        silent = words[4:4 + pad].view(np.int32)[:n].copy()
        return FiringRead(list(self.names), sums, self.elems.numpy().copy(), count, silent, latch(words[1], self.names), self.scale)

    def report(self, n, since, iteration_of=int):
        """runner.LoggerHook's share of the log line of iteration `n`, over the rows since the line of iteration `since` -> (keys for
        the line and scalars.json, the line of firing.jsonl or None, a warning or None).  Keys: the mean rate over the watched neurons,
        the neuron with the lowest mean rate, the watched neurons that did not fire in the last row.  firing.jsonl: every watched
        neuron's mean rate and non-zero share.  Warning: the latched first dead neuron and the iteration its streak reached `patience`."""
        read = self.read()
        k = min(n - since, len(read.sums), read.count)
        watched = read.elems > 0
        keys, items, warning = {}, None, None
        if k > 0 and watched.any():
            rates, nz = read.rates()[-k:].mean(0), read.nonzero()[-k:].mean(0)
            low = int(np.flatnonzero(watched)[np.argmin(rates[watched])])
            keys["firing/mean"] = float(rates[watched].mean())
            keys["firing/min"], keys["firing/min_name"] = float(rates[low]), read.names[low]
            keys["firing/silent"] = int((read.silent[watched] >= 1).sum())
            idx = np.flatnonzero(watched)
            items = dict(iter=n, rows=k, rates={read.names[i]: float(rates[i]) for i in idx},
                         nonzero={read.names[i]: float(nz[i]) for i in idx})
        if read.first_dead is not None:
            row, name = read.first_dead
            warning = f"neuron {name} has not fired for {self.patience} iterations, up to iteration {iteration_of(self.base + row + 1)}"
        return keys, items, warning
