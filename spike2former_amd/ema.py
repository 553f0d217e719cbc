"""An exponential moving average of the weights, kept on the device inside the captured step -- mmengine's

    custom_hooks = [dict(type='EMAHook', ema_type='ExpMomentumEMA', momentum=0.0002, gamma=2000, begin_iter=...)]

for a step that is one hipGraph with no ATen in the update.  `WeightEMA` is a second flat copy of the parameters in the layout of
`train.FlatAdamW`'s moments; `update()` is ONE launch behind s2f_adamw_step (csrc/ema.hip), recorded by `FlatAdamW.step()` and so
captured with the update; `swap()` / `restore()` exchange the averaged and the training weights in place, one launch each, so that
validation (eager or through `GraphedPredict` graphs: no pointer moves) runs on the average; `runner.TrainState` writes both into the
checkpoint by mmengine's EMAHook rule.

mmengine (0.8.4) is not part of the reference tree; the semantics are restated from its published behaviour and their parity is
UNPINNED:

    ExponentialMovingAverage.avg_func     avg.lerp_(src, momentum)
    ExpMomentumEMA.avg_func               momentum_c = (1 - momentum) * exp(-(1 + c) / gamma) + momentum,  c = `steps`
    BaseAveragedModel.update_parameters   steps == 0: copy;  steps % interval == 0: avg_func;  steps += 1 on every call
    EMAHook.after_train_iter              iteration i (from 0) has started when i + 1 >= begin_iter; before that avg = copy of src

The device holds no counter of its own: the kernel derives `steps` from the optimizer's update count (`FlatAdamW.state[4]`), which
a resumed run restores, and the momenta are a table the host computes once in fp64 and rounds to fp32 -- the schedule cannot differ
between host and device.  Stated deviation: with `accumulative_counts=k` the average moves once per UPDATE (`begin_iter` and
`interval` count updates too); mmengine's hook lerps on every iteration, also on those where the wrapper withholds the update."""
import math

import numpy as np
import torch

from . import ops

TYPES = ("ExponentialMovingAverage", "ExpMomentumEMA")
MAX_TABLE = 1 << 22          # entries (16 MiB of fp32): a schedule that needs more is refused


def momentum_table(type="ExponentialMovingAverage", momentum=0.0002, gamma=2000):
    """-> fp32 numpy [n]: entry c is the momentum of started update c (`steps` == c), computed in fp64 and rounded once; the last
    entry is the value the schedule has converged to in fp32 (every later c rounds to it), so `table[min(c, n - 1)]` is the
    schedule.  ExponentialMovingAverage: one entry."""
    if type == "StochasticWeightAverage":
        raise NotImplementedError("WeightEMA(type='StochasticWeightAverage'): an equal-weight average is no exponential one")
    if type not in TYPES:
        raise ValueError(f"WeightEMA: type {type!r} is none of {TYPES}")
    momentum = float(momentum)
    if not 0.0 < momentum < 1.0:
        raise ValueError(f"WeightEMA: momentum {momentum} outside (0, 1)")
    limit = np.float32(momentum)
    if type == "ExponentialMovingAverage":
        return np.array([limit], dtype=np.float32)
    gamma = float(gamma)
    if not gamma > 0:
        raise ValueError(f"WeightEMA: gamma {gamma} must be positive")
    # the sequence falls monotonically towards `momentum` and rounds to it once the exponential term is of the order of half an ulp
    # of it, between momentum * 2^-25 and 2^-24; with a factor 4 for the rounding of `momentum` itself, no sooner than at
    # c = gamma * ln((1 - momentum) * 2^22 / momentum) - 1: a table that long is refused without being built
    too_long = ValueError(f"WeightEMA: ExpMomentumEMA(momentum={momentum}, gamma={gamma}) needs a momentum table of more than "
                          f"{MAX_TABLE} entries")
    if gamma * math.log((1.0 - momentum) * 2.0 ** 22 / momentum) - 1.0 > MAX_TABLE:
        raise too_long
    out = []
    for c in range(MAX_TABLE):          # (math.exp, one value at a time: what tests/ema_ref.py evaluates, to the bit)
        out.append(np.float32((1.0 - momentum) * math.exp(-(1.0 + c) / gamma) + momentum))
        if out[-1] == limit:
            return np.array(out, dtype=np.float32)
    raise too_long


def ema_plan(update, begin_iter=0, interval=1):
    """What update number `update` (the optimizer's count, from 1) does to the average -> (action, c): 'copy' (not started, or the
    first started update), 'skip' (a started update that `interval` passes over) or 'lerp' with the momentum of `steps` == c;
    c = update - max(begin_iter, 1), the started updates before this one.  The rule of s2f_ema_update (include/s2f.h)."""
    c = int(update) - max(int(begin_iter), 1)
    if c <= 0:
        return "copy", c
    return ("skip", c) if c % int(interval) else ("lerp", c)


class WeightEMA:
    """`optimizer`: a train.FlatAdamW.  Build it through `FlatAdamW(..., ema=True | dict(...))`, which records `update()` behind its
    own launches; the arguments are mmengine's EMAHook's (`type` is its `ema_type`).

    `ema`: fp32, the averaged parameters in the layout of `optimizer.exp_avg` (starts as a copy of the parameters, as mmengine's
    deep copy of the model does).  `update_buffers=False` only: buffers are not averaged, the averaged model carries the training
    model's BatchNorm statistics.  `partials`: fp64 [chunks, 2], what `report()` reads."""

    def __init__(self, optimizer, type="ExponentialMovingAverage", momentum=0.0002, gamma=2000, interval=1, begin_iter=0,
                 update_buffers=False, **unknown):
        type = unknown.pop("ema_type", type)
        if unknown.pop("begin_epoch", 0):
            raise NotImplementedError("WeightEMA(begin_epoch=...): the loop counts iterations")
        if unknown:
            raise TypeError(f"WeightEMA: unexpected arguments {sorted(unknown)}")
        if update_buffers:
            raise NotImplementedError("WeightEMA(update_buffers=True): buffers are not averaged")
        interval, begin_iter = int(interval), int(begin_iter)
        if interval < 1 or begin_iter < 0:
            raise ValueError(f"WeightEMA: interval {interval} below 1 or begin_iter {begin_iter} below 0")
        self.momenta = momentum_table(type, momentum, gamma)          # (raises for the type and the momentum)
        self.args = dict(type=type, momentum=float(momentum), gamma=float(gamma), interval=interval, begin_iter=begin_iter,
                         update_buffers=False)
        self.optimizer, self.interval, self.begin_iter = optimizer, interval, begin_iter
        self.swapped = False
        dev = optimizer.exp_avg.device
        self.table = torch.from_numpy(self.momenta).to(dev)
        self._allocate()
        self.reset()

    def _allocate(self):
        opt = self.optimizer
        self.ema = torch.zeros_like(opt.exp_avg)
        self.partials = torch.zeros(opt.chunks.shape[0], 2, dtype=torch.float64, device=self.ema.device)
        self._offsets = {id(p): off for p, off in zip(opt.params, opt.red.offsets)}
        self._tables = (opt.slots.data_ptr(), opt.chunks.data_ptr())

    def _check(self, what):
        if self.swapped:
            raise RuntimeError(f"WeightEMA.{what} while the averaged weights are swapped in; restore() first")
        opt = self.optimizer
        if (opt.slots.data_ptr(), opt.chunks.data_ptr()) != self._tables or self.ema.numel() != opt.exp_avg.numel():
            raise RuntimeError("WeightEMA: the optimizer's tables were rebuilt; call rebuild() (FlatAdamW.rebuild() does)")

    def reset(self):
        """the average <- a copy of the parameters as they are in stream order now (one launch): a fresh average, or one behind a
        checkpoint that carried none"""
        self._check("reset")
        opt = self.optimizer
        ops.state_copy(opt.params, opt.slots, opt.chunks, self.ema.view(torch.int32))

    def update(self):
        """one launch behind s2f_adamw_step (`FlatAdamW.step()` calls it); capturable"""
        self._check("update")
        opt = self.optimizer
        ops.ema_update(opt.slots, opt.chunks, self.ema, opt.state, self.table, self.begin_iter, self.interval, self.partials,
                       params=opt.params)

    def _exchange(self):
        opt = self.optimizer
        ops.ema_swap(opt.slots, opt.chunks, self.ema, params=opt.params)
        self.swapped = not self.swapped
        # the parameters changed behind autograd's back: every version-keyed cache re-converts at its next use
        opt.mark_updated()

    def swap(self):
        """the parameters <- the average, `ema` <- the training weights: one launch, then `optimizer.mark_updated()`"""
        self._check("swap")
        self._exchange()

    def restore(self):
        """the way back from `swap()`: the training weights return bit for bit"""
        if not self.swapped:
            raise RuntimeError("WeightEMA.restore without a swap()")
        self._exchange()

    def steps(self, updates):
        """mmengine's `steps` (the calls of update_parameters) after `updates` updates of the optimizer"""
        return max(0, int(updates) - max(self.begin_iter, 1) + 1)

    def momentum_at(self, updates):
        """the momentum applied by the last of `updates` updates that touched the average: the table's entry, 1.0 for a copy, None
        before the first update"""
        for t in range(int(updates), 0, -1):
            action, c = ema_plan(t, self.begin_iter, self.interval)
            if action == "copy":
                return 1.0
            if action == "lerp":
                return float(self.momenta[min(c, len(self.momenta) - 1)])
        return None

    def report(self, updates=None):
        """-> {'ema/drift': |p - e| / |e| over all parameters as of the last update that touched the average, 'ema/momentum': that
        update's momentum}: ONE read of `partials`, summed on the host in chunk order.  `updates`: the optimizer's update count
        where the caller knows it (a loop does); None reads it from the device."""
        updates = int(self.optimizer.state[4].item()) if updates is None else int(updates)
        m = self.momentum_at(updates)
        if m is None:
            return {}
        d2 = e2 = 0.0
        for d, e in self.partials.cpu().tolist():
            d2 += d
            e2 += e
        return {"ema/drift": math.sqrt(d2 / e2) if e2 > 0 else float("nan"), "ema/momentum": m}

    def rebuild(self):
        """after `FlatAdamW.rebuild()` laid the moments out again (it calls this): the average follows, values kept per parameter"""
        if self.swapped:
            raise RuntimeError("WeightEMA.rebuild while the averaged weights are swapped in; restore() first")
        old, offsets = self.ema, self._offsets
        self._allocate()
        for p, off in zip(self.optimizer.params, self.optimizer.red.offsets):
            o = offsets[id(p)]
            self.ema[off:off + p.numel()] = old[o:o + p.numel()]
