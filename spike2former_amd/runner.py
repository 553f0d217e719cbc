"""The training LOOP around the captured step -- what mmengine's runner does between iterations for the Spike2Former configs:

    train_cfg = dict(type='IterBasedTrainLoop', max_iters=160000, val_interval=2500)       configs/_base_/schedules/schedule_160k.py
    default_hooks = dict(logger=dict(type='LoggerHook', interval=50, log_metric_by_epoch=False),
                         param_scheduler=dict(type='ParamSchedulerHook'),
                         checkpoint=dict(type='CheckpointHook', by_epoch=False, interval=10000, save_best='mIoU'), ...)
    load_from = None; resume = False                                                         configs/_base_/default_runtime.py

`graph.GraphedHungarianStep(assign="device", optimizer=FlatAdamW(...))` is a whole iteration that never waits for the GPU; three
things a loop needs would each put a host stop back into it, and each has a device-side piece here instead:

  * the losses `step()` returns are static tensors, valid until the next call: `TrainLog` is a ring on the device (devring.py) that
    the step's last graph appends one row to per replay (ops.train_log_append);
  * a checkpoint of ~1 000 parameter and buffer tensors behind a pointer table: `TrainState.snapshot()` is ONE launch into a staging
    buffer (ops.state_copy) plus three device-to-device copies, all queued on the step's stream -- the next replay may start at
    once; the copy to pinned memory runs on a side stream, `torch.save` in a writer thread;
  * a step whose status word is set has NaN losses and has applied them: the ring's head latches the FIRST row that held a
    non-finite value, `LoggerHook` raises `FloatingPointError` naming that iteration, and no checkpoint is written past it.

mmengine (0.8.4) is not part of the reference tree: `LoggerHook`, `CheckpointHook` and the loop are restated from its published
behaviour, and like the schedulers of train.py their parity is UNPINNED (DESIGN.md section 7 lists the deviations).  Iterations are
named as mmengine names them in file names and log lines: "iteration n" is the n-th, counted from 1.

    log = TrainLog(window=50)
    step = GraphedHungarianStep(model, example_in, example_seg, red, optimizer=optim, assign="device", log=log,
                                firing=FiringLog(model, window=50))          # (optional: per-neuron firing rates in the log)
    loop = TrainLoop(step, optim, sched, aug, batches, max_iters=160000, val_interval=2500, validate=lambda: evaluate(...),
                     hooks=[dict(type='LoggerHook', interval=50), dict(type='CheckpointHook', interval=10000, save_best='mIoU')],
                     work_dir='work_dirs/run')
    loop.run()
"""
import collections
import concurrent.futures
import copy
import datetime
import json
import logging
import os
import time

import numpy as np
import torch

from . import ops
from .devring import DeviceRing, unwrap
from .graph import step_tail
from .registry import HOOKS

logger = logging.getLogger("spike2former_amd")

LogRead = collections.namedtuple("LogRead", "names rows count first_nonfinite")


def _rank_world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def noise_scale(micro_sq, accum_sq, small, big):
    """The simple gradient-noise-scale estimate from two batch sizes (McCandlish et al. 2018, "An Empirical Model of Large-Batch
    Training", appendix A.1): `micro_sq` = mean |g|^2 at batch `small`, `accum_sq` = mean |g|^2 at batch `big` ->
        G2 = (big * accum_sq - small * micro_sq) / (big - small)          (unbiased for |G|^2, the true gradient's)
        S  = (micro_sq - accum_sq) / (1 / small - 1 / big)                (unbiased for the trace of the per-example covariance)
    -> (S / G2, G2, S): the noise scale in the unit of `small` and `big` (images); S / G2 is None where G2 <= 0 (the estimate of
    |G|^2 is itself noise then).  The ratio is taken of means, not as a mean of ratios."""
    small, big = float(small), float(big)
    g2 = (big * accum_sq - small * micro_sq) / (big - small)
    s = (micro_sq - accum_sq) / (1.0 / small - 1.0 / big)
    return (s / g2 if g2 > 0 else None), g2, s


class TrainLog(DeviceRing):
    """A devring.DeviceRing of the last `window` iterations' scalars: fp32 [window, capacity], no state words; head[1] latches the
    first row with a non-finite value.  `terms`: ordered {name: one-element fp32 tensor}, static tensors of a captured step (its
    losses, their sum, the optimizer's grad_norm and clip_coef).  `append()` is one launch that copies them into the next row.

    A captured step knows its static tensors only while it is being recorded, where nothing may be uploaded: build the log without
    terms (`TrainLog(window=..., device=...)`, at most `capacity` of them), hand it to the step (`log=`), and the step `declare`s the
    names while recording -- the recorded launch reads a pointer table that `bind` fills after the capture."""
    HEAD = (0, -1)

    def __init__(self, terms=None, window=64, device=None, capacity=64):
        if window < 1:
            raise ValueError(f"TrainLog: window {window} below 1")
        if terms is not None:
            capacity = len(terms)
            device = next(iter(terms.values())).device if device is None else device
        if not 1 <= capacity <= ops.TRAIN_LOG_MAX_TERMS:
            raise ValueError(f"TrainLog: {capacity} terms outside 1 .. {ops.TRAIN_LOG_MAX_TERMS}")
        self.window, self.stride = int(window), int(capacity)
        cells = self.window * self.stride
        _, ring = self._allocate(0, (cells + 1) // 2, "cuda" if device is None else device)
        self.ring = ring.view(torch.float32)[:cells].view(self.window, self.stride)
        self.clear()
        self._table = torch.zeros(self.stride, dtype=torch.int64, device=self.device) if self.device.type == "cuda" else None
        self.names, self._srcs = None, None
        if terms is not None:
            self.bind(terms)

    def declare(self, names):
        """the names of the terms, before their tensors can be bound (host only: legal while a capture records)"""
        names = list(names)
        if not 1 <= len(names) <= self.stride:
            raise ValueError(f"TrainLog: {len(names)} terms for a capacity of {self.stride}")
        self.names = names

    def bind(self, terms):
        """the tensors behind the names: uploads their addresses into the pointer table (not under capture)"""
        self.declare(terms.keys())
        self._srcs = list(terms.values())
        if self._table is not None:
            self._table[:len(self._srcs)].copy_(ops.train_log_table(self._srcs, "cpu"))

    def append(self):
        if self.names is None:
            raise RuntimeError("TrainLog.append before its terms are declared")
        if self._table is None and self._srcs is None:
            raise RuntimeError("TrainLog.append on the CPU before its terms are bound")
        ops.train_log_append(self._srcs, self.ring, self.head[:2], table=self._table, n=len(self.names))

    def read(self):
        """-> LogRead(names, rows, count, first_nonfinite): the last min(count, window) rows, oldest first, as numpy fp32
        [rows, terms]; the number of rows appended so far; the index (from 0) of the first row that held a non-finite value, or
        None.  One `fetch()`."""
        words = self.fetch()
        count, bad = int(words[0]), int(words[1])
        ring = words[4:].view(np.float32)[:self.window * self.stride].reshape(self.window, self.stride)
        rows = unwrap(ring, count, self.window)[:, :len(self.names or ())]
        return LogRead(list(self.names or ()), np.ascontiguousarray(rows), count, None if bad < 0 else bad)


class TrainState:
    """Snapshot, file and resume of a run's whole state: every tensor of `model.state_dict()` (parameters and buffers, by name),
    `optimizer`'s two moments and step count (a train.FlatAdamW), `scheduler.t`, `augment`'s generator.

    `snapshot()` queues, on the current stream, one `ops.state_copy` of the model into a device staging buffer and the device-to-
    device copies of the moments and the optimizer's state words; the copies into pinned memory follow on a side stream.  The next
    replay of the step may be queued at once: it can overtake nothing, the stagings are written before it in stream order.
    `write(path, meta)` hands the pinned buffers to ONE writer thread, which waits for the side stream's event and `torch.save`s
    views of them; a following `snapshot()`, `load()` or `close()` joins a write still running (`async_write=False`: written by
    the caller).

    An optimizer with a weight average (`FlatAdamW(ema=...)`): the snapshot also copies the average's flat buffer, exactly like the
    moments, and the file follows mmengine's EMAHook rule -- `state_dict` holds the AVERAGED parameters next to the model's buffers
    (what `load_from` and inference read), `ema_state_dict` holds `module.<name>` = the training value of every `state_dict` entry
    and `steps`.  `load(resume=True)` restores both; a file without `ema_state_dict`, and every load without `resume`, starts the
    average from the loaded weights.  No snapshot while the average is swapped in.  Without an average the file is what it was."""

    def __init__(self, model, optimizer, scheduler=None, augment=None, async_write=True):
        self.model, self.optimizer, self.scheduler, self.augment = model, optimizer, scheduler, augment
        self.async_write = bool(async_write)
        self._ptrs = self._tag = self._host_side = None
        self._pending = []
        self._pool = None
        self._staged = self._copied = self._side = None
        self._build(self._tensors())
        if optimizer is not None:
            self._opt_dev = [torch.empty_like(t) for t in (optimizer.exp_avg, optimizer.exp_avg_sq, optimizer.state)]
            self._opt_host = [self._pinned(torch.zeros_like(t, device="cpu")) for t in self._opt_dev]
        self._ema_dev = self._ema_host = None
        if self.ema is not None:
            self._ema_dev = torch.empty_like(self.ema.ema)
            self._ema_host = self._pinned(torch.zeros_like(self._ema_dev, device="cpu"))

    @property
    def ema(self):
        """the optimizer's ema.WeightEMA (FlatAdamW(ema=...)), or None"""
        return getattr(self.optimizer, "ema", None)

    # ------------------------------------------------------------------------------------------------ tables
    def _tensors(self):
        return self.model.state_dict(keep_vars=True)

    def _pinned(self, t):
        return t.pin_memory() if self.device.type == "cuda" else t

    def _build(self, named):
        self.names, self.tensors = list(named.keys()), list(named.values())
        if not self.tensors:
            raise ValueError("TrainState: the model has no state")
        self.device = self.tensors[0].device
        for n, t in named.items():
            if not t.is_contiguous():
                raise RuntimeError(f"TrainState: {n} is not contiguous")
            if t.device != self.device:
                raise RuntimeError(f"TrainState: {n} on {t.device}, the model on {self.device}")
        self.slots, self.chunks, words = ops.state_table(self.tensors, self.device)
        self._spans = [(off, n) for _, off, n in self.slots.tolist()]
        self._ptrs = tuple(t.data_ptr() for t in self.tensors)
        if getattr(self, "flat", None) is None or self.flat.numel() != words:
            self.flat = torch.zeros(words, dtype=torch.int32, device=self.device)
            self.host_flat = self._pinned(torch.zeros(words, dtype=torch.int32))

    def _refresh(self):
        """the table follows the model: rebuilt when a tensor's storage moved (model.to(...), a re-flattened sibling group)"""
        named = self._tensors()
        if list(named.keys()) != self.names or tuple(t.data_ptr() for t in named.values()) != self._ptrs:
            self._build(named)

    # ------------------------------------------------------------------------------------------------ snapshot and file
    def join(self):
        """wait for the writes still running; re-raises what a write raised"""
        pending, self._pending = self._pending, []
        for f in pending:
            f.result()

    def host_state(self):
        """What of the state lives on the host and differs between the ranks: the augment generator's state.  A collective at
        world size > 1 (every rank calls it) -> the states by rank, for the one rank that writes; a single process: its state."""
        mine = None if self.augment is None else copy.deepcopy(self.augment.rng.bit_generator.state)
        rank, world = _rank_world()
        if world == 1:
            return mine
        import torch.distributed as dist
        states = [None] * world
        dist.all_gather_object(states, mine)
        return states

    def snapshot(self, tag=None, rng=None):
        """Queue a copy of the whole state as it is in stream order NOW.  `tag`: a snapshot with the tag of the last one (not None)
        is that one -- two files of one iteration share one copy.  `rng`: what `host_state()` returned (default: it is called
        here, which at world size > 1 every rank has to do)."""
        ema = self.ema
        if ema is not None and ema.swapped:
            raise RuntimeError("TrainState.snapshot while the averaged weights are swapped in (WeightEMA.restore() first)")
        if tag is not None and tag == self._tag:
            return
        self.join()          # the views of the file being written alias the pinned buffers
        self._refresh()
        opt = self.optimizer
        cuda = self.device.type == "cuda"
        if cuda:
            cur = torch.cuda.current_stream()
            if self._copied is not None:
                cur.wait_event(self._copied)          # the last snapshot's copies to the host still read the stagings
        ops.state_copy(self.tensors, self.slots, self.chunks, self.flat)
        if opt is not None:
            if self._opt_dev[0].shape != opt.exp_avg.shape:
                raise RuntimeError("TrainState: the optimizer's buffers were laid out again (FlatAdamW.rebuild()); build a new TrainState")
            for dst, src in zip(self._opt_dev, (opt.exp_avg, opt.exp_avg_sq, opt.state)):
                dst.copy_(src, non_blocking=True)
        if ema is not None:
            if self._ema_dev.shape != ema.ema.shape:
                raise RuntimeError("TrainState: the weight average was laid out again (FlatAdamW.rebuild()); build a new TrainState")
            self._ema_dev.copy_(ema.ema, non_blocking=True)
        if cuda:
            if self._side is None:
                self._side, self._staged, self._copied = torch.cuda.Stream(), torch.cuda.Event(), torch.cuda.Event()
            self._staged.record(cur)
            with torch.cuda.stream(self._side):
                self._side.wait_event(self._staged)
                self.host_flat.copy_(self.flat, non_blocking=True)
                if opt is not None:
                    for dst, src in zip(self._opt_host, self._opt_dev):
                        dst.copy_(src, non_blocking=True)
                if ema is not None:
                    self._ema_host.copy_(self._ema_dev, non_blocking=True)
                self._copied.record(self._side)
        else:
            self.host_flat.copy_(self.flat)
            if opt is not None:
                for dst, src in zip(self._opt_host, self._opt_dev):
                    dst.copy_(src)
            if ema is not None:
                self._ema_host.copy_(self._ema_dev)
        # what lives on the host is taken now: the loop moves both on while the file is written
        self._host_side = dict(t=None if self.scheduler is None else int(self.scheduler.t),
                               rng=self.host_state() if rng is None else rng,
                               names=list(self.names), spans=list(self._spans),
                               shapes=[(tuple(t.shape), t.dtype) for t in self.tensors], ema=ema is not None,
                               opt=None if opt is None else [(g["name"], off, tuple(p.shape))
                                                             for g, p, off in zip(opt.param_groups, opt.params, opt.red.offsets)])
        self._tag = tag

    def _payload(self, meta, best):
        s = self._host_side
        sd = collections.OrderedDict()
        for name, (off, n), (shape, dtype) in zip(s["names"], s["spans"], s["shapes"]):
            t = self.host_flat[off:off + n].view(dtype).view(shape)
            # (torch.save refuses views of ONE storage under two dtypes: the fp32 tensors alias the pinned buffer, the few others
            # -- BatchNorm's int64 counters -- are copied out of it)
            sd[name] = t if dtype == torch.float32 else t.clone()
        out = dict(meta=dict(meta or {}), state_dict=sd)
        if s["opt"] is not None:
            m, v, st = self._opt_host
            out["optimizer"] = dict(step=int(st[4]), state={name: {"exp_avg": m[off:off + int(np.prod(shape))].view(shape),
                                                                   "exp_avg_sq": v[off:off + int(np.prod(shape))].view(shape)}
                                                            for name, off, shape in s["opt"]})
        if s["ema"]:
            # mmengine's EMAHook.before_save_checkpoint: `state_dict` is what inference reads, the average; the training values
            # move to `ema_state_dict` under the averaged model's `module.` prefix, next to its `steps`
            slot = {name: (off, int(np.prod(shape)), shape) for name, off, shape in s["opt"]}
            train = collections.OrderedDict(steps=torch.tensor(self.ema.steps(int(self._opt_host[2][4])), dtype=torch.long))
            for name, t in list(sd.items()):
                train[f"module.{name}"] = t
                if name in slot:
                    off, n, shape = slot[name]
                    sd[name] = self._ema_host[off:off + n].view(shape)
            out["ema_state_dict"] = train
        out["param_schedulers"] = [] if s["t"] is None else [dict(t=s["t"])]
        out["augment"] = s["rng"]
        out["best"] = best
        return out

    def write(self, path, meta=None, best=None, done=None, async_write=None):
        """The last snapshot -> `path` (torch.save; written under another name and renamed, so a file that exists is complete).
        `done(path)` runs behind the file, in the thread that wrote it."""
        if self._host_side is None:
            raise RuntimeError("TrainState.write before snapshot")
        meta, best = copy.deepcopy(meta), copy.deepcopy(best)

        def job():
            if self._copied is not None:
                self._copied.synchronize()
            tmp = f"{path}.tmp"
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            torch.save(self._payload(meta, best), tmp)
            os.replace(tmp, path)
            if done is not None:
                done(path)
        if self.async_write if async_write is None else async_write:
            if self._pool is None:
                self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix="s2f-checkpoint")
            self._pending.append(self._pool.submit(job))
        else:
            self.join()
            job()

    def close(self):
        try:
            self.join()
        finally:
            if self._pool is not None:
                self._pool.shutdown(wait=True)
                self._pool = None

    # ------------------------------------------------------------------------------------------------ load and resume
    def load(self, path, resume=False):
        """`path`: a file of `write`, or any checkpoint whose 'state_dict' (or the file itself) maps this model's names to tensors
        of its shapes -- strict: a RuntimeError lists what is missing, unexpected or mis-shaped.  The values go through the pinned
        and the device staging buffers and ONE `ops.state_copy(to_params=True)`.  `resume`: also both moments, the step count, the
        scheduler's `t` and the augment generator.  -> the file's dictionary without its tensors (meta, best, ...)."""
        ck = torch.load(path, map_location="cpu", weights_only=True)
        sd = ck["state_dict"] if isinstance(ck, dict) and "state_dict" in ck else ck
        self.join()
        self._refresh()
        missing = [n for n in self.names if n not in sd]
        have = set(self.names)
        unexpected = [n for n in sd if n not in have]
        shapes = [f"{n}: {tuple(sd[n].shape)} in the file, {tuple(t.shape)} in the model" for n, t in zip(self.names, self.tensors)
                  if n in sd and tuple(sd[n].shape) != tuple(t.shape)]
        opt, om = self.optimizer, None
        if resume:
            if not isinstance(ck, dict) or "optimizer" not in ck or "meta" not in ck:
                raise RuntimeError(f"{path} holds no optimizer state to resume from")
            if opt is None:
                raise RuntimeError("TrainState.load(resume=True) needs the optimizer")
            om = ck["optimizer"]["state"]
            missing += [f"optimizer:{g['name']}" for g in opt.param_groups if g["name"] not in om]
            unexpected += [f"optimizer:{n}" for n in om if n not in {g["name"] for g in opt.param_groups}]
            shapes += [f"optimizer:{g['name']}: {tuple(om[g['name']][k].shape)} in the file, {tuple(p.shape)} in the model"
                       for g, p in zip(opt.param_groups, opt.params) if g["name"] in om
                       for k in ("exp_avg", "exp_avg_sq") if tuple(om[g["name"]][k].shape) != tuple(p.shape)]
        # a run with a weight average resumes BOTH copies: the file's `state_dict` is the average, the training values are in its
        # `ema_state_dict` (see the class); every other load takes `state_dict` and starts the average from it
        ema = self.ema
        if ema is not None and ema.swapped:
            raise RuntimeError("TrainState.load while the averaged weights are swapped in (WeightEMA.restore() first)")
        esd = ck.get("ema_state_dict") if resume and ema is not None and isinstance(ck, dict) else None
        src = sd
        if esd is not None:
            missing += [f"ema_state_dict:module.{n}" for n in self.names if f"module.{n}" not in esd]
            shapes += [f"ema_state_dict:module.{n}: {tuple(esd[f'module.{n}'].shape)} in the file, {tuple(t.shape)} in the model"
                       for n, t in zip(self.names, self.tensors)
                       if f"module.{n}" in esd and tuple(esd[f"module.{n}"].shape) != tuple(t.shape)]
            src = {n: esd.get(f"module.{n}") for n in self.names}
        if missing or unexpected or shapes:
            raise RuntimeError(f"{path} does not fit the model -- missing: {missing}; unexpected: {unexpected}; mis-shaped: {shapes}")
        if self._copied is not None:
            self._copied.synchronize()
        for name, t, (off, n) in zip(self.names, self.tensors, self._spans):
            self.host_flat[off:off + n].copy_(src[name].to(t.dtype).contiguous().reshape(-1).view(torch.int32))
        self.flat.copy_(self.host_flat, non_blocking=True)
        ops.state_copy(self.tensors, self.slots, self.chunks, self.flat, to_params=True)
        if esd is not None:
            self._ema_host.zero_()
            for g, p, off in zip(opt.param_groups, opt.params, opt.red.offsets):
                self._ema_host[off:off + p.numel()].copy_(sd[g["name"]].to(torch.float32).reshape(-1))
            ema.ema.copy_(self._ema_host, non_blocking=True)
        elif ema is not None:
            ema.reset()          # (one launch behind the copy above: the average starts from the loaded weights)
        if resume:
            m, v, _ = self._opt_host
            m.zero_(), v.zero_()
            for g, p, off in zip(opt.param_groups, opt.params, opt.red.offsets):
                m[off:off + p.numel()].copy_(om[g["name"]]["exp_avg"].reshape(-1))
                v[off:off + p.numel()].copy_(om[g["name"]]["exp_avg_sq"].reshape(-1))
            opt.exp_avg.copy_(m, non_blocking=True)
            opt.exp_avg_sq.copy_(v, non_blocking=True)
            opt.state[4:5].fill_(float(ck["optimizer"]["step"]))
            sched = ck.get("param_schedulers") or []
            if self.scheduler is not None and sched:
                self.scheduler.t = int(sched[0]["t"])
                self.scheduler._apply()
            if self.augment is not None and ck.get("augment") is not None:
                rng, (rank, world) = ck["augment"], _rank_world()
                if isinstance(rng, list):          # a run of several ranks: one generator each
                    if len(rng) != world:
                        raise RuntimeError(f"{path} was written by a run of {len(rng)} ranks; this one has {world}")
                    rng = rng[rank]
                elif world > 1:
                    raise RuntimeError(f"{path} was written by a single process; this run has {world} ranks")
                self.augment.rng.bit_generator.state = rng
        # the weights changed behind autograd's back, as after a replayed update: every cache keyed on a tensor's version
        # re-converts; the graph's own (lr, weight_decay) table is uploaded again
        torch.autograd.graph.increment_version(self.tensors)
        if opt is not None:
            opt.mark_updated()
            opt._hyper_last = None
        if self.device.type == "cuda":
            torch.cuda.current_stream().synchronize()          # the pinned buffers are free again
        self._tag = None
        return {k: v for k, v in ck.items() if k not in ("state_dict", "optimizer", "ema_state_dict")} if isinstance(ck, dict) and "state_dict" in ck else {}


# ---------------------------------------------------------------------------------------------------- hooks
class _Hook:
    priority = 50          # mmengine's NORMAL; a loop runs its hooks in ascending order of it

    def before_run(self, loop):
        pass

    def after_train_iter(self, loop):
        pass

    def after_val(self, loop, metrics):
        pass

    def after_run(self, loop):
        pass


@HOOKS.register_module()
class ParamSchedulerHook(_Hook):
    """Accepted for the configs' `default_hooks`; `TrainLoop` steps the scheduler itself, after every iteration."""
    priority = 70


@HOOKS.register_module()
class LoggerHook(_Hook):
    """mmengine's LoggerHook + LogProcessor(window_size=10, by_epoch=False) for the train loop: at iteration n with n % interval ==
    0, and at the last one, ONE `TrainLog.read()`; the mean of the last `window_size` rows of every term, the learning rate of
    parameter group 0 in that iteration, seconds per iteration since the last line, the time left at that rate and the peak of
    allocated device memory in MiB -- one line on the `spike2former_amd` logger and one JSON line in {work_dir}/vis_data/scalars.json.
    A non-finite value in ANY iteration since the last check raises FloatingPointError naming the first (TrainLoop.check_finite).

    Every ring log of `loop.logs` (a step built with `firing=FiringLog(...)`, an optimizer built with `grad_log=...`): ONE read more
    per log line, over the rows appended since the last line (the ring holds at least `interval` of them).  Its `report()` says what
    the line and scalars.json carry (`firing/...`, `grad/...`), the JSON line that goes to {work_dir}/vis_data/{firing,grad}.jsonl
    and what its latch warns of, ONCE: a finding, not an error -- nothing is raised.  Every rank reads its own rings; rank 0 writes.

    An optimizer built with `accumulative_counts=k`: the gradient log's rows count UPDATES (the warning and grad.jsonl name the
    iteration of the update), and the line carries `grad/accum` = k and `grad/noise_scale`, in images: `noise_scale()` of the means
    of the step's two hidden terms `grad_sq_micro` (mean |g|^2 of the group's micro-batches, b images each) and `grad_sq_accum`
    (|g|^2 of the accumulated and all-reduced gradient, k b W images) over the rows of UPDATE iterations since the last line that
    the TrainLog's ring still holds; omitted where no such row is in reach or the estimate of |G|^2 is not positive.  A diagnostic
    without a counterpart in the reference, and approximate: train-mode BatchNorm and the matching couple the images of a
    micro-batch; at world size > 1 the micro-batch term is this rank's.

    An optimizer built with `ema=...`: the line carries `ema/drift` (|p - e| / |e| over all parameters, as of the last update that
    touched the average) and `ema/momentum` (that update's), one read of the average's partial sums (ema.WeightEMA.report)."""
    priority = 60
    HIDDEN = ("clip_coef", "grad_sq_micro", "grad_sq_accum")

    def __init__(self, interval=50, window_size=10, log_metric_by_epoch=False, **unused):
        if log_metric_by_epoch:
            raise NotImplementedError("LoggerHook(log_metric_by_epoch=True): the loop counts iterations")
        if interval < 1 or window_size < 1:
            raise ValueError("LoggerHook: interval and window_size are at least 1")
        self.interval, self.window_size = int(interval), int(window_size)

    def before_run(self, loop):
        if loop.log is None:
            raise ValueError("LoggerHook needs a step built with log=TrainLog(...)")
        for log, what, rows in ((loop.log, "window_size", self.window_size), *((log, "interval", self.interval) for log, _ in loop.logs)):
            if log.window < rows:
                raise ValueError(f"LoggerHook({what}={rows}) over a {type(log).__name__} of {log.window} rows")
        self._clock, self._last, self._warned = time.perf_counter(), loop.iter, set()          # (the logs whose latch was reported)

    def _accum(self, loop, n, read, record):
        """grad/accum and grad/noise_scale (see the class); `read`: the TrainLog as of iteration n, whose last row is iteration n"""
        counts = loop.accum.counts
        record["grad/accum"] = counts
        if "grad_sq_micro" not in read.names or "grad_sq_accum" not in read.names:
            return
        first = n - len(read.rows) + 1          # the iteration (from 1) of the ring's oldest row
        at = [i for i in range(len(read.rows)) if first + i > self._last and ((first + i) % counts == 0 or first + i == loop.max_iters)]
        if not at:
            return
        m = float(np.mean(read.rows[at, read.names.index("grad_sq_micro")].astype(np.float64)))
        big = float(np.mean(read.rows[at, read.names.index("grad_sq_accum")].astype(np.float64)))
        b = int(loop.step.static_in.shape[0])
        ratio = noise_scale(m, big, b, counts * b * loop.world)[0]
        if ratio is not None:
            record["grad/noise_scale"] = float(ratio)

    def _write(self, loop, name, record):
        """one JSON line more in {work_dir}/vis_data/{name}; rank 0 alone writes"""
        if loop.work_dir is not None and loop.rank == 0:
            path = os.path.join(loop.work_dir, "vis_data", name)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "a") as f:
                f.write(json.dumps(record) + "\n")

    def _emit(self, loop, record, line):
        logger.info(line)
        self._write(loop, "scalars.json", record)

    def after_train_iter(self, loop):
        n = loop.iter + 1
        if n % self.interval and n != loop.max_iters:
            return
        read = loop.check_finite()
        rows = read.rows[-self.window_size:]
        now = time.perf_counter()
        per_iter = (now - self._clock) / max(n - self._last, 1)
        record = dict(lr=float(loop.lr), time=per_iter, eta=per_iter * (loop.max_iters - n),
                      memory=int(torch.cuda.max_memory_allocated() // 2 ** 20) if torch.cuda.is_available() else 0)
        for j, name in enumerate(read.names):
            if name not in self.HIDDEN and len(rows):
                record[name] = float(np.mean(np.ascontiguousarray(rows[:, j])))          # fp32, in the rows' order
        for log, iteration_of in loop.logs:
            keys, items, warning = log.report(n, self._last, iteration_of)
            record.update(keys)
            if items is not None:
                self._write(loop, f"{log.prefix}.jsonl", items)
            if warning is not None and log.prefix not in self._warned:
                self._warned.add(log.prefix)
                logger.warning(warning)
        if getattr(loop, "accum", None) is not None:
            self._accum(loop, n, read, record)
        ema = getattr(loop.optimizer, "ema", None)
        if ema is not None:          # ema/drift, ema/momentum: one read of the average's partial sums
            record.update(ema.report(loop.updates_done(n)))
        self._clock, self._last = now, n
        record.update(iter=n, step=n)
        eta = str(datetime.timedelta(seconds=int(record["eta"])))
        terms = "  ".join(f"{k}: {v}" if isinstance(v, (str, int)) else f"{k}: {v:.4f}" for k, v in record.items()
                          if k not in ("lr", "time", "eta", "memory", "iter", "step"))
        self._emit(loop, record, f"Iter(train) [{n:>{len(str(loop.max_iters))}}/{loop.max_iters}]  lr: {record['lr']:.4e}  eta: {eta}  "
                                 f"time: {per_iter:.4f}  memory: {record['memory']}  {terms}")

    def after_val(self, loop, metrics):
        n = loop.iter + 1
        scalars = {k: float(v) for k, v in metrics.items() if np.isscalar(v) or getattr(v, "ndim", 1) == 0}
        self._emit(loop, dict(scalars, step=n), f"Iter(val) [{n}]  " + "  ".join(f"{k}: {v:.4f}" for k, v in scalars.items()))


@HOOKS.register_module()
class CheckpointHook(_Hook):
    """mmengine's CheckpointHook by iteration: `iter_{n}.pth` every `interval` iterations (and, `save_last`, after the last),
    `last_checkpoint` naming the newest complete file, at most `max_keep_ckpts` of them kept (-1: all); `save_best='mIoU'`:
    after each validation the key is compared by `rule` ('greater' / 'less'; None: by mmengine's key lists, 'less' for keys that
    contain 'loss') and `best_{key}_iter_{n}.pth` replaces the previous best file.  Rank 0 alone writes.  Every file is a
    `TrainState` snapshot; none is written for an iteration at or behind a non-finite loss."""
    priority = 90
    GREATER = ("acc", "top", "AR@", "auc", "precision", "mAP", "mDice", "mIoU", "mAcc", "aAcc")
    LESS = ("loss",)

    def __init__(self, interval=-1, by_epoch=False, save_last=True, max_keep_ckpts=-1, save_best=None, rule=None, **unused):
        if by_epoch:
            raise NotImplementedError("CheckpointHook(by_epoch=True): the loop counts iterations")
        if save_best is not None and not isinstance(save_best, str):
            raise NotImplementedError("CheckpointHook: save_best is one key")
        if rule is None and save_best is not None:
            low = save_best.lower()
            if any(k.lower() in low for k in self.LESS):
                rule = "less"
            elif any(k.lower() in low for k in self.GREATER):
                rule = "greater"
            else:
                raise ValueError(f"CheckpointHook: no rule can be inferred for save_best={save_best!r}; pass rule='greater' or 'less'")
        if rule not in (None, "greater", "less"):
            raise ValueError(f"CheckpointHook: rule {rule!r} is neither 'greater' nor 'less'")
        self.interval, self.save_last, self.max_keep = int(interval), bool(save_last), int(max_keep_ckpts)
        self.save_best, self.rule = save_best, rule
        self.kept, self.best_score, self.best_path = [], None, None

    def before_run(self, loop):
        if loop.work_dir is None:
            raise ValueError("CheckpointHook needs the loop's work_dir")
        accum = getattr(loop, "accum", None)
        if accum is not None and self.interval > 0 and self.interval % accum.counts:
            # a checkpoint inside a group would drop the accumulator (it is in no file); the one after the last iteration is always
            # on a boundary: the last iteration closes its group
            raise ValueError(f"CheckpointHook(interval={self.interval}) is no multiple of accumulative_counts={accum.counts}")
        best = (loop.resumed or {}).get("best") or {}
        if self.save_best is not None and best.get("key") == self.save_best:
            self.best_score, self.best_path = best.get("score"), best.get("path")

    def _best(self):
        return dict(key=self.save_best, score=self.best_score, path=self.best_path)

    def _published(self, loop, path):
        """behind a complete iter_{n}.pth (in the writer's thread): last_checkpoint, then the files beyond max_keep_ckpts"""
        with open(os.path.join(loop.work_dir, "last_checkpoint"), "w") as f:
            f.write(path)
        self.kept.append(path)
        while 0 < self.max_keep < len(self.kept):
            old = self.kept.pop(0)
            if os.path.exists(old):
                os.remove(old)

    def after_train_iter(self, loop):
        n = loop.iter + 1
        if not ((self.interval > 0 and n % self.interval == 0) or (self.save_last and n == loop.max_iters)):
            return
        loop.check_finite()          # on every rank: the error is everybody's
        rng = loop.state.host_state()          # (a collective)
        if loop.rank != 0:
            return
        loop.state.snapshot(tag=n, rng=rng)
        loop.state.write(os.path.join(loop.work_dir, f"iter_{n}.pth"), meta=loop.meta(), best=self._best(),
                         done=lambda path: self._published(loop, path))

    def after_val(self, loop, metrics):
        if self.save_best is None:
            return
        if self.save_best not in metrics:
            raise KeyError(f"CheckpointHook(save_best={self.save_best!r}): validation returned {sorted(metrics)}")
        score = float(metrics[self.save_best])
        better = self.best_score is None or (score > self.best_score if self.rule == "greater" else score < self.best_score)
        rng = loop.state.host_state() if loop.world > 1 else None          # (a collective: before any rank turns back)
        if not better or loop.rank != 0:
            return
        n, old = loop.iter + 1, self.best_path
        self.best_score, self.best_path = score, os.path.join(loop.work_dir, f"best_{self.save_best}_iter_{n}.pth")

        def replaced(path):
            if old is not None and old != path and os.path.exists(old):
                os.remove(old)
        loop.state.snapshot(tag=n, rng=rng)
        loop.state.write(self.best_path, meta=loop.meta(), best=self._best(), done=replaced)


@HOOKS.register_module()
class EMAHook(_Hook):
    """mmengine's EMAHook for a captured step: validation and the checkpoints' `state_dict` use an exponential moving average of
    the weights (ema.WeightEMA).  The average itself lives in the optimizer -- `FlatAdamW(..., ema=dict(...))` records its launch
    behind the update, inside the captured step, and a graph holds the launches it was recorded with -- so the hook attaches
    nothing: `before_run` checks that the optimizer's average is there and was built with THESE arguments (`ema_type` is the
    average's `type`), `before_val` swaps the averaged weights in and `after_val` swaps the training weights back (TrainLoop
    guarantees the way back when validation raises).  What the file holds: TrainState."""
    priority = 50

    def __init__(self, ema_type="ExponentialMovingAverage", momentum=0.0002, gamma=2000, interval=1, begin_iter=0,
                 update_buffers=False, strict_load=False, **unknown):
        from .ema import momentum_table
        if unknown.pop("begin_epoch", 0):
            raise NotImplementedError("EMAHook(begin_epoch=...): the loop counts iterations")
        if unknown:
            raise TypeError(f"EMAHook: unexpected arguments {sorted(unknown)}")
        if update_buffers:
            raise NotImplementedError("EMAHook(update_buffers=True): buffers are not averaged")
        if int(interval) < 1 or int(begin_iter) < 0:
            raise ValueError(f"EMAHook: interval {interval} below 1 or begin_iter {begin_iter} below 0")
        momentum_table(ema_type, momentum, gamma)          # (raises for the type, the momentum and a schedule too long for a table)
        self.args = dict(type=ema_type, momentum=float(momentum), gamma=float(gamma), interval=int(interval),
                         begin_iter=int(begin_iter), update_buffers=False)
        self.ema = None

    def before_run(self, loop):
        ema = getattr(loop.optimizer, "ema", None)
        want = {k: v for k, v in self.args.items() if k != "gamma" or self.args["type"] == "ExpMomentumEMA"}
        if ema is None or any(ema.args[k] != v for k, v in want.items()):
            have = None if ema is None else ema.args
            raise ValueError(f"EMAHook: the average is recorded with the optimizer's update and cannot be attached to a built step; "
                             f"build the optimizer as FlatAdamW(ema=dict({', '.join(f'{k}={v!r}' for k, v in want.items())})) "
                             f"(it has ema={have})")
        self.ema = ema

    def before_val(self, loop):
        self.ema.swap()

    def after_val(self, loop, metrics):
        if self.ema.swapped:
            self.ema.restore()


# ---------------------------------------------------------------------------------------------------- the loop
def _cycle(batches, skip):
    """the batches, restarted when exhausted, from the `skip`-th on (a resumed run continues where the data stood)"""
    if hasattr(batches, "__len__") and hasattr(batches, "__getitem__"):
        if len(batches) == 0:
            raise ValueError("TrainLoop: no batches")
        i = skip
        while True:
            yield batches[i % len(batches)]
            i += 1
    while True:
        got = False
        for b in batches:
            got = True
            if skip:
                skip -= 1
                continue
            yield b
        if not got:
            raise ValueError("TrainLoop: no batches")


class TrainLoop:
    """mmengine's IterBasedTrainLoop for a captured step: per iteration the next (images, segs) of `batches` (decoded uint8
    pictures and annotations; an iterable that is restarted when exhausted) -> `augment(images, segs, out=(step.static_in,
    step.static_seg))` -> `step()` (at world size > 1, where the step holds no optimizer: -> `step.red.reduce()` ->
    `optimizer.step()` -> `log.append()`) -> `scheduler.step()` -> the hooks.  With an optimizer built with `accumulative_counts=k`
    (handed to the step as well) the step accumulates, and updates every k-th iteration and after the last (train.GradAccum); at
    world size > 1 reduce, update and `accum.finish()` run here, only on the iterations that close a group: ONE all-reduce per k
    iterations.  The scheduler steps every iteration, as mmengine's ParamSchedulerHook does.  A run resumed inside a group raises
    (the partial group's gradients are in no file; mmengine only warns).  Nothing in an iteration reads the device; the log,
    validation and checkpoint iterations do (one `TrainLog.read()`, `step.check()`).  Every `val_interval` iterations and after the
    last, `validate()` -> a metric dictionary (a closure over `evaluate(...)`), handed to the hooks' `after_val`; the hooks'
    `before_val` runs ahead of it -- an `EMAHook` (optimizer built with `ema=...`) swaps the averaged weights in there and the
    training weights back in `after_val`, and the loop itself swaps back behind anything that raises in between.

    `hooks`: objects or the configs' dictionaries (`dict(type='LoggerHook', interval=50)`), run in ascending `priority`.
    `load_from`: a checkpoint whose weights are loaded before the first iteration; with `resume` also the optimizer, the scheduler,
    the augment generator and the iteration count (`resume=True` alone: the file `{work_dir}/last_checkpoint` names)."""

    def __init__(self, step, optimizer, scheduler, augment, batches, max_iters, val_interval=None, validate=None, hooks=(),
                 work_dir=None, load_from=None, resume=False, async_write=True):
        self.step, self.optimizer, self.scheduler, self.augment, self.batches = step, optimizer, scheduler, augment, batches
        self.max_iters, self.val_interval, self.validate = int(max_iters), val_interval, validate
        self.work_dir, self.load_from, self.resume = work_dir, load_from, bool(resume)
        self.rank, self.world = _rank_world()
        self.log = getattr(step, "log", None)
        self.firing = getattr(step, "firing", None)          # a firing.FiringLog the step appends a row to per replay
        self.grad_log = getattr(optimizer, "grad_log", None)          # a gradlog.GradLog `optimizer.step()` appends a row to
        self.seg_log = getattr(step, "seg_log", None)          # a seglog.SegLog the step appends a row to per replay
        self.match_log = getattr(step, "match_log", None)          # a matchlog.MatchLog the step appends a row to per replay
        self.accum = getattr(optimizer, "accum", None)          # a train.GradAccum: FlatAdamW(accumulative_counts=k), k > 1
        own = getattr(step, "optimizer", None)
        if self.accum is not None and own is not optimizer:
            raise ValueError("TrainLoop: an optimizer with accumulative_counts > 1 has to be the step's own (optimizer=...): "
                             "the step accumulates behind its packing")
        # what graph.step_tail leaves to the caller: `step.red.reduce()`, `optimizer.step()` (`accum.finish()`), the log's row behind them
        update, row = step_tail(own is not None, self.accum is not None, self.world)
        if self.accum is None and hasattr(step, "log_captured"):          # (a step says itself whether its graph holds the row)
            row = "graph" if step.log_captured else "caller"
        self.eager_update = update == "caller" and (own is not None or hasattr(step, "red"))
        self.eager_append = self.log is not None and row == "caller"
        # the ring logs a LoggerHook reports, in the line's order: (log, the map from its row number to the iteration of that row)
        self.logs = [(log, of) for log, of in ((self.firing, int), (self.grad_log, self.update_iteration), (self.seg_log, int),
                                               (self.match_log, int)) if log is not None]
        if self.eager_append:
            self.log.bind({**step.log_terms, "grad_norm": optimizer.grad_norm, "clip_coef": optimizer.clip_coef})
        self.state = TrainState(step.model, optimizer, scheduler, augment, async_write=async_write)
        built = [HOOKS.build(h) if isinstance(h, dict) else h for h in hooks]
        self.hooks = sorted(built, key=lambda h: getattr(h, "priority", 50))
        self.iter, self.lr, self.resumed, self.val_metrics = 0, None, None, None
        self._read = (None, None)

    def _call(self, name, *args):
        for h in self.hooks:
            fn = getattr(h, name, None)
            if fn is not None:
                fn(self, *args)

    def meta(self):
        return dict(iter=self.iter + 1, max_iters=self.max_iters)

    def update_iteration(self, updates):
        """the iteration (from 1) whose update was the `updates`-th (from 1): every accumulative_counts-th, and the last one"""
        return updates if self.accum is None else min(updates * self.accum.counts, self.max_iters)

    def updates_done(self, n):
        """the updates of the first `n` iterations: one per closed group, the run's last iteration closes its own"""
        if self.accum is None:
            return n
        return n // self.accum.counts + (1 if n == self.max_iters and n % self.accum.counts else 0)

    def check_finite(self):
        """-> the log as of this iteration (read once per iteration, whoever asks), after raising for what went wrong on the device
        since the last look: FloatingPointError naming the FIRST iteration with a non-finite term, carrying the step's own status
        error (`step.check()`: a label outside the classes, non-finite matching costs) where that is the cause."""
        if self._read[0] == self.iter:
            return self._read[1]
        read = self.log.read() if self.log is not None else None
        bad = None if read is None or read.first_nonfinite is None else self.log.base + read.first_nonfinite + 1
        try:
            if hasattr(self.step, "check"):
                self.step.check()
        except Exception as e:
            if bad is None:
                raise
            raise FloatingPointError(f"non-finite training terms first at iteration {bad}: {e}") from e
        if bad is not None:
            row = self.log.base + read.count - len(read.rows)
            seen = ""
            if row < bad <= row + len(read.rows):
                vals = read.rows[bad - 1 - row]
                seen = ": " + ", ".join(f"{k} = {v}" for k, v in zip(read.names, vals) if not np.isfinite(v))
            where = ""
            first = self.grad_log.read(consume=False).first_nonfinite if self.grad_log is not None else None
            if first is not None:          # the tensor it started in: the lowest parameter of the first row with a non-finite gradient
                where = (f"; the first non-finite gradient is in {first[1]}, iteration "
                         f"{self.update_iteration(self.grad_log.base + first[0] + 1)}")
            raise FloatingPointError(f"non-finite training terms first at iteration {bad}{seen}; checkpoints up to iteration "
                                     f"{bad - 1} predate it{where}")
        self._read = (self.iter, read)
        return read

    def _validate(self):
        self.check_finite()
        model = self.step.model
        training = getattr(model, "training", None)
        watching = self.firing is not None and self.firing.attached
        if watching:
            self.firing.detach()          # a validation forward's spikes are not the next iteration's
        ema = getattr(self.optimizer, "ema", None)
        try:
            try:
                self._call("before_val")          # (an EMAHook swaps the averaged weights in; hooks without the method are passed over)
                metrics = self.validate()
            finally:
                if watching:
                    self.firing.attach()          # (the same counters at the same addresses: the captured launches still hold)
            if training:
                model.train()
            self.val_metrics = metrics
            self._call("after_val", metrics)          # (the EMAHook swaps back, ahead of the logger and the checkpoint)
        finally:
            if ema is not None and ema.swapped:
                ema.restore()          # whatever was raised above, the next iteration trains the training weights

    def run(self):
        start = 0
        try:
            path = self.load_from
            if self.resume and path is None:
                with open(os.path.join(self.work_dir, "last_checkpoint")) as f:
                    path = f.read().strip()
            if path is not None:
                self.resumed = self.state.load(path, resume=self.resume)
                if self.resume:
                    start = int(self.resumed["meta"]["iter"])
            self.iter = start
            counts = 1 if self.accum is None else self.accum.counts
            if self.accum is not None:
                if start % counts:
                    raise ValueError(f"TrainLoop: resumed at iteration {start}, inside a group of accumulative_counts={counts}: the "
                                     f"group's gradients are in no checkpoint")
                self.accum.total, self.accum.count = self.max_iters, start
            for log in (self.log, self.firing, self.grad_log, self.seg_log, self.match_log):          # (no ring is in a checkpoint: a resumed run starts them afresh)
                if log is not None:
                    log.rebase(start, counts if log is self.grad_log else 1)          # (the gradient log's rows count updates)
            self._call("before_run")
            batches = _cycle(self.batches, start)
            out = (self.step.static_in, self.step.static_seg)
            for it in range(start, self.max_iters):
                self.iter = it
                images, segs = next(batches)
                self.augment(images, segs, out=out)
                self.step()
                if self.eager_update and (self.accum is None or self.accum.plan(it)[2]):
                    self.step.red.reduce()
                    self.step.red.wait()
                    self.optimizer.step()
                    if self.accum is not None:
                        self.accum.finish()
                if self.eager_append:
                    self.log.append()
                self.lr = self.optimizer.param_groups[0]["lr"]          # this iteration's: the scheduler moves on below
                self.scheduler.step()
                self._call("after_train_iter")
                n = it + 1
                if self.validate is not None and ((self.val_interval and n % self.val_interval == 0) or n == self.max_iters):
                    self._validate()
            self._call("after_run")
        finally:
            self.state.close()
        return self.val_metrics
