"""The thin training driver around the hot path -- SURVEY section 8 row f2: what mmengine's runner does per iteration for
the Spike2Former configs (configs/Spike2Former/SDTv2_maskformer_DCNpixelDecoder_ade20k.py:137-167), without the runner:

    ResetModelHook -> data_preprocessor(training=True) -> model(mode='loss') -> parse_losses -> backward ->
    [all-reduce] -> clip_grad(max_norm=0.01) -> AdamW(paramwise lr / decay multipliers) -> LinearLR -> PolyLR

mmengine itself is not part of the reference tree (third-party, mmengine 0.8.4 per Seg/README.md:25): `parse_losses`,
the `custom_keys` rule of DefaultOptimWrapperConstructor and the two schedulers are restated from its published behaviour;
parity is pinned by the config's own values only.  The reference's optimiser is torch.optim.AdamW behind clip_grad_norm_;
`OptimWrapper` runs exactly that (eager, one group per parameter), `FlatAdamW` is the same update as three HIP launches over
the flat gradient buffer of the data-parallel step (csrc/optim.hip), pinned against the former in tests/test_gpu_round5.py.
Both take mmengine's `accumulative_counts`: `GradAccum` adds micro-batch gradients up on the flat buffer (one launch each),
`OptimWrapper` does it the way mmengine does, through autograd (tests/test_gpu_grad_accum.py compares the two)."""
import torch

from .neuron import reset_net


def parse_losses(losses):
    """mmengine BaseModel.parse_losses: tensors -> mean, lists -> sum of means; the step's loss = sum of the entries whose
    key contains 'loss'.  -> (loss, log_vars)"""
    log_vars = {}
    for k, v in losses.items():
        if torch.is_tensor(v):
            log_vars[k] = v.mean()
        elif isinstance(v, (list, tuple)):
            log_vars[k] = sum(t.mean() for t in v)
        else:
            raise TypeError(f"{k} is not a tensor or list of tensors")
    loss = sum(v for k, v in log_vars.items() if "loss" in k)
    log_vars = {"loss": loss, **log_vars}
    return loss, log_vars


def param_groups(model, lr, weight_decay, paramwise_cfg=None):
    """One group per parameter, DefaultOptimWrapperConstructor's `custom_keys` rule: the longest key (ties: alphabetical)
    that is a substring of the parameter's full name sets `lr_mult` / `decay_mult`."""
    custom = dict((paramwise_cfg or {}).get("custom_keys", {}))
    keys = sorted(sorted(custom.keys()), key=len, reverse=True)
    groups = []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        g = {"params": [p], "lr": lr, "weight_decay": weight_decay, "name": name}
        for k in keys:
            if k in name:
                g["lr"] = lr * custom[k].get("lr_mult", 1.0)
                g["weight_decay"] = weight_decay * custom[k].get("decay_mult", 1.0)
                break
        groups.append(g)
    return groups


def _multipliers(names, paramwise_cfg):
    """DefaultOptimWrapperConstructor's `custom_keys` rule per parameter name -> [(lr_mult, decay_mult)]"""
    custom = dict((paramwise_cfg or {}).get("custom_keys", {}))
    keys = sorted(sorted(custom.keys()), key=len, reverse=True)
    out = []
    for name in names:
        lm, dm = 1.0, 1.0
        for k in keys:
            if k in name:
                lm, dm = custom[k].get("lr_mult", 1.0), custom[k].get("decay_mult", 1.0)
                break
        out.append((lm, dm))
    return out


def accumulation_plan(i, counts, total=None):
    """mmengine 0.8.4 OptimWrapper's gradient accumulation rule (`accumulative_counts`, `should_update`, `_get_loss_factor` after
    `initialize_count_status(model, 0, total)`), restated: iteration `i` (from 0) of a run of `total` iterations (None: unknown, no
    trailing group) -> (scale, first, last).  Groups are counted from iteration 0; `first` opens a group, `last` closes it (the
    update follows); `scale` multiplies the micro-batch's gradient: 1 / counts, and 1 / (total % counts) in the trailing partial
    group, the iterations >= total - total % counts when counts does not divide total."""
    first = i % counts == 0
    last = (i + 1) % counts == 0 or (total is not None and i + 1 == total)
    scale = 1.0 / counts
    if total is not None and total % counts and i >= total - total % counts:
        scale = 1.0 / (total % counts)
    return scale, first, last


class GradAccum:
    """mmengine's `OptimWrapper(accumulative_counts=k)` on the flat gradient buffer: the gradients of k micro-batches are added up,
    then ONE clip and ONE AdamW step follow.  The accumulator is a second flat buffer of `grad_buffer.flat`'s layout; `add()` is
    one streaming launch (s2f_grad_accumulate, csrc/optim.hip) behind the step's packing:

        not the group's last iteration:  acc = [acc +] scale * flat            (and the micro-batch's g^2 partials, row i % k)
        the group's last iteration:      flat = acc + scale * flat             -> `grad_buffer.flat` holds the accumulated MEAN gradient:
                                         reduce(), FlatAdamW.step() and GradLog read the buffer they always read

    `finish()`, directly behind `FlatAdamW.step()`: one launch (s2f_grad_accum_stats) turns the micro partials of the group just
    closed and the optimizer's own partials (s2f_grad_sqnorm of the accumulated gradient, written inside step()) into
    `stats` = {mean micro-batch |g|^2, |accumulated g|^2, micro-batches, 0}: the two terms of the gradient-noise-scale estimate
    (runner.LoggerHook).  Rows of `micro` hold |g|^2 of the UNSCALED micro-batch gradient.

    `count`: the iterations done (host; set it for a resumed run), `total`: the run's max_iters or None -- what `plan()` needs.
    mmengine is not part of the reference tree: the rule is restated from mmengine 0.8.4's OptimWrapper and, like the schedulers',
    its parity is UNPINNED.  Stated deviation: mmengine scales the LOSS before backward, here the finished gradient is scaled --
    fp32 round-off apart the same, and exactly the same for power-of-two counts."""

    def __init__(self, grad_buffer, counts, total=None):
        from ._lib import lib
        counts = int(counts)
        if counts < 1:
            raise ValueError(f"GradAccum: accumulative_counts {counts} below 1")
        self.red, self.counts, self.total, self.count = grad_buffer, counts, total, 0
        flat = grad_buffer.flat
        self.acc = torch.zeros_like(flat)
        self.parts = int(lib.s2f_grad_sqnorm_parts(flat.numel()))
        self.micro = torch.zeros(counts, self.parts, dtype=torch.float64, device=flat.device)
        self.stats = torch.zeros(4, dtype=torch.float32, device=flat.device)
        self._rows = counts          # the micro-batches of the group closed last
        self._layout = self._layout_now()
        self.partials = None         # the optimizer's s2f_grad_sqnorm partials (FlatAdamW sets it)

    def _layout_now(self):
        return tuple(getattr(self.red, "offsets", ())), tuple(id(p) for p in getattr(self.red, "params", ()))

    def plan(self, i):
        return accumulation_plan(i, self.counts, self.total)

    @property
    def open(self):
        """whether a group is under way (gradients in the accumulator that no update has consumed)"""
        return self.count % self.counts != 0 and self.count != self.total

    def add(self):
        """-> whether this iteration closed its group (the caller updates).  One launch, no wait."""
        from ._lib import check, lib
        from .ops.core import _stream
        flat = self.red.flat
        if flat.numel() != self.acc.numel() or self._layout_now() != self._layout:
            raise RuntimeError("GradAccum: the gradient buffer was laid out again (compact()); call rebuild()")
        scale, first, last = self.plan(self.count)
        row = self.count % self.counts
        check(lib.s2f_grad_accumulate(flat.data_ptr(), None if first else self.acc.data_ptr(),
                                      (flat if last else self.acc).data_ptr(), flat.numel(), scale,
                                      self.micro[row].data_ptr(), _stream()), "s2f_grad_accumulate")
        if last:
            self._rows = row + 1
        self.count += 1
        return last

    def finish(self, partials=None):
        """directly behind `FlatAdamW.step()`.  `partials`: the optimizer's (FlatAdamW.partials, which FlatAdamW hands over when it
        builds the accumulator), as its step() on the accumulated gradient just left them"""
        from ._lib import check, lib
        from .ops.core import _stream
        partials = self.partials if partials is None else partials
        if partials is None or partials.numel() != self.parts or partials.dtype != torch.float64:
            raise ValueError(f"GradAccum.finish needs the optimizer's {self.parts} fp64 partials")
        check(lib.s2f_grad_accum_stats(self.micro.data_ptr(), self._rows, partials.data_ptr(), self.parts, self.stats.data_ptr(),
                                       _stream()), "s2f_grad_accum_stats")

    def rebuild(self):
        """after grad_buffer.compact(): a new accumulator in the new layout.  Only at a group boundary: between updates the old
        one holds gradients whose slots moved."""
        if self.open:
            raise RuntimeError(f"GradAccum.rebuild inside a group (iteration {self.count}, accumulative_counts {self.counts})")
        self.acc = torch.zeros_like(self.red.flat)
        self._layout = self._layout_now()


class FlatAdamW:
    """clip_grad_norm_(max_norm) + AdamW over `dist.FlatGradAllReduce`'s flat gradient buffer: three HIP launches per iteration
    (s2f_grad_sqnorm -> s2f_adamw_prepare -> s2f_adamw_step), no host synchronisation -- `step()` can be captured behind the
    step's hipGraph (graph.GraphedStep(optimizer=...)) or called eagerly after the all-reduce when N > 1.

    What mmengine's OptimWrapper does for the config (configs/Spike2Former/SDTv2_maskformer_DCNpixelDecoder_ade20k.py:137-155) with
    ~1 000 single-parameter groups: gradients are read where the step packed (and the all-reduce averaged) them, both moments
    are flat buffers of the same layout, parameters are addressed through a pointer table (they stay where their modules own
    them).  `param_groups` is a list of {'lr', 'weight_decay', 'name'} dictionaries, one per parameter, that a scheduler
    (LinearThenPoly) may rewrite between iterations; the table goes to the device at the start of `step()`.
    Build it AFTER `grad_buffer.compact()`: the tables follow the buffer's layout (checked at every step).

    `grad_log`: None (default: the step is the three launches above, nothing else is allocated or launched), True or a dictionary of
    `gradlog.GradLog` arguments (`dict(window=50, patience=200)`): `step()` appends one row of per-parameter gradient, weight and
    update norms directly behind s2f_adamw_step, two launches more that only read (`self.grad_log`; `attach_grad_log` takes a log
    built by the caller).

    `accumulative_counts` (mmengine's OptimWrapper argument): 1 (default) -- `self.accum` is None, nothing is allocated, the class is
    what it is without the argument; k > 1 -- `self.accum = GradAccum(grad_buffer, k)`: whoever drives the step calls
    `accum.add()` behind the packing of EVERY iteration and `step(); accum.finish()` behind the one that closes a group
    (graph.GraphedStep / GraphedHungarianStep and runner.TrainLoop do).

    `ema`: None (default: `self.ema` is None, nothing is allocated or launched), True or a dictionary of `ema.WeightEMA` arguments
    (mmengine's EMAHook's: `dict(type='ExpMomentumEMA', momentum=0.0002, gamma=2000, begin_iter=...)`): `step()` records the
    average's ONE launch directly behind s2f_adamw_step, before the gradient log's -- captured with the update at world size 1,
    launched eagerly behind the all-reduce otherwise (no communication: every rank applies a deterministic function of identical
    weights).  With `accumulative_counts=k` the average moves once per update.  A step that was captured before holds the launches
    it was recorded with: the average cannot be attached afterwards (runner.EMAHook checks that it is there)."""

    def __init__(self, model, grad_buffer, lr=0.001, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.005, paramwise_cfg=None,
                 clip_grad=None, grad_log=None, accumulative_counts=1, ema=None):
        from ._lib import lib
        self.red, self.betas, self.eps = grad_buffer, (float(betas[0]), float(betas[1])), float(eps)
        self.max_norm = float((clip_grad or {}).get("max_norm", 0.0)) if clip_grad else 0.0
        if clip_grad and clip_grad.get("norm_type", 2) != 2:
            raise NotImplementedError("FlatAdamW clips by the 2-norm (the Spike2Former configs' norm_type)")
        names = {id(p): n for n, p in model.named_parameters()}
        self.params = list(grad_buffer.params)
        mult = _multipliers([names.get(id(p), "") for p in self.params], paramwise_cfg)
        self.param_groups = [{"params": [p], "lr": lr * lm, "weight_decay": weight_decay * dm, "name": names.get(id(p), "")}
                             for p, (lm, dm) in zip(self.params, mult)]
        dev = grad_buffer.flat.device
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(grad_buffer.flat), torch.zeros_like(grad_buffer.flat)
        n = grad_buffer.flat.numel()
        self.partials = torch.zeros(int(lib.s2f_grad_sqnorm_parts(n)), dtype=torch.float64, device=dev)
        self.state = torch.zeros(8, dtype=torch.float32, device=dev)
        self._hyper_host = [torch.empty(len(self.params), 2, dtype=torch.float32) for _ in range(2)]
        if dev.type == "cuda":
            self._hyper_host = [h.pin_memory() for h in self._hyper_host]
        self._hyper_events, self._hyper_turn, self._hyper_last = [None, None], 0, None
        self.hyper = torch.zeros(len(self.params), 2, dtype=torch.float32, device=dev)
        self._build_tables()
        self.accum = None
        if int(accumulative_counts) != 1:
            self.accum = GradAccum(grad_buffer, accumulative_counts)          # (raises for a count below 1)
            self.accum.partials = self.partials
        self.ema = None
        if ema is not None and ema is not False:
            from .ema import WeightEMA
            self.ema = WeightEMA(self, **({} if ema is True else dict(ema)))
        self.grad_log = None
        if grad_log is not None and grad_log is not False:
            from .gradlog import GradLog
            self.attach_grad_log(GradLog(self, **({} if grad_log is True else dict(grad_log))))

    def attach_grad_log(self, log):
        """`log`: a gradlog.GradLog over THIS optimizer (None detaches); from the next `step()` on every update is followed by one row.
        A step that was captured before holds the launches it was recorded with: attach before building the captured step."""
        if log is not None and log.optimizer is not self:
            raise ValueError("FlatAdamW.attach_grad_log: the log was built over another optimizer")
        self.grad_log = log
        return log

    def _build_tables(self):
        from ._lib import lib
        chunk = int(lib.s2f_adamw_chunk_elems())
        dev = self.red.flat.device
        self._layout = (tuple(self.red.offsets), tuple(p.data_ptr() for p in self.params))
        slots, chunks = [], []
        for i, (p, off) in enumerate(zip(self.params, self.red.offsets)):
            if not p.is_contiguous():
                raise RuntimeError("FlatAdamW: parameters must be contiguous")
            slots.append((p.data_ptr(), off, p.numel()))
            chunks += [(i, s) for s in range(0, p.numel(), chunk)]
        self.slots = torch.tensor(slots, dtype=torch.int64).to(dev)
        self.chunks = torch.tensor(chunks, dtype=torch.int32).to(dev)

    def sync_hyper(self):
        """the per-parameter (lr, weight_decay) table of this iteration -> device.  Uploaded only when a scheduler changed a value,
        from one of TWO pinned tables in turn: the copy reads host memory when it EXECUTES, and the host may run several replays
        ahead -- the table a queued copy still has to read is never the one being rewritten (its event is waited for first)."""
        import numpy as np
        vals = np.array([(g["lr"], g["weight_decay"]) for g in self.param_groups], dtype=np.float32).reshape(-1, 2)
        for i in getattr(self.red, "missing", ()):
            vals[i, 0] = -1.0          # no gradient in the step just packed (p.grad is None): the kernel skips the parameter (optim.hip)
        if self._hyper_last is not None and np.array_equal(vals, self._hyper_last):
            return
        self._hyper_turn ^= 1
        host, ev = self._hyper_host[self._hyper_turn], self._hyper_events[self._hyper_turn]
        if ev is not None:
            ev.synchronize()
        host.copy_(torch.from_numpy(vals))
        self.hyper.copy_(host, non_blocking=True)
        if self.hyper.is_cuda:
            ev = torch.cuda.Event() if ev is None else ev
            ev.record()
            self._hyper_events[self._hyper_turn] = ev
        self._hyper_last = vals

    def mark_updated(self):
        """The kernels wrote the parameters behind autograd's back: bump their version counters so that every cache keyed on a
        weight's version (the bf16 term splits / packs of ops.gemm, the composed eval-mode BatchNorm affines of fused.py) re-converts
        at its next eager use.  step() does it itself when it runs eagerly; a REPLAY of a hipGraph that holds the update cannot
        (nothing of Python runs inside it): graph.GraphedStep / GraphedHungarianStep call this after every replay."""
        torch.autograd.graph.increment_version(self.params)

    def step(self, sync_hyper=True):
        """Gradients: `grad_buffer.flat` as the step left it (packed, averaged).  -> the gradient norm (device scalar)."""
        from ._lib import check, lib
        from .ops.core import _stream
        if ((tuple(self.red.offsets), tuple(p.data_ptr() for p in self.params)) != self._layout
                or [id(p) for p in self.red.params] != [id(p) for p in self.params]):
            raise RuntimeError("FlatAdamW: the gradient buffer's layout (compact()) or a parameter's storage changed since the tables "
                               "were built; call rebuild()")
        if sync_hyper:
            self.sync_hyper()
        flat, b1, b2 = self.red.flat, self.betas[0], self.betas[1]
        s = _stream()
        check(lib.s2f_grad_sqnorm(flat.data_ptr(), flat.numel(), self.partials.data_ptr(), s), "s2f_grad_sqnorm")
        check(lib.s2f_adamw_prepare(self.partials.data_ptr(), self.partials.numel(), self.max_norm, b1, b2, self.state.data_ptr(), s),
              "s2f_adamw_prepare")
        check(lib.s2f_adamw_step(self.slots.data_ptr(), self.hyper.data_ptr(), self.chunks.data_ptr(), self.chunks.shape[0],
                                 flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.state.data_ptr(),
                                 b1, b2, self.eps, s), "s2f_adamw_step")
        if self.ema is not None:
            self.ema.update()
        if self.grad_log is not None:
            self.grad_log.append()
        # the kernels wrote the parameters behind autograd's back: bump their version counters so that every cache keyed on a
        # weight's version (the bf16 term splits / packs of ops.gemm) re-converts in eager use; a captured step re-converts inside
        # the graph anyway (ops.resplit_all)
        if not torch.cuda.is_current_stream_capturing():
            self.mark_updated()
        return self.state[1]

    def rebuild(self):
        """after grad_buffer.compact(): re-lay the moments out with the buffer (values kept per parameter)"""
        old_off = dict(zip((id(p) for p in self.params), self._layout[0]))
        m, v = torch.zeros_like(self.red.flat), torch.zeros_like(self.red.flat)
        groups = {id(g["params"][0]): g for g in self.param_groups}
        for p, off in zip(self.red.params, self.red.offsets):
            o = old_off[id(p)]
            m[off:off + p.numel()] = self.exp_avg[o:o + p.numel()]
            v[off:off + p.numel()] = self.exp_avg_sq[o:o + p.numel()]
        self.exp_avg, self.exp_avg_sq = m, v
        self.params = list(self.red.params)
        self.param_groups = [groups[id(p)] for p in self.params]
        self._hyper_last = None                      # the table's row order changed with the buffer's layout: upload again
        self._build_tables()
        if self.accum is not None:
            self.accum.rebuild()                     # (only at a group boundary: raises inside a group)
        if self.ema is not None:
            self.ema.rebuild()                       # (the average follows the moments' layout, values kept per parameter)
        if self.grad_log is not None:
            self.grad_log.rebuild()                  # (its span table follows the slot table; its rows start afresh)

    @property
    def grad_norm(self):
        return self.state[1]

    @property
    def clip_coef(self):
        return self.state[0]

    def state_dict(self):
        """per-parameter moments by name + the step count (what torch.optim.AdamW.state_dict carries, keyed by name)"""
        out = {"step": int(self.state[4].item()), "state": {}}
        for g, p, off in zip(self.param_groups, self.params, self.red.offsets):
            out["state"][g["name"]] = {"exp_avg": self.exp_avg[off:off + p.numel()].view_as(p).clone(),
                                       "exp_avg_sq": self.exp_avg_sq[off:off + p.numel()].view_as(p).clone()}
        return out

    def load_state_dict(self, sd):
        self.state[4] = float(sd["step"])
        for g, p, off in zip(self.param_groups, self.params, self.red.offsets):
            st = sd["state"][g["name"]]
            self.exp_avg[off:off + p.numel()].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[off:off + p.numel()].copy_(st["exp_avg_sq"].reshape(-1))


class LinearThenPoly:
    """LinearLR(start_factor, begin=0, end=warmup) followed by PolyLR(eta_min, power, begin=warmup, end=total), by iteration:
    factor(t) multiplies every group's base lr."""

    def __init__(self, optimizer, warmup=1500, total=160000, start_factor=1e-6, eta_min=0.0, power=1.0):
        self.opt, self.warmup, self.total = optimizer, warmup, total
        self.start_factor, self.eta_min, self.power = start_factor, eta_min, power
        self.base = [g["lr"] for g in optimizer.param_groups]
        self.t = 0
        self._apply()

    def factor(self, t):
        if t < self.warmup:
            return self.start_factor + (1.0 - self.start_factor) * t / max(self.warmup - 1, 1) if self.warmup > 1 else 1.0
        # mmengine 0.8.4 PolyLR.__init__: total_iters = end - begin - 1; its recursive rule
        #   lr_t = (lr_{t-1} - eta_min) * (1 - 1 / (total_iters - s + 1))^power + eta_min,  s = t - begin = 1 .. total_iters
        # telescopes to (1 - s / total_iters)^power: the floor eta_min is reached at t = end - 1 and held
        span = max(self.total - self.warmup - 1, 1)
        return max(1.0 - min(t - self.warmup, span) / span, 0.0) ** self.power

    def _apply(self):
        f = self.factor(self.t)
        for g, b in zip(self.opt.param_groups, self.base):
            g["lr"] = self.eta_min + (b - self.eta_min) * f if self.t >= self.warmup else b * f

    def step(self):
        self.t += 1
        self._apply()


class OptimWrapper:
    """optimizer + clip_grad, as the config's `optim_wrapper` (:150-155).

    `accumulative_counts=k`: mmengine's own mechanics, the readable statement of what GradAccum does on the flat buffer --
    `update_params(loss)` scales the loss by the plan's factor (accumulation_plan) and runs backward, autograd adds into `p.grad`,
    and the clip, the step and zero_grad happen only where the plan says the group closes.  `initialize_count_status(total)`
    tells the plan where the run ends (the trailing partial group); `count` is the number of `update_params` calls so far.
    Restated from mmengine 0.8.4 (not part of the reference tree); parity UNPINNED."""

    def __init__(self, model, optimizer=None, clip_grad=None, paramwise_cfg=None, accumulative_counts=1):
        cfg = dict(optimizer or dict(type="AdamW", lr=0.001, betas=(0.9, 0.999), weight_decay=0.005))
        kind = cfg.pop("type", "AdamW")
        if kind != "AdamW":
            raise NotImplementedError(f"optimizer {kind}: the Spike2Former configs use AdamW")
        lr, wd = cfg.pop("lr"), cfg.pop("weight_decay", 0.0)
        self.optimizer = torch.optim.AdamW(param_groups(model, lr, wd, paramwise_cfg), lr=lr, weight_decay=wd, **cfg)
        self.clip = dict(clip_grad) if clip_grad else None
        self.params = [p for g in self.optimizer.param_groups for p in g["params"]]
        self.counts, self.count, self.total = int(accumulative_counts), 0, None
        if self.counts < 1:
            raise ValueError(f"OptimWrapper: accumulative_counts {self.counts} below 1")

    def initialize_count_status(self, total, count=0):
        """`total`: the run's max_iters; `count`: the iterations already done (a resumed run)"""
        self.total, self.count = total, int(count)

    def update_params(self, loss):
        """-> the gradient norm where an update happened (and a clip is configured), else None"""
        if self.counts == 1:
            loss.backward()
            return self.step()
        scale, _, last = accumulation_plan(self.count, self.counts, self.total)
        (loss * scale).backward()
        self.count += 1
        return self.step() if last else None

    def step(self):
        norm = None
        if self.clip:
            norm = torch.nn.utils.clip_grad_norm_(self.params, self.clip.get("max_norm", 0.01), self.clip.get("norm_type", 2))
        self.optimizer.step()
        self.optimizer.zero_grad(set_to_none=True)
        return norm


def train_step(model, data, optim_wrapper, scheduler=None):
    """One iteration: reset (ResetModelHook.before_train_iter) -> preprocess -> loss -> backward -> clip -> AdamW -> lr.
    `model` is an EncoderDecoder carrying a `data_preprocessor` (or data is already {'inputs': tensor, 'data_samples': ...}).
    -> log_vars (python floats) with 'grad_norm'."""
    reset_net(model)
    pre = getattr(model, "data_preprocessor", None)
    if pre is not None:
        data = pre(data, True)
    losses = model(data["inputs"], data["data_samples"], mode="loss")
    loss, log_vars = parse_losses(losses)
    norm = optim_wrapper.update_params(loss)
    if scheduler is not None:
        scheduler.step()
    out = {k: float(v) for k, v in log_vars.items()}
    if norm is not None:
        out["grad_norm"] = float(norm)
    return out
