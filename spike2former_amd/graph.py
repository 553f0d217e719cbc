"""hipGraph capture of the whole training step.

One C2 step issues ~5 000 kernel launches from Python; at ~20 us of host time per launch the step is host-bound long
before the GPU is busy.  Shapes are static (fixed crop, fixed T), so the step -- membrane reset, gradient-buffer clear,
forward, loss, backward -- is captured once into a hipGraph (torch.cuda.CUDAGraph on ROCm) and replayed: one host call
per step.  The kernels launched through the C ABI take the capture stream like any other launch; the ABI allocates
nothing and never synchronises, so it is capture-safe by construction (clears are fill KERNELS: no hipMemsetAsync nodes).

Weights: the spike GEMMs read bf16 hi / mid / lo terms of every weight that `ops.split_weight*` caches per weight version.
A captured step does not rely on that cache: `reset_net -> ops.begin_step` re-splits EVERY registered weight inside the
graph (ops.resplit_all, one launch over a pointer table), so each replay multiplies by the live fp32 weights -- an optimiser
step or load_state_dict between replays is honoured, forward and backward stay consistent
(tests/test_gpu_full_size.py::test_graph_replay_follows_weight_updates).  Weights that enter the model only after the
capture (none on this path) would need a new capture.

Every step class below is a `_Captured`: the capture protocol (`_capture`) and the replay prologue / epilogue (`_begin`,
`_end`) are written there once; a class says which warm-up pass it runs, which stages it records and what lies between them.

Inference is captured by the same protocol: `GraphedPredict` keeps one hipGraph per input shape of the stateless pass
`reset_net(model); model.encode_decode(x, metas)` and `CapturePolicy` (host arithmetic only) decides which shapes are worth one.
"""
import collections
import contextlib
import gc
import time
import weakref

import torch

from . import ops
from .neuron import reset_net, reset_state, resettable


def _process_group():
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized()


def _world_size():
    import torch.distributed as dist
    return dist.get_world_size() if _process_group() else 1


def step_tail(optimizer_in_step, accumulating, world):
    """Who runs what follows the gradient packing of a training step -> (update, row): the parameter update and the row of the
    step's log (runner.TrainLog), each "graph" (recorded into the step's last hipGraph), "call" (eager in the step's `__call__`,
    behind the replay) or "caller" (runner.TrainLoop, behind the step: beyond one rank the all-reduce lies before the update, and
    the row holds the update's grad_norm).  An accumulating optimizer (accumulative_counts > 1; always the step's own) updates on
    some calls only, so never inside the graph.  (optimizer handed to the step, accumulating, world) -> update, row:
        yes, no, 1   -> graph, graph         no, no, 1   -> caller, graph          yes, yes, 1   -> call, call
        yes, no, > 1 -> graph, caller        no, no, > 1 -> caller, caller         yes, yes, > 1 -> caller, caller"""
    if accumulating:
        return ("call", "call") if world == 1 else ("caller", "caller")
    return "graph" if optimizer_in_step else "caller", "graph" if world == 1 else "caller"


class _Captured:
    """A step with static input `static_in`, recorded as one hipGraph per stage.  `red`: the flat gradient buffer
    (dist.FlatGradAllReduce) of the steps that pack into one; `optimizer`: a train.FlatAdamW captured behind the packing."""
    optimizer = log = firing = seg_log = match_log = None

    def _tail(self):
        return step_tail(self.optimizer is not None, self.accum is not None, _world_size())

    @property
    def grad_log(self):
        """the captured optimizer's gradlog.GradLog (FlatAdamW(grad_log=...)): `optimizer.step()` appends its row behind the update,
        so the recorded stages hold its two launches without knowing of them; None: the capture is the one without them"""
        return getattr(self.optimizer, "grad_log", None)

    @property
    def accum(self):
        """the optimizer's train.GradAccum (FlatAdamW(accumulative_counts=k), k > 1) or None.  With one, the recorded stages end with
        the packing (plus the status and firing launches), and every call runs `_accumulate()` behind the replay, on the same stream."""
        return getattr(self.optimizer, "accum", None)

    def _update_in_graph(self):
        return self._tail()[0] == "graph"

    def _accumulate(self):
        """behind the last replay of a call, with an accumulating optimizer: `accum.add()`, then what `step_tail` gives to the "call"
        (world size 1; beyond, the caller runs reduce, update, `finish()` and the append): on the iteration that closes a group,
        `optimizer.step()` and `accum.finish()`, and on every call the log's row -- the loss terms of THIS iteration, and grad_norm,
        clip_coef, grad_sq_micro, grad_sq_accum as the last update left them (zeros before the first), as grad_norm repeats in
        mmengine's log.  Nothing here waits for the GPU.  -> whether the weights were updated."""
        update, row = self._tail()
        updated = self.accum.add() and update == "call"
        if updated:
            self.optimizer.step(sync_hyper=False)          # (`_begin` uploaded the table; eager: bumps the weight versions itself)
            self.accum.finish()
        if self.log is not None and row == "call":
            self.log.append()
        return updated

    def _after_capture(self):
        """once the capture has ended: the table the log's launch reads is uploaded (nothing may be while a capture records), and
        the firing, gradient, segmentation and match logs start afresh -- what the warm-up passes appended is not row 0"""
        if self.log is not None and self._tail()[1] != "caller":
            self.log.bind(self.log_terms)
        for ring in (self.firing, self.grad_log, self.seg_log, self.match_log):
            if ring is not None:
                ring.clear()

    def _capture(self, warm, warmup, stages, context=None):
        """`warmup` calls of `warm` on a side stream (allocator pools, lazy inits, caches), then each callable of `stages`
        recorded into a hipGraph of its own -> the graphs, in that order.  `context`: a context manager factory that changes
        the launch structure; every stage is recorded under it, after one more warm-up pass under it."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                warm()
            if context is not None:
                with context():
                    warm()
        torch.cuda.current_stream().wait_stream(side)
        # Warm-up gradients are not packed: drop their deferred launches.  A pass that ends without ops.wgrad_join() leaves
        # them queued, and inside a capture the drop of `red.zero()` is a no-op: the recorded join would launch them into the
        # graph, over warm-up tensors that are freed by the time it replays.
        ops.wgrad_drop()
        ops.resplit_all(self.static_in.device)          # builds the weight-split job table the captured step replays
        torch.cuda.synchronize()
        # With a process group alive, RCCL's watchdog thread polls its events while this thread captures: "thread_local"
        # keeps its (legal, uncaptured) calls from invalidating the capture; single-process runs keep the strict default.
        mode = "thread_local" if _process_group() else "global"
        pool = torch.cuda.graph_pool_handle() if len(stages) > 1 else None          # a later stage reads an earlier one's tensors
        graphs = [torch.cuda.CUDAGraph() for _ in stages]
        for graph, stage in zip(graphs, stages):
            with torch.cuda.graph(graph, pool=pool, capture_error_mode=mode), (context or contextlib.nullcontext)():
                stage()
        torch.cuda.synchronize()
        # the graphs bake in the addresses of the conversion job tables and of every cached split / pack buffer: hold them (an
        # eager forward after an optimiser step re-converts INTO the same buffers, ops/wcache.py, and replaces tables)
        self._converted = ops.conversion_state()
        # ... and the launch structure the op-layer switches selected (ops.cfg): see _begin
        self._settings = ops.cfg.launch_snapshot()
        return graphs

    def _begin(self, x):
        """Before a replay.  Replaying under other op-layer settings than the captured ones would mix two configurations
        silently -- e.g. eager steps of a comparison running with a switch flipped while the graph still replays the old
        kernels.  The optimizer's per-parameter (lr, weight_decay) table is uploaded (a scheduler may have rewritten it)."""
        now = ops.cfg.launch_snapshot()
        if now != self._settings:
            diff = {k: (self._settings[k], now[k]) for k in now if now[k] != self._settings.get(k)}
            raise RuntimeError(f"this hipGraph was captured under different op-layer settings (captured, now): {diff}; re-capture")
        if x is not None:
            self.static_in.copy_(x, non_blocking=True)
        if self.optimizer is not None:
            self.optimizer.sync_hyper()

    def _end(self):
        """After the last replay of a step (with an accumulating optimizer: `_accumulate()` takes its place, and the versions are
        bumped only behind an update).  A replayed update changed every weight after this replay's own re-split ran (at
        its START): the version-keyed conversion caches now hold the terms of the weights BEFORE the update under unchanged
        version counters -- an eager forward (validation, predict(), export) would multiply by one-step-stale bf16 terms.
        Bump the versions."""
        if self.accum is not None:
            self._accumulate()          # (its `optimizer.step()` runs eagerly and bumps the versions itself, behind an update only)
        elif self.optimizer is not None:
            self.optimizer.mark_updated()

    def _record_log(self, terms):
        """while the LAST stage is recorded, behind the optimizer's update: one row of `terms` ({name: static scalar}, plus this
        iteration's grad_norm and clip_coef of a captured optimizer) per replay into `self.log` (runner.TrainLog).  The launch
        reads the scalars through a pointer table that `_after_capture` fills."""
        if self.optimizer is not None:
            terms = {**terms, "grad_norm": self.optimizer.grad_norm, "clip_coef": self.optimizer.clip_coef}
        if self.accum is not None:
            terms = {**terms, "grad_sq_micro": self.accum.stats[0:1], "grad_sq_accum": self.accum.stats[1:2]}
        self.log_terms = terms
        # (a row that is the caller's: runner.TrainLoop also binds the optimizer's terms; the call's: `_accumulate`)
        self.log_captured = self._tail()[1] == "graph"
        if self.log_captured:
            self.log.declare(terms.keys())
            self.log.append()

    def _watch_firing(self, forward):
        """before the warm-up passes: every neuron counts into `self.firing` (firing.FiringLog) from here on -- which changes the
        launch structure: the memoised, pre-fired and fused-neuron routes step aside for a neuron with counters -- and one
        `forward()` tells the log which neurons the step runs, and over how many elements."""
        if self.firing is not None:
            self.firing.attach()
            with torch.no_grad():
                self.firing.measure(forward)

    def _record_firing(self):
        """while the LAST stage is recorded, as its last launch: one row of every neuron's counters per replay, at every world
        size (the forward is inside the graph on every rank; each rank logs its own shard)"""
        if self.firing is not None:
            self.firing.append()

    def _forward(self):
        reset_net(self.model)
        self.red.zero()
        return tuple(self.model(self.static_in))

    def _grads(self, outputs, grad_outputs=None):
        grads = torch.autograd.grad(outputs, self.red.params, grad_outputs, allow_unused=True)
        ops.wgrad_join()                  # side-stream (ops.WGRAD_STREAM) and deferred weight gradients are in their sinks
        return grads


class GraphedStep(_Captured):
    """`optimizer` (train.FlatAdamW over `grad_buffer`): the parameter update -- clip + AdamW, three launches -- is captured behind
    the gradient packing, so one replay is one training ITERATION (single process; with N > 1 the all-reduce sits between the step
    and the update, which the caller then runs eagerly: `step(); grad_buffer.reduce(); optimizer.step()`).  `log` (runner.TrainLog):
    every replay appends {loss, grad_norm, clip_coef} to it, at the end of the graph; None: the capture holds no such launch.
    `firing` (firing.FiringLog): see GraphedHungarianStep.  `step_tail` is the table of who updates and who appends the log's row
    (`log_captured`: the graph does), at every world size and for an optimizer built with `accumulative_counts=k`."""

    def __init__(self, model, loss_fn, example_input, grad_buffer=None, warmup=3, optimizer=None, log=None, firing=None):
        self.model, self.loss_fn, self.log, self.firing = model, loss_fn, log, firing
        self.static_in = example_input.clone()
        self.grad_buffer = grad_buffer
        self.optimizer = optimizer
        if optimizer is not None:
            optimizer.sync_hyper()

        def record():
            self.static_loss = self._eager_step()
            if self.log is not None:
                self._record_log({"loss": self.static_loss})
            self._record_firing()
        self._watch_firing(lambda: (reset_net(self.model), self.model(self.static_in)))
        # ops.GLUE_MODE: the residual aten calls of the step (autograd's gradient accumulation, scalar multiples, copies, fills, small
        # sums) are routed to csrc/glue.hip while the step is RECORDED -- the replay then consists of this package's kernels only
        self.graph, = self._capture(self._eager_step, warmup, [record], context=ops.glue_mode if ops.GLUE_MODE else None)
        self._after_capture()

    def _eager_step(self):
        reset_net(self.model)
        if self.grad_buffer is not None:
            self.grad_buffer.zero()
        else:
            for p in self.model.parameters():
                p.grad = None
        out = self.model(self.static_in)
        loss = self.loss_fn(*out)
        loss.backward()
        ops.wgrad_join()                  # side-stream weight gradients (ops.WGRAD_STREAM) rejoin before packing
        if self.grad_buffer is not None:
            self.grad_buffer.gather()
        if self._update_in_graph():
            self.optimizer.step(sync_hyper=False)
        return loss.detach()

    def __call__(self, x=None):
        self._begin(x)
        self.graph.replay()
        self._end()
        return self.static_loss


class GraphedSplitStep(_Captured):
    """The training step with a loss that needs the host in the middle (the Hungarian assignment):
    TWO hipGraphs around an eager loss --
        graph A : membrane reset + gradient-buffer clear + model forward           (autograd recorded once, at capture)
        eager   : loss(outputs.detach()) and its backward -> d loss / d outputs
        graph B : backward of graph A's recorded autograd graph from those gradients + packing into the flat buffer
    The same construction as torch.cuda.make_graphed_callables, but the parameter gradients never leave the graph as
    per-parameter tensors (that path clones 1 200 gradients per step: 79 ms/step, no better than eager launches).
    No autograd graph of an earlier eager step may be alive when this is built (drop the old outputs / losses first): its
    gradient accumulators belong to the default stream, the capture would have to wait on it, and ROCm 7.2 crashes in
    hipStreamEndCapture instead of reporting the illegal dependency."""

    def __init__(self, model, example_input, grad_buffer, warmup=3):
        self.model, self.red = model, grad_buffer
        self.static_in = example_input.clone()

        def warm():
            outs = self._forward()
            self._grads(outs, [torch.ones_like(o) for o in outs])

        def graph_a():
            self.outs = self._forward()

        def graph_b():
            # static inputs of this graph, from its pool (an allocation, no launch): backward() fills every one before a replay
            self.grad_outs = [torch.empty_like(o) for o in self.outs]
            self.red.pack(self._grads(self.outs, self.grad_outs))
        self.graph_a, self.graph_b = self._capture(warm, warmup, [graph_a, graph_b])

    def forward(self, x=None):
        """-> the model outputs (static tensors, valid until the next forward), detached leaves that require grad."""
        self._begin(x)
        self.graph_a.replay()
        return [o.detach().requires_grad_(True) for o in self.outs]

    def backward(self, leaves):
        """`leaves`: what forward() returned, after loss.backward() has filled their .grad."""
        for buf, leaf in zip(self.grad_outs, leaves):
            if leaf.grad is None:
                buf.zero_()
            else:
                buf.copy_(leaf.grad)
        self.graph_b.replay()


class GraphedHungarianStep(_Captured):
    """The REAL training step (Hungarian-matched loss on semantic maps) as two hipGraphs around the one
    thing that has to happen on the host, the assignment:
        graph A : membrane reset + gradient-buffer clear + model forward + matching costs against every class id
                  (loss.MaskFormerLoss.costs_all_classes) + their copy into pinned host memory
        host    : scipy linear_sum_assignment per (layer, image) on the columns of the classes present -> three small tables
                  (loss.MaskFormerLoss.match_tables), uploaded into static device buffers
        graph B : the losses from the tables (loss_from_tables: every shape is independent of the matching) + backward of the
                  whole model + packing of the gradients into the flat buffer (+ `optimizer`'s update, see GraphedStep)
    Between the graphs the GPU idles for the copy, the assignment and one upload -- not for ~450 eager launches of the loss and
    its backward as with GraphedSplitStep.  `__call__` returns the loss dictionary (static tensors, valid until the next call).

    assign="device": the assignment is a kernel of the step (ops.lsa_tables, csrc/lsa.hip: the same solver, fp64, one wave per
    (layer, image)) and the host stop disappears --
        single process : ONE hipGraph  reset + clear + forward + costs + assignment + losses + backward + packing (+ update);
        process group  : graph A (... + assignment), at world size > 1 the `num_masks` all-reduce queued on the step's stream,
                         graph B (losses ...) -- as the host route, without its synchronisation, copies and uploads.
    `__call__` then never waits for the GPU.  What the host route raises for (a label >= num_classes in the map, non-finite costs)
    arrives as a status word: every replay ORs the kernel's word into a STICKY device word and copies that to pinned memory at the
    end of the last graph, so a later replay on clean inputs cannot erase it.  `check()` synchronises and raises; `__call__` raises,
    before it touches the static inputs, when the word an earlier replay left has landed (a copy still in flight is seen on a
    later call or by `check()`).  Raising clears the word (the error path waits for the stream).  A step with a set status has NaN
    losses (the kernel writes num_masks = NaN), never quietly wrong ones -- and, with a captured optimizer, has already applied
    them: validate label maps before training on them.

    `log` (runner.TrainLog): the last graph ends with one more launch that appends every entry of the loss dictionary, their sum
    `loss` and, with a captured optimizer, its grad_norm and clip_coef to a ring on the device -- the record of EVERY iteration,
    and of the first one with a non-finite term, that runner.LoggerHook reads once per log interval.  None: the capture is the
    one without it.

    `firing` (firing.FiringLog over `model`): every neuron counts its spikes into the log's counters, and the last graph ends with
    one launch that turns them into a row per replay -- per-neuron firing rates of EVERY iteration, and the first neuron that stays
    silent for the log's `patience` iterations, read by runner.LoggerHook with the losses.  Counters change the launch structure of
    the step (the memoised, pre-fired and fused-neuron routes step aside for a neuron that has them); None: nothing is attached,
    allocated or launched, the capture is the one without it.  (An accumulating optimizer: see GraphedStep and `step_tail`.)

    `seg_log` (seglog.SegLog): the last graph ends with two more launches that score the step's own outputs -- the class scores and
    mask logits of the scored decoder layers, detached -- against `static_seg` at the mask resolution and append the per-class areas
    of intersect_and_union to a ring: train-crop accuracy and mIoU of EVERY iteration (a micro-batch, with an accumulating
    optimizer), read by runner.LoggerHook with the losses; in the one-graph and the two-graph forms alike, and at every world size
    (each rank scores its own crops).  None: nothing is allocated, launched or captured.

    `match_log` (matchlog.MatchLog): behind the assignment and behind `seg_log`, the last graph ends with two more read-only launches
    that turn the assignment's `row_class`, the costs it read and the class scores into one row of figures per replay -- matched
    pairs and their cost, greedy and moved shares, DETR's class_error, unmatched queries that claim an object, the usage of every
    query -- for all decoder layers, read by runner.LoggerHook with the losses; on both `assign` routes (two graphs: in graph B,
    after the tables' upload).  With it the step HOLDS the tensors of `_costs()` as `match_inputs = (cost, count)`, like `outs`:
    the pool must not hand their memory out again before the log's launches have read it, and a caller can read exactly what the
    kernel read.  None: nothing is allocated, held, launched or captured."""

    def __init__(self, model, example_input, example_seg, grad_buffer, warmup=3, ignore_index=None, optimizer=None, assign="host",
                 log=None, firing=None, seg_log=None, match_log=None):
        if assign not in ("host", "device"):
            raise ValueError(f"assign must be 'host' or 'device', got {assign!r}")
        if assign == "device" and not (example_input.is_cuda and example_seg.is_cuda):
            raise RuntimeError("GraphedHungarianStep(assign='device') needs CUDA tensors: the device assignment is a HIP kernel and "
                               "has no host fall-back")
        self.assign, self.log, self.firing, self.seg_log, self.match_log = assign, log, firing, seg_log, match_log
        head = model.decode_head
        self.optimizer = optimizer
        if optimizer is not None:
            optimizer.sync_hyper()
        self.model, self.red, self.crit = model, grad_buffer, head.criterion
        self.ignore_index = head.ignore_index if ignore_index is None else ignore_index
        self.static_in = example_input.clone()
        self.static_seg = self.crit.seg_as_u8(example_seg, self.ignore_index).clone()
        dev = example_input.device
        self._watch_firing(self._forward)
        with torch.no_grad():                                     # shapes of the outputs (and a first warm-up)
            cls, masks = self._forward()
        if not self.crit.semantic_ok(masks, self.static_seg):
            raise RuntimeError("GraphedHungarianStep needs semantic maps at twice the mask predictions' resolution")
        L, B, Q = cls.shape[:3]
        if seg_log is not None:
            if seg_log.K != self.crit.num_classes:
                raise ValueError(f"GraphedHungarianStep: a SegLog of {seg_log.K} classes on a head of {self.crit.num_classes}")
            seg_log.bind(L, B, Q, *masks.shape[-2:], device=dev)
        if match_log is not None:
            match_log.bind(L, B, Q, self.crit.num_classes, device=dev)
        del cls, masks
        self.tgt_labels = torch.full((L, B, Q), self.crit.num_classes, dtype=torch.int64, device=dev)
        self.row_class = torch.full((B, L * Q), -1, dtype=torch.int32, device=dev)
        self.num_masks = torch.ones(L, dtype=torch.float32, device=dev)
        if assign == "device":                                    # no pinned cost buffer: a status word instead
            self.status = torch.zeros(1, dtype=torch.int32, device=dev)
            self.sticky = torch.zeros(1, dtype=torch.int32, device=dev)          # OR of the status words since the last raise
            self.host_status = torch.zeros(1, dtype=torch.int32).pin_memory()
        else:
            self.host_cost = torch.empty(L, B, Q, self.crit.num_classes, dtype=torch.float32).pin_memory()
            self.host_count = torch.empty(B, 256, dtype=torch.float32).pin_memory()
            self.host_tgt, self.host_rows, self.host_avg = (torch.empty(t.shape, dtype=t.dtype).pin_memory()
                                                            for t in (self.tgt_labels, self.row_class, self.num_masks))
        self.two_graphs = assign == "host" or _process_group()

        def warm():
            outs = self._forward()
            self._costs(outs)
            self._assign()
            self._grads(sum(self._losses(outs).values()))

        def head():
            self.outs = self._forward()
            self._costs(self.outs)

        def tail():
            losses = self._losses(self.outs)
            total = sum(losses.values())
            self.red.pack(self._grads(total))
            if self._update_in_graph():
                self.optimizer.step(sync_hyper=False)
            self.losses = {k: v.detach() for k, v in losses.items()}
            if self.log is not None:          # behind the update: grad_norm is this iteration's
                self._record_log({**self.losses, "loss": total.detach()})
            if assign == "device":
                self.sticky.bitwise_or_(self.status)
                self.host_status.copy_(self.sticky, non_blocking=True)
            self._record_firing()
            if self.seg_log is not None:          # the step's own prediction against its own labels: two launches, one row
                self.seg_log.append(self.outs[0], self.outs[1], self.static_seg)
            if self.match_log is not None:          # what the assignment did with the costs it was given: two launches, one row
                self.match_log.append(self.match_inputs[0], self.outs[0], self.row_class)

        def whole():
            head()
            tail()
        self._graphs = self._capture(warm, warmup, [head, tail] if self.two_graphs else [whole])
        for name, graph in zip(("graph", "graph_tail") if assign == "device" else ("graph_a", "graph_b"), self._graphs):
            setattr(self, name, graph)
        self._after_capture()
        if assign == "device":
            self.sticky.zero_()                              # (whatever the warm-up on the example inputs left is not a replay's)
            torch.cuda.synchronize()
            self.host_status.zero_()

    def _costs(self, outs):
        """matching costs against every class id -> host: pinned memory, for _match; device: the assignment kernel, into the
        static tables (and the status word)"""
        with torch.no_grad():
            cost, count = self.crit.costs_all_classes(outs[0], outs[1], self.static_seg)
            if self.match_log is not None:          # held like `outs`: the log's launches read the costs at the END of the step
                cost = cost.contiguous()          # (the assignment makes this copy itself where it is one: no launch more)
                self.match_inputs = (cost, count)
            if self.assign == "device":
                self.crit.match_tables_device(cost, count, out=(self.tgt_labels, self.row_class, self.num_masks, self.status))
            else:
                self.host_cost.copy_(cost, non_blocking=True)
                self.host_count.copy_(count, non_blocking=True)

    def _assign(self):
        """what lies between the two graphs (in the one-graph form: nothing, there is no process group)"""
        if self.assign == "device":
            self._reduce_num_masks()
        else:
            torch.cuda.current_stream().synchronize()
            self._match()

    def _match(self):
        """host_cost / host_count (complete: the stream was synchronised) -> the three device tables."""
        tgt, rows, avg = self.crit.match_tables(self.host_cost.numpy(), self.host_count.numpy())
        self.host_tgt.copy_(torch.from_numpy(tgt))
        self.host_rows.copy_(torch.from_numpy(rows))
        self.host_avg.copy_(torch.from_numpy(avg))
        self.tgt_labels.copy_(self.host_tgt, non_blocking=True)
        self.row_class.copy_(self.host_rows, non_blocking=True)
        self.num_masks.copy_(self.host_avg, non_blocking=True)
        self._reduce_num_masks()

    def _reduce_num_masks(self):
        import torch.distributed as dist
        if _process_group() and dist.get_world_size() > 1:
            dist.all_reduce(self.num_masks.div_(dist.get_world_size()))          # reduce_mean (maskformer_head.py:459)

    def _losses(self, outs):
        return self.crit.loss_from_tables(outs[0], outs[1], self.static_seg, self.tgt_labels, self.row_class, self.num_masks)

    def _raise_for(self, word):
        if word:
            torch.cuda.current_stream().synchronize()      # the error path may wait: replays already queued have copied by now
            word |= int(self.host_status[0])
            self.sticky.zero_()
            torch.cuda.current_stream().synchronize()
            self.host_status.zero_()
            self.crit.raise_for_status(word)

    def check(self):
        """assign="device": wait for the last replay and raise what the host route would have raised for its inputs (a label
        >= num_classes in the map; non-finite matching costs).  The host route has raised inside `__call__` already."""
        if self.assign == "device":
            torch.cuda.current_stream().synchronize()
            self._raise_for(int(self.host_status[0]))

    def __call__(self, x=None, seg=None):
        if self.assign == "device":
            self._raise_for(int(self.host_status[0]))          # the word of an earlier replay, if it has landed; no wait
        self._begin(x)
        if seg is not None:
            self.static_seg.copy_(self.crit.seg_as_u8(seg, self.ignore_index), non_blocking=True)
        self._graphs[0].replay()
        if self.two_graphs:
            self._assign()
            self._graphs[1].replay()
        self._end()
        return self.losses


class GraphedOverlapStep(_Captured):
    """BENCHMARK-ONLY (no weight update between steps): forward(k+1) replays before all-reduce(k) has finished, so an optimiser
    could not apply the averaged gradients of step k before step k+1 reads (and re-splits) the weights -- with an optimiser in the
    loop this would be one-step-stale data parallelism, not the reference's synchronous MMDistributedDataParallel step.  The
    synchronous form is GraphedStep + FlatGradAllReduce.reduce().
    The data-parallel step with its gradient all-reduce OVERLAPPED ("launched as backward finishes"):
    the step is two hipGraphs,
        graph F : membrane reset + weight re-split + forward + loss                    (does not touch the gradient buffer)
        graph B : gradient-buffer clear + backward + packing
    and the averaging all-reduce of step k runs on a side stream while graph F of step k + 1 replays:
        F(k+1) | wait for all-reduce(k) | B(k+1) | all-reduce(k+1) async | F(k+2) ...
    At C2 the forward is ~1/3 of a 50 ms step, the collective moves 137 MB (0.2-1.6 ms over xGMI): it disappears behind the
    forward.  `finish()` joins the last collective (the gradients of the last step are then averaged in `grad_buffer.flat`)."""

    def __init__(self, model, loss_fn, example_input, grad_buffer, warmup=3, buckets=1):
        self.model, self.loss_fn, self.red, self.buckets = model, loss_fn, grad_buffer, buckets
        self.static_in = example_input.clone()

        def warm():
            loss = self._forward()
            self.red.zero()
            self._grads([loss])

        def graph_f():
            self.loss = self._forward()

        def graph_b():
            self.red.zero()
            self.red.pack(self._grads([self.loss]))
        self.graph_f, self.graph_b = self._capture(warm, warmup, [graph_f, graph_b])

    def _forward(self):
        reset_net(self.model)
        return self.loss_fn(*self.model(self.static_in))

    def __call__(self, x=None):
        self._begin(x)
        self.graph_f.replay()                 # runs under the previous step's all-reduce
        self.red.wait()                       # ... which must be done before the buffer is cleared
        self.graph_b.replay()
        self.red.reduce_async(self.buckets)
        return self.loss

    def finish(self):
        self.red.wait()


class CapturePolicy:
    """Which inference calls become hipGraphs -- host arithmetic only, the device work injected:
        eager(*args)          -> result                       a key not (yet) captured
        capture(key, *args)   -> (entry, result)              at sighting number `capture_after` of a key
        replay(entry, *args)  -> result                       every later call of that key
    At most `max_graphs` entries live at once, the least recently used one is dropped (its graph and memory pool go with the last
    reference); the sighting counts of uncaptured keys sit in a table of at most `max_sightings` keys, the oldest forgotten first, so
    a stream of pictures whose shapes never repeat costs a dictionary entry each and nothing else.  `census`: what happened."""

    def __init__(self, eager, capture, replay, max_graphs=8, capture_after=2, max_sightings=256):
        if max_graphs < 1 or capture_after < 1 or max_sightings < 1:
            raise ValueError(f"max_graphs, capture_after and max_sightings are >= 1, got {(max_graphs, capture_after, max_sightings)}")
        self.eager, self.capture, self.replay = eager, capture, replay
        self.max_graphs, self.capture_after, self.max_sightings = int(max_graphs), int(capture_after), int(max_sightings)
        self.graphs, self.sightings = collections.OrderedDict(), collections.OrderedDict()
        self.census = dict(captures=0, replays=0, evictions=0, eager={})

    def count_eager(self, reason):
        self.census["eager"][reason] = self.census["eager"].get(reason, 0) + 1

    def __call__(self, key, *args):
        entry = self.graphs.get(key)
        if entry is not None:
            self.graphs.move_to_end(key)
            self.census["replays"] += 1
            return self.replay(entry, *args)
        seen = self.sightings.pop(key, 0) + 1
        if seen < self.capture_after:
            self.sightings[key] = seen                       # (re-inserted: the most recently seen key is forgotten last)
            while len(self.sightings) > self.max_sightings:
                self.sightings.popitem(last=False)
            self.count_eager("sightings")
            return self.eager(*args)
        while len(self.graphs) >= self.max_graphs:           # before the capture: the dropped pool is free for the new one
            self.graphs.popitem(last=False)
            self.census["evictions"] += 1
        entry, result = self.capture(key, *args)
        self.graphs[key] = entry
        self.census["captures"] += 1
        return result


class _PredictGraph(_Captured):
    """one captured key of GraphedPredict: static input, graph, static output"""


class GraphedPredict:
    """The stateless inference `reset_net(model); model.encode_decode(x, metas)` (eval mode, no autograd) as hipGraph replays: one
    graph per KEY = (input shape [B, 3, H, W], the `img_shape` MaskFormerHead.predict reads from batch_img_metas[0],
    maskformer_head.PREDICT_LAST_ONLY, fused.EVAL_FUSION, ops.cfg.launch_snapshot()), by the rules of CapturePolicy.  `fn`: the
    callable that is captured instead of `model.encode_decode` (EncoderDecoder routes its own encode_decode through here and passes
    the plain one).

    `gp(inputs, batch_img_metas)` -> seg logits [B, K, H, W].  A replay's result is the graph's STATIC output: the next replay of
    that key overwrites it (`is_static(t)`: whether `t` is the buffer the last call returned).

    Stateless by contract: the captured pass resets the membranes itself and runs with keep_membrane = False on every neuron (each
    neuron's flag is put back when the capture ends); after every call of an eligible input -- eager, capturing or replaying -- the
    membranes are in their reset state.
    Weights stay live: ops.RESPLIT_IN_GRAPH is left alone, so a replay re-converts every weight from the fp32 parameters, and what
    the eval routes fold from BatchNorm's affine and running statistics is folded inside the graph (fused.live_fold): an optimizer
    step, an in-place edit or load_state_dict between replays is honoured without a new capture.  A parameter that is MOVED
    (model.to(...), a new flat buffer) needs a new GraphedPredict.

    Eligible: a contiguous fp32 CUDA input, the model in eval mode, autograd off, no capture under way, and no neuron with counters
    (FiringRecorder, FiringLog) or forward hooks.  Anything else runs `fn` unchanged, and `census["eager"]` counts the reason next
    to the captures, replays and evictions."""

    def __init__(self, model, max_graphs=8, capture_after=2, warmup=2, fn=None):
        self.model, self.warmup = model, max(int(warmup), 1)
        self.fn = fn if fn is not None else model.encode_decode
        # (through a weak reference: no cycle gp -> policy -> bound method -> gp, so a GraphedPredict that is dropped releases its
        # graphs and their pools at once, by reference count, and not whenever the cycle collector next runs -- see _capture)
        me = weakref.ref(self)
        self.policy = CapturePolicy(lambda *a: me()._eager(*a), lambda *a: me()._capture(*a), lambda *a: me()._replay(*a),
                                    max_graphs, capture_after)
        self.census = self.policy.census
        self.capture_log = []          # per capture: dict(key, seconds, reserved_bytes): what max_graphs is sized by
        self._last_static = None
        # the module tree is walked once, not per call (a replay is a few hundred microseconds of host time in all)
        self._neurons = [m for m in model.modules() if hasattr(m, "keep_membrane")]
        self._resettable = resettable(model)

    def __deepcopy__(self, memo):      # a copied model captures its own graphs (EncoderDecoder builds a new one lazily)
        return None

    def key(self, inputs, batch_img_metas):
        from . import fused, maskformer_head
        return (tuple(inputs.shape), tuple(int(v) for v in batch_img_metas[0]["img_shape"]), bool(maskformer_head.PREDICT_LAST_ONLY),
                bool(fused.EVAL_FUSION), tuple(sorted(ops.cfg.launch_snapshot().items())))

    def ineligible(self, inputs):
        """-> the reason this call cannot be a replay, or None"""
        if not (torch.is_tensor(inputs) and inputs.is_cuda):
            return "not_cuda"
        if inputs.dtype != torch.float32 or inputs.dim() != 4 or not inputs.is_contiguous():
            return "not_contiguous_fp32"
        if self.model.training:
            return "training_mode"
        if torch.is_grad_enabled():
            return "grad_enabled"
        if torch.cuda.is_current_stream_capturing():
            return "capturing"
        if ops.census_active():          # (an OpCensus measures the operands of eager launches)
            return "op_census"
        for m in self._neurons:
            if getattr(m, "stats", None) is not None:
                return "firing_stats"
            if m._forward_hooks:
                return "forward_hooks"
        return None

    def is_static(self, t):
        return t is not None and t is self._last_static

    def __call__(self, inputs, batch_img_metas):
        self._last_static = None
        reason = self.ineligible(inputs)
        if reason is not None:
            self.policy.count_eager(reason)
            return self.fn(inputs, batch_img_metas)
        return self.policy(self.key(inputs, batch_img_metas), inputs, batch_img_metas)

    def _eager(self, inputs, batch_img_metas):
        reset_net(self.model)
        out = self.fn(inputs, batch_img_metas)
        reset_state(self.model, self._resettable)
        return out

    def _capture(self, key, inputs, batch_img_metas):
        g = _PredictGraph()
        neurons = self._neurons
        flags = [m.keep_membrane for m in neurons]

        def run():
            reset_net(self.model)
            return self.fn(g.static_in, batch_img_metas)

        def warm():
            g.result = run()

        def record():
            g.out = run()
        # Nothing that owns a hipGraph may be released WHILE this capture records: destroying a graph or returning its pool inside a
        # global-mode capture aborts the process, and the cycle collector runs whenever an allocation count says so (torch.cuda.graph
        # no longer collects on entry).  Dead cycles -- a dropped model with its GraphedPredict -- are collected here, before.
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()          # (torch.cuda.graph does so on entry anyway: the growth below is then the graph's own)
        t0, reserved = time.perf_counter(), torch.cuda.memory_reserved()
        g.static_in = inputs.clone()
        for m in neurons:
            m.keep_membrane = False
        try:
            g.graph, = g._capture(warm, self.warmup, [record])
        finally:
            for m, keep in zip(neurons, flags):
                m.keep_membrane = keep
            reset_state(self.model, self._resettable)          # no module keeps a tensor of the graph's pool (a pre-fired spike map)
        self.capture_log.append(dict(key=key[:2], seconds=time.perf_counter() - t0,
                                     reserved_bytes=torch.cuda.memory_reserved() - reserved))
        result, g.result = g.result, None          # the last warm-up pass computed this call's answer: a tensor of its own
        result.record_stream(torch.cuda.current_stream())          # (allocated on the warm-up's side stream, read on this one)
        return g, result

    def _replay(self, g, inputs, batch_img_metas):
        g._begin(inputs)
        g.graph.replay()
        for meta in batch_img_metas:          # what MaskFormerHead.predict leaves in the caller's metas
            meta["batch_input_shape"] = meta["img_shape"]
        reset_state(self.model, self._resettable)
        self._last_static = g.out
        return g.out
