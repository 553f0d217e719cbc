#!/usr/bin/env python3
"""bench.py -- forward+backward images/sec of the Spike2Former hot path on N MI355X (one process per GPU).

A "step" is one pass of the hot path over one synthetic batch: reset every membrane (what
ResetModelHook does before each iteration) -> forward (Meta-SpikeFormer backbone + MaskFormer head) -> scalar loss
`cls.mean() + masks.mean()` -> backward -> (N > 1) one RCCL all-reduce of the flat gradient buffer.  Optimiser excluded.
Inputs are resident in HBM before the timed region.  Prints ONE JSON line on rank 0.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload C2]      (N > 1 without a launcher: starts its own N ranks)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the line.  --full adds what takes runs of its own: the per-launch
HIP-event pass behind the roofline lines and the CPU baseline of the oracle.  --dump-outputs DIR writes what the last timed step
computed (loss, class scores, mask predictions, parameter gradients; predict: the seg logits) as DIR/<name>.npy in float32.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DTYPE = "f32 (fp32-equivalent: bf16 hi+mid+lo split operands on bf16 MFMA, fp32 accumulate; spike maps stored as bf16, exact)"
HBM_PEAK_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_BF16_PEAK_TFLOPS = 2500.0  # same guide: dense bf16 MFMA peak (no sparsity)
DUMP_BUDGET_ELEMS = 15_000_000   # --dump-outputs: at most 60 MB of float32 in all


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch override (informational: the metric's config is B = 2)")
    ap.add_argument("--gt", default="regions", choices=["regions", "noise"],
                    help="--loss hungarian: synthetic semantic maps; regions = --gt-classes classes per image as rectangles "
                         "(ADE20K averages 10.5 classes per image), noise = an independent class per pixel (all 150 present)")
    ap.add_argument("--gt-classes", type=int, default=10)
    ap.add_argument("--hungarian-graphs", default="tables", choices=["tables", "split"],
                    help="tables: graph.GraphedHungarianStep (loss inside the second graph); split: graph.GraphedSplitStep (eager loss)")
    ap.add_argument("--loss", default="headline", choices=["headline", "hungarian"],
                    help="hungarian: the reference's real training loss (SURVEY 8 row f1) on a synthetic semantic map; the "
                         "matching runs on the host in the middle of the step, so the step is launched eagerly (secondary figure)")
    ap.add_argument("--mode", default="train", choices=["train", "predict"],
                    help="predict: SECONDARY figure (SURVEY section 8 row f4) -- the inference path in eval mode under no_grad "
                         "(reset -> backbone -> head -> whole-image seg logits), hipGraph replay; --no-eval-fusion runs it on the "
                         "two-kernel conv -> BatchNorm+neuron path for comparison")
    ap.add_argument("--no-eval-fusion", action="store_true")
    ap.add_argument("--predict-all-layers", action="store_true",
                    help="predict: evaluate the SDME block and the mask contraction for all L + 1 decoder layers as `forward` does "
                         "(default: only the last layer's predictions, the ones the segmentation logits are formed from)")
    ap.add_argument("--optimizer", action="store_true",
                    help="SECONDARY figure (SURVEY section 8 row f2): one full training ITERATION per step -- the step above + (N > 1: "
                         "all-reduce) + clip_grad_norm_(0.01) + AdamW with the config's per-parameter multipliers, as three HIP "
                         "launches over the flat gradient buffer (train.FlatAdamW), captured behind the step when N = 1.  The "
                         "headline metric excludes the optimiser (BASELINE.md section 3); this line includes it")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the per-launch HIP-event pass (roofline lines, --dump-events) and the "
                         "CPU baseline (cpu_baseline, gpu_over_cpu); a plain run measures the headline figure only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step computed as DIR/<name>.npy (float32; an array over its share of the "
                         "60 MB budget is written as <name>_sample.npy, a fixed seeded sample of its elements)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-kernel-events", action="store_true", help="--full: skip the per-launch HIP-event pass on the LIF kernels")
    ap.add_argument("--dump-events", default=None, help="--full: write (kernel, algorithmic bytes, us) of every timed launch here")
    ap.add_argument("--wgrad-stream", action="store_true",
                    help="launch the sunk weight-gradient kernels on a side stream (measured: 69.4 vs 67.2 ms/step -- slower)")
    ap.add_argument("--branch-streams", type=int, default=0,
                    help="run sibling chains (q / k / v projections, DCN input vs offset/mask) on this many side streams; "
                         "measured 54.4 - 56.6 vs 56.7 - 57.0 ms/step: the gain depends on how the HIP runtime maps the graph's "
                         "branches onto its queues, which varies from process to process -- off by default")
    ap.add_argument("--long-streams", type=int, default=0,
                    help="1: lateral convs / H/2 FPN level + mask_feature / decoder key-value projections on side streams "
                         "(S2F_LONG_WHAT=lat,mf,kv selects; measured: mf -0.8 ms, kv +0.7 ms, lat 0 -- off by default)")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel from Python instead of replaying a hipGraph")
    ap.add_argument("--overlap-allreduce", action="store_true",
                    help="N > 1: forward / backward as two graphs with the all-reduce of step k overlapped with the forward of "
                         "step k + 1 (graph.GraphedOverlapStep) instead of ONE graph + a blocking all-reduce behind it.  "
                         "Measured in the one-rank RCCL rehearsal: 52.1 vs 49.8 ms/step -- the second graph launch and the "
                         "two stream hand-overs cost ~2.3 ms, more than the 0.2-1.6 ms collective they hide: off by default")
    ap.add_argument("--rendezvous-only", action="store_true",
                    help="N > 1 plumbing check (runs on CPU with S2F_DIST_BACKEND=gloo): launch the ranks, rendezvous, one "
                         "all-reduce, print {\"rendezvous\": \"ok\", \"ranks_seen\": N} on rank 0 and exit -- no model, no GPU")
    ap.add_argument("--allow-eager", action="store_true",
                    help="N > 1: fall back to eager launches when the hipGraph capture fails (host-bound, ~2x slower: a curve "
                         "that mixes graph and eager points is meaningless, so the default is to fail)")
    args = ap.parse_args()
    if not args.full:
        args.no_cpu_baseline = args.no_kernel_events = True
    return args


def dump_outputs(dirname, arrays):
    """--dump-outputs: each tensor as DIR/<name>.npy in float32.  The budget is shared equally; a tensor larger than its share
    is written flattened as <name>_sample.npy: its elements at sorted indices drawn by numpy's default_rng(0), so the same
    arguments select the same elements in every run."""
    import numpy as np
    import torch
    os.makedirs(dirname, exist_ok=True)
    share = DUMP_BUDGET_ELEMS // len(arrays)
    for name, t in arrays.items():
        t = t.detach()
        if t.numel() > share:
            idx = np.sort(np.random.default_rng(0).integers(0, t.numel(), size=share))
            t, name = t.reshape(-1)[torch.from_numpy(idx).to(t.device)], name + "_sample"
        np.save(os.path.join(dirname, name + ".npy"), t.float().cpu().numpy())


def cpu_baseline(workload, timed_steps=3):
    """The oracle (a port of the reference's PyTorch CPU path, pinned against it on golden vectors) timed on this box's
    host cores: fwd+bwd steps at the workload's shapes with B=1 -- a bounded sample of the same workload -- 1 warm-up + 3
    timed steps."""
    import torch

    from oracle import s2f_oracle as so        # cpu_baseline leg only
    import dataclasses
    cfg = dataclasses.replace(so.CONFIGS[workload], B=1)
    logical = os.cpu_count() or 1
    cores = logical // 2 if logical >= 16 else logical        # physical cores (SMT siblings do not help fp32 GEMM/conv)
    torch.set_num_threads(cores)
    st = so.make_params(cfg)
    net = so.OracleNet(st, cfg, training=True)
    img = so.synthetic_image(cfg)
    times = []
    for _ in range(1 + timed_steps):
        for p in st.values():
            p.grad = None
        t0 = time.perf_counter()
        net.reset()
        cls, masks = net.forward(img)
        so.headline_loss(cls, masks).backward()
        times.append(time.perf_counter() - t0)
    dt = sum(times[1:]) / timed_steps
    return {"value": round(cfg.B / dt, 5), "unit": "images/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"1 warm-up + {timed_steps} timed fwd+bwd steps, B=1, {cfg.H}x{cfg.W}, T={cfg.T}, fp32, "
                      f"oracle/s2f_oracle.py (torch {torch.__version__} CPU kernels); step times "
                      + ", ".join(f"{t:.1f}" for t in times) + " s (first = warm-up)"}


def predict_bench(args, s2f, ops, dev, w, B, rank, world):
    """Secondary line: inference images/s (eval mode, running-statistics BatchNorm, no autograd), one hipGraph per step."""
    import torch
    from spike2former_amd import fused
    from spike2former_amd.init_utils import seeded_init
    fused.EVAL_FUSION = not args.no_eval_fusion
    from spike2former_amd import maskformer_head
    maskformer_head.PREDICT_LAST_ONLY = not args.predict_all_layers
    # inference: the weights are frozen, so the graph does not re-convert them (bf16 packs) on every replay as a training step must
    # (0.23 ms per replay at C2); they are converted once below, before the capture
    resplit_was, ops.RESPLIT_IN_GRAPH = ops.RESPLIT_IN_GRAPH, False
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg(args.workload))).to(dev).eval()
    s2f.set_keep_membrane(model, False)
    img = torch.randn(B, 3, w["H"], w["W"], generator=torch.Generator().manual_seed(1000 + rank)).to(dev)

    def fwd():
        s2f.reset_net(model)
        with torch.no_grad():
            return model(img, mode="logits")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(max(args.warmup, 2)):
            fwd()
    torch.cuda.current_stream().wait_stream(side)
    ops.resplit_all(dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fwd()
    keep = ops.conversion_state()          # noqa: F841  (addresses baked into the graph)
    for _ in range(args.warmup):
        graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        graph.replay()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"logits": out})
    if rank == 0:
        print(json.dumps({
            "metric": f"predict images/sec ({args.workload}: eval mode, whole-image inference to seg logits) [secondary]",
            "value": round(B * world * args.steps / dt, 3), "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": DTYPE, "data": "synthetic", "launch": "hipGraph replay",
            "eval_fusion": bool(fused.EVAL_FUSION), "logits_shape": list(out.shape),
            "sdme_layers_evaluated": ("last (the one the logits are formed from)" if maskformer_head.PREDICT_LAST_ONLY else "all L + 1"),
            "config": {"workload": f"{args.workload}: {w['H']}x{w['W']} T={w['T']} K={w['K']}, per-GPU batch {B}",
                       "global_batch": B * world, "parallelism": f"dp{world}", "weights": "random-init (name-seeded)"}}), flush=True)
    ops.RESPLIT_IN_GRAPH = resplit_was          # (process-global: a training graph captured later must re-convert its weights)


def self_launch(args):
    """`python bench.py --gpus N` typed without a launcher (no WORLD_SIZE in the environment): start the N ranks ourselves, the
    way the reference's tools/dist_train.sh:5-12 does -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node N
    --master-addr 127.0.0.1 --master-port P bench.py <same arguments>` as a CHILD process, before this process has imported
    torch or touched a GPU (nothing is re-exec'ed) -- relay its output (rank 0 prints the JSON line) and exit with its code."""
    import socket
    import subprocess
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    rc = 1
    for attempt in range(3):
        # a free port found by bind / close can be taken by somebody else before the launcher binds it again: the rendezvous then
        # fails within seconds (nothing has been measured yet) and the launch is repeated on another port
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        p = subprocess.run(cmd, env=env, stderr=subprocess.PIPE, text=True)
        sys.stderr.write(p.stderr)
        rc = p.returncode
        if rc == 0 or "EADDRINUSE" not in p.stderr and "Address already in use" not in p.stderr:
            break
    return rc


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    import torch
    import torch.distributed as dist

    import spike2former_amd as s2f
    from spike2former_amd import ops
    from spike2former_amd.dist import FlatGradAllReduce, broadcast_params, init_process_group
    from spike2former_amd.init_utils import seeded_init

    # a shape that leaves the package's kernels for a vendor library / ATen path is an error here, not a slower number
    ops.STRICT = os.environ.get("S2F_STRICT", "1") != "0"
    rank, world, local = init_process_group()
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}: the launcher's --nproc-per-node must equal --gpus"
    if args.rendezvous_only:
        seen = torch.ones(1)
        if world > 1:
            if dist.get_backend() == "nccl":
                seen = seen.cuda(local)
            dist.all_reduce(seen)
            dist.barrier()
        if rank == 0:
            print(json.dumps({"rendezvous": "ok", "ranks_seen": int(seen.item()), "n_gpus": args.gpus,
                              "backend": dist.get_backend() if world > 1 else None}), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return
    assert torch.cuda.is_available(), "bench.py measures the HIP path; no GPU visible"
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)

    w = s2f.WORKLOADS[args.workload]
    B = args.batch or w["B"]                        # per-GPU batch: weak scaling (BASELINE.json configs[1]: batch=2 on 1 GPU)
    if args.mode == "predict":
        return predict_bench(args, s2f, ops, dev, w, B, rank, world)
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg(args.workload))).to(dev).train()
    broadcast_params(model)
    s2f.set_keep_membrane(model, False)             # a reset precedes every step -> the membrane is never read back
    red = FlatGradAllReduce(model.parameters(), world)
    red.install_sinks()                             # weight-gradient kernels add straight into the flat buffer
    if args.wgrad_stream:
        ops.WGRAD_STREAM = torch.cuda.Stream(device=dev)   # ... from a side stream, off the data-gradient chain
    if args.branch_streams > 0:
        ops.BRANCH_STREAMS = [torch.cuda.Stream(device=dev) for _ in range(args.branch_streams)]
    if args.long_streams:
        ops.LONG_STREAMS = [torch.cuda.Stream(device=dev) for _ in range(2)]
        if os.environ.get("S2F_LONG_WHAT"):
            ops.LONG_WHAT = tuple(os.environ["S2F_LONG_WHAT"].split(","))
    img = torch.randn(B, 3, w["H"], w["W"], generator=torch.Generator().manual_seed(1000 + rank)).to(dev)

    seg = None
    graphed_model = None
    want_split_graphs = False
    hungarian = None
    held = {}               # the headline step's outputs, for --dump-outputs: a captured step's are its graph's static tensors

    def headline_loss(cls, masks):
        # detached: a reference to the outputs themselves would keep the step's autograd graph alive into the next step
        held["cls"], held["masks"] = cls.detach(), masks.detach()
        return s2f.headline_loss(cls, masks)

    if args.loss == "hungarian":
        args.no_cpu_baseline = args.no_kernel_events = True
        gen = torch.Generator().manual_seed(1 + rank)
        if args.gt == "noise":          # every pixel an independent class: all K classes present, every query matched (worst case)
            seg = torch.randint(0, w["K"], (B, 1, w["H"], w["W"]), generator=gen)
        else:                           # ADE20K-like: ~10.5 classes per image (Zhou et al. 2017) as axis-aligned regions
            seg = torch.empty(B, 1, w["H"], w["W"], dtype=torch.int64)
            for i in range(B):
                classes = torch.randperm(w["K"], generator=gen)[:args.gt_classes]
                ys = torch.sort(torch.randint(1, w["H"], (3,), generator=gen)).values.tolist()
                plane = torch.empty(w["H"], w["W"], dtype=torch.int64)
                k = 0
                for y0, y1 in zip([0] + ys, ys + [w["H"]]):
                    cuts = max(args.gt_classes // 4, 1)
                    xs = torch.sort(torch.randint(1, w["W"], (cuts,), generator=gen)).values.tolist()
                    for x0, x1 in zip([0] + xs, xs + [w["W"]]):
                        plane[y0:y1, x0:x1] = classes[k % args.gt_classes]
                        k += 1
                seg[i, 0] = plane
        seg = seg.to(dev)
        want_split_graphs = not args.no_graph
        args.no_graph = True

    def eager_step():
        if hungarian is not None:
            hungarian()                                  # graph A (forward + costs) | host assignment | graph B (loss + backward)
            red.reduce()
            red.wait()
            return
        if seg is not None and graphed_model is not None:
            leaves = graphed_model.forward()            # graph A: reset + gradient clear + forward
            gts = [s2f.seg_to_instances(seg[i]) for i in range(B)]
            sum(model.decode_head.loss_by_feat(leaves[0], leaves[1], gts).values()).backward()
            graphed_model.backward(leaves)              # graph B: backward + gradient packing
            red.reduce()
            red.wait()
            return
        s2f.reset_net(model)
        red.zero()
        if seg is not None:
            sum(model(img, [seg[i] for i in range(B)], mode="loss").values()).backward()
        else:
            loss = headline_loss(*model(img))
            loss.backward()
            held["loss"] = loss.detach()
        ops.wgrad_join()
        red.gather()
        red.reduce()
        red.wait()

    eager_step()                                    # discovers which gradients arrive through a sink ...
    red.compact()                                   # ... and moves them behind the others: packing stays one batched copy
    optim = sched = None
    if args.optimizer and args.overlap_allreduce:
        # GraphedOverlapStep replays forward(k + 1) under all-reduce(k): no update can sit in between (one-step-stale data
        # parallelism otherwise), and a line labelled "training iteration" must have run the optimiser
        raise SystemExit("bench.py: --optimizer and --overlap-allreduce exclude each other (the overlapped step is benchmark-only)")
    if args.optimizer:
        # configs/Spike2Former/SDTv2_maskformer_DCNpixelDecoder_ade20k.py:137-167
        from spike2former_amd.train import FlatAdamW, LinearThenPoly
        args.no_cpu_baseline = args.no_kernel_events = True
        optim = FlatAdamW(model, red, lr=0.001, betas=(0.9, 0.999), weight_decay=0.005, clip_grad=dict(max_norm=0.01, norm_type=2),
                          paramwise_cfg=dict(custom_keys={"backbone": dict(lr_mult=0.1, decay_mult=1.0),
                                                          "query_embed": dict(lr_mult=1.0, decay_mult=0.0),
                                                          "query_feat": dict(lr_mult=1.0, decay_mult=0.0),
                                                          "level_embed": dict(lr_mult=1.0, decay_mult=0.0)}))
        sched = LinearThenPoly(optim, warmup=1500, total=160000, start_factor=1e-6, eta_min=0.0, power=1.0)
    if seg is not None and want_split_graphs and args.hungarian_graphs == "tables":
        # The assignment runs on the host, so the step cannot be ONE graph: forward + matching costs are one graph, the losses (from
        # the assignment's tables) + backward another (graph.GraphedHungarianStep).
        from spike2former_amd.graph import GraphedHungarianStep
        hungarian = GraphedHungarianStep(model, img, seg, red, warmup=max(args.warmup, 2), optimizer=optim if world == 1 else None)
    elif seg is not None and want_split_graphs:
        # forward and backward as two graphs around the EAGER loss (graph.GraphedSplitStep; generic instance masks)
        from spike2former_amd.graph import GraphedSplitStep
        graphed_model = GraphedSplitStep(model, img, red, warmup=max(args.warmup, 2))
    graphed = overlapped = None
    distributed = dist.is_available() and dist.is_initialized()
    if not args.no_graph and distributed and args.overlap_allreduce:
        # N > 1: forward and backward as two graphs, the all-reduce of step k under the forward of step k + 1
        from spike2former_amd.graph import GraphedOverlapStep
        try:
            overlapped = GraphedOverlapStep(model, s2f.headline_loss, img, red, warmup=max(args.warmup, 2))
        except RuntimeError as e:
            print(f"[bench rank {rank}] forward / backward graph capture failed ({e}); single graph + blocking all-reduce",
                  file=sys.stderr, flush=True)
            overlapped = None
            torch.cuda.synchronize()
    if not args.no_graph and overlapped is None:
        # reset + grad clear + forward + loss + backward captured once as a hipGraph; the RCCL all-reduce stays eager
        from spike2former_amd.graph import GraphedStep
        try:
            graphed = GraphedStep(model, headline_loss, img, grad_buffer=red, warmup=max(args.warmup, 2),
                                  optimizer=optim if world == 1 else None)
        except RuntimeError as e:                   # N > 1 with --allow-eager only: eager launches, labelled as such
            if world == 1 or not args.allow_eager:
                raise
            print(f"[bench rank {rank}] hipGraph capture failed ({e}); timing eager launches", file=sys.stderr, flush=True)
            graphed = None
            torch.cuda.synchronize()

    def step():
        if overlapped is not None:
            return overlapped()
        if graphed is None:
            eager_step()
        else:
            graphed()
            red.reduce()
            red.wait()
        if optim is not None:
            if world > 1 or (graphed is None and hungarian is None):
                optim.step()                          # N > 1: behind the all-reduce (eager: three launches); eager steps likewise
            sched.step()

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    if overlapped is not None:
        overlapped.finish()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    if overlapped is not None:
        overlapped.finish()               # the last step's all-reduce belongs to the timed region
    fence()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        # what a caller of the step receives: the loss and the model's outputs (headline loss only) and every parameter's
        # gradient, averaged over the ranks, in model.parameters() order (the flat buffer's own order depends on compact())
        got = dict(held)
        if graphed is not None:
            got["loss"] = graphed.static_loss
        elif overlapped is not None:            # captured with s2f.headline_loss: its outputs are not kept
            got = {"loss": overlapped.loss}
        slot = dict(zip(map(id, red.params), red.views))
        got["grads"] = torch.cat([slot[id(p)].reshape(-1) for p in model.parameters() if id(p) in slot])
        dump_outputs(args.dump_outputs, got)
    # Per-launch durations of the neuron kernels: HIP events cannot be read back from inside a replayed hipGraph, so the
    # same kernels on the same tensors are timed in eager steps right after the timed region (events on the launch stream).
    events = None
    if not args.no_kernel_events:
        side, ops.WGRAD_STREAM = ops.WGRAD_STREAM, None     # per-kernel durations are taken with the GPU to themselves
        eager_step(); torch.cuda.synchronize()
        ops.KERNEL_EVENTS = []
        for _ in range(2):
            eager_step()
        events = ops.drain_kernel_events()          # [(kernel, algorithmic bytes, MFMA flops, us)]
        ops.WGRAD_STREAM = side
    tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax)

    out = None
    if rank == 0:
        ms = dt / args.steps * 1e3
        out = {
            "metric": (("training iteration (fwd+bwd+clip+AdamW) images/sec [secondary], " if optim is not None else "") +
                       ("fwd+bwd images/sec, 512x512 T=4 ADE20K-150" if args.workload == "C2" else f"fwd+bwd images/sec ({args.workload})"))
                      + ((f" [Hungarian-matched loss, synthetic semantic maps: {'per-pixel noise, all classes present' if args.gt == 'noise' else str(args.gt_classes) + ' classes per image'}; "
                         + ("forward+costs / losses+backward hipGraphs around the host-side assignment]" if hungarian is not None
                            else "forward / backward hipGraphs around the eager loss]" if graphed_model is not None else "eager]"))
                         if seg is not None else ""),
            "value": round(B * world * args.steps / dt, 3), "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": DTYPE, "data": "synthetic", "launch": ("forward / backward hipGraphs, all-reduce of step k under the forward of step k+1 (benchmark-only: no weight update fits in between)" if overlapped is not None
                                             else "forward+costs / losses+backward hipGraphs around the host-side assignment" if hungarian is not None
                                             else "forward / backward hipGraphs around the eager loss" if graphed_model is not None
                                             else "eager" if graphed is None else "hipGraph replay"),
            "ranks_seen": (dist.get_world_size() if distributed else 1),
            "config": {"workload": f"{args.workload}: {w['H']}x{w['W']} T={w['T']} K={w['K']} "
                                   f"{'E-SpikeFormer (SDT-v3)' if 'v2' in str(w.get('backbone', '')) else 'Meta-SpikeFormer'} "
                                   f"{w['embed_dim']} + MaskFormer head, per-GPU batch {B}",
                       "global_batch": B * world, "parallelism": f"dp{world}", "weights": "random-init (name-seeded)"},
        }
        out["peak_hbm_GB"] = round(torch.cuda.max_memory_allocated(dev) / 1e9, 2)     # of 288 GB (allocator high-water mark)
        if events:
            # HBM bytes per launch from the PMC passes committed under profiles/ (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in
            # separate runs, gfx950 corrections applied there); null when no such profile exists for a kernel
            traffic, traffic_src = {}, None
            try:
                # the newest committed profile, and only if it was taken on THESE streaming kernels: the profile records a hash of
                # csrc/bn_lif.hip + lif.hip (tools/pmc_traffic.py); after a change to them it is stale and `traffic` is null
                import hashlib
                h = hashlib.sha256()
                for f_ in ("bn_lif.hip", "lif.hip"):
                    h.update(open(os.path.join(ROOT, "spike2former_amd", "csrc", f_), "rb").read())
                sha = h.hexdigest()[:16]
                import glob
                cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")))          # the newest round's profile
                path = cands[-1] if cands else os.path.join(ROOT, "profiles", "pmc_traffic.json")
                pname = "profiles/" + os.path.basename(path)
                if os.path.exists(path):
                    with open(path) as f:
                        prof = json.load(f)
                    if prof.get("streaming_kernel_sources_sha16") == sha:
                        traffic = {k: v["hbm_bytes_per_launch"] for k, v in prof["kernels"].items()}
                        traffic_src = (pname + " (rocprofv3 --pmc passes of an earlier run of this command on the "
                                       "same kernel sources, not measured in this run)")
                    else:
                        traffic_src = pname + " is STALE (the streaming kernels changed since): traffic not reported"
            except (OSError, KeyError, ValueError):
                pass
            if args.dump_events:
                with open(args.dump_events, "w") as f:
                    for name, nbytes, flops, us, moved in events:
                        f.write(f"{name} {nbytes} {flops} {us:.2f} {moved}\n")
            agg = {}
            for name, nbytes, flops, us, moved in events:
                a = agg.setdefault(name, [0, 0.0, 0, 0, 0])
                a[0] += nbytes; a[1] += us * 1e-6; a[2] += 1; a[3] += flops; a[4] += moved
            for name, key in (("bn_lif_fwd", "roofline"), ("bn_lif_bwd", "roofline_bn_lif_bwd"), ("lif_fwd", "roofline_lif_fwd"),
                              ("lif_bwd", "roofline_lif_bwd"), ("bn_fwd", "roofline_bn_fwd"), ("bn_bwd", "roofline_bn_bwd"),
                              ("bn_stats", "roofline_bn_stats")):
                if name in agg:
                    nbytes, secs, launches, _, moved = agg[name]
                    gbs = nbytes / secs / 1e9
                    # `achieved` prices the launch at SURVEY 8d's ALGORITHMIC bytes (the reference's fp32 tensors: 4 B per
                    # element read or written); `moved_*` is what this build's kernel actually transfers for them (spike
                    # maps leave as bf16: 2 B per element) -- both are reported, as 8d asks
                    # `achieved` / `frac`: the bytes this build's kernel actually MOVES (spike maps leave as bf16: 2 B per
                    # element) over the launch time -- the bandwidth really used, which is what the 8 TB/s roof bounds.
                    # `algorithmic_*`: the same launches priced at SURVEY 8d's figures for the reference's fp32 tensors (4 B
                    # per element read or written) -- reported next to it, as 8d asks.
                    mgbs = moved / secs / 1e9
                    out[key] = {"kernel": name, "bound": "hbm", "achieved": round(mgbs, 1), "peak": HBM_PEAK_GBS,
                                "unit": "GB/s", "frac": round(mgbs / HBM_PEAK_GBS, 4),
                                "traffic": traffic.get(name) if args.workload == "C2" else None,
                                "traffic_source": (traffic_src if args.workload == "C2" else None),
                                "launches": launches, "avg_launch_us": round(secs / launches * 1e6, 2),
                                "moved_bytes_per_launch": moved // launches,
                                "algorithmic_bytes_per_launch": nbytes // launches,
                                "algorithmic_GBps": round(gbs, 1), "algorithmic_frac": round(gbs / HBM_PEAK_GBS, 4)}
            # the same fused forward kernel restricted to launches whose operands cannot sit in the caches (>= 128 MB of
            # algorithmic traffic): what the kernel itself sustains, next to the all-launches figure above that is dominated
            # by the 5 us launch floor of the 2-33 MB launches ("streaming-kernel efficiency")
            big = [(nb, us, mv) for name, nb, _, us, mv in events if name == "bn_lif_fwd" and nb >= 128e6]
            if big:
                tsec = sum(us for _, us, _ in big)
                gbs, mgbs = sum(nb for nb, _, _ in big) / tsec / 1e3, sum(mv for _, _, mv in big) / tsec / 1e3
                out["roofline_bn_lif_fwd_hbm_resident"] = {
                    "kernel": "bn_lif_fwd", "bound": "hbm", "achieved": round(mgbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(mgbs / HBM_PEAK_GBS, 4), "traffic": None, "launches": len(big),
                    "avg_launch_us": round(tsec / len(big), 2), "min_algorithmic_bytes": 128000000,
                    "algorithmic_GBps": round(gbs, 1), "algorithmic_frac": round(gbs / HBM_PEAK_GBS, 4)}
            # the MFMA kernels: ALGORITHMIC flops (2 M N K per GEMM) against the dense bf16 MFMA peak.  Every fp32
            # multiply-add is issued as 3 bf16 products (W or dY split hi + mid + lo, fp32-equivalent accuracy):
            # `issued_frac` = 3 x frac is the matrix pipes' own utilisation.  The K <= 256 shapes of the path are bound by
            # streaming X / Y (moved_GBps), see DESIGN.md section 4.
            for name, key in (("spike_gemm_fwd", "roofline_spike_gemm_fwd"), ("spike_gemm_dw", "roofline_spike_gemm_dw"),
                              ("dx_gemm", "roofline_dx_gemm")):
                if name in agg:
                    nbytes, secs, launches, flops, moved = agg[name]
                    out[key] = {"kernel": name, "bound": "mfma", "achieved": round(flops / secs / 1e12, 1),
                                "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                                "frac": round(flops / secs / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": None,
                                "issued_frac": round((6 if name == "dx_gemm" else 3) * flops / secs / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4),
                                "launches": launches, "avg_launch_us": round(secs / launches * 1e6, 2),
                                "hbm_GBps_algorithmic": round(nbytes / secs / 1e9, 1),
                                "moved_GBps": round(moved / secs / 1e9, 1)}
            out["timed_kernels_ms_per_step"] = round(sum(a[1] for a in agg.values()) / 2 * 1e3, 3)
        if world == 1 and not args.no_cpu_baseline:
            del model, red
            torch.cuda.empty_cache()
            out["cpu_baseline"] = cpu_baseline(args.workload)
            out["gpu_over_cpu"] = round(out["value"] / out["cpu_baseline"]["value"], 1)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
