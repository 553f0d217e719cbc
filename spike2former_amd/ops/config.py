"""The process-global switches of the op layer in ONE object (`ops.cfg`; `ops.X` reads and writes forward to it for the names
below): the runtime objects a step installs (sinks, side streams, the event list), the settings that select semantics or a debugging
aid, and the few A/B switches a test, bench.py or smoke() still sets.  A finished comparison leaves no switch behind: its winner is
the code, its figures are in docs/EXPERIMENTS.md.  A captured step bakes the launch structure these select into its hipGraph:
graph.py snapshots the scalar ones at capture (`cfg.snapshot()`) and refuses to replay under a different setting.  Assigning a name
that is not in FIELDS raises (a stale probe must not measure A against A)."""
import os


class Config:
    FIELDS = ("KERNEL_EVENTS", "GRAD_SINKS", "WGRAD_STREAM", "BRANCH_STREAMS", "LONG_STREAMS", "LONG_WHAT", "SPIKES_BF16",
              "SPIKE_GEMM_TERMS", "SPIKE_GEMM_ENABLED", "SPIKE_GEMM_CHECK", "CONV3X3_IMPLICIT", "CONV3X3_IMPLICIT_MIN_PIXELS",
              "CONV3X3_DX_IMPLICIT", "DEFER_DW", "DW_PIPE", "BN_PARTIALS", "BN_PARTIALS_SINGLE", "DENSE_GROUPED", "RESPLIT_IN_GRAPH",
              "FANOUT_PORTS", "GLUE_MODE", "STRICT_GLUE", "STRICT", "GENERAL_RESIZE")
    RUNTIME = ("KERNEL_EVENTS", "GRAD_SINKS", "WGRAD_STREAM", "BRANCH_STREAMS", "LONG_STREAMS")          # objects, not settings
    # A/B switches of changes whose comparison is still on record as open or fresh: part of what a captured graph depends on
    # (launch_snapshot) next to the settled list above, which tests/test_host_logic.py pins name by name
    LAUNCH_FIELDS = ("DECODER_SIBLINGS", "DCN_CHANNEL_MAJOR")

    def __setattr__(self, name, value):
        if name not in self.FIELDS and name not in self.LAUNCH_FIELDS:
            raise AttributeError(f"ops.cfg has no switch {name!r} (the switches are ops.cfg.FIELDS)")
        object.__setattr__(self, name, value)

    def __init__(self):
        self.KERNEL_EVENTS = None
        self.GRAD_SINKS = None
        self.WGRAD_STREAM = None
        self.DEFER_DW = True
        self.BRANCH_STREAMS = None
        self.LONG_STREAMS = None
        self.LONG_WHAT = ("lat", "mf", "kv")
        self.SPIKES_BF16 = True
        self.SPIKE_GEMM_TERMS = 3
        self.SPIKE_GEMM_ENABLED = True
        self.CONV3X3_IMPLICIT = True
        self.CONV3X3_IMPLICIT_MIN_PIXELS = int(os.environ.get("S2F_CONV3_MIN_PIXELS", 32 * 32))
        self.CONV3X3_DX_IMPLICIT = True
        # deferred / grouped weight gradients on the LDS-DMA pipeline (csrc/dwp.hip) where the shape qualifies (L % 4 == 0, L >= 32)
        self.DW_PIPE = os.environ.get("S2F_DW_PIPE", "1") != "0"
        self.SPIKE_GEMM_CHECK = False
        self.BN_PARTIALS = os.environ.get("S2F_BN_PARTIALS", "1") != "0"
        self.BN_PARTIALS_SINGLE = os.environ.get("S2F_BN_PARTIALS_SINGLE", "0") != "0"
        self.DENSE_GROUPED = os.environ.get("S2F_DENSE_GROUPED", "1") != "0"          # the groups of a grouped 1x1 as one launch
        # a captured step re-converts every weight (bf16 splits / packs) from the live fp32 values inside the graph, so that a replay after
        # an optimiser step multiplies by the current weights.  False: frozen weights (an inference graph) -- the conversions of capture
        # time are replayed against; a weight update then needs a new capture
        self.RESPLIT_IN_GRAPH = True
        # FANOUT_PORTS: a neuron hands out a second autograd handle for a second consumer of its spike map and a pass-through of its input
        # for a residual branch; its backward kernel sums the gradients that arrive on them (otherwise the autograd engine launches an
        # add per fan-out: 75 per C2 step, 209 M elements)
        self.FANOUT_PORTS = os.environ.get("S2F_FANOUT_PORTS", "1") != "0"
        # GLUE_MODE: the captured steps (graph.py) run their warm-up and capture under ops.GlueMode -- the residual aten calls of a step
        # (autograd's gradient accumulation, scalar multiples, sigmoid, copies, fills, small sums) on csrc/glue.hip instead of ATen;
        # STRICT_GLUE: an aten call that GlueMode cannot route and that touches a CUDA tensor is an error
        self.GLUE_MODE = os.environ.get("S2F_GLUE_MODE", "0") != "0"
        self.STRICT_GLUE = os.environ.get("S2F_STRICT_GLUE", "0") != "0"
        # STRICT: a shape that leaves this package's kernels for a library / ATen path is an error, not a slower number
        self.STRICT = os.environ.get("S2F_STRICT", "0") != "0"
        # GENERAL_RESIZE: bilinear resizes that are not the exact-2x even-width case (the predict path at image sizes that are not
        # multiples of 32) run on csrc/resize.hip; False sends them to ATen through the `upsample_bilinear` fall-back site (A/B runs)
        self.GENERAL_RESIZE = True
        # DECODER_SIBLINGS: the q / k / v projection chains of the decoder's self-attention (conv1x1 -> BatchNorm -> neuron on the
        # 100-token maps) run as ONE grouped launch per stage, forward and backward, instead of three (S2F_DEC_SIBLINGS=0: one by one)
        self.DECODER_SIBLINGS = os.environ.get("S2F_DEC_SIBLINGS", "1") != "0"
        # DCN_CHANNEL_MAJOR: the pixel decoder's DCNv3 sampling core reads and writes the channel-major stream itself where an
        # (image, group) slice fits one workgroup's LDS (s2f_dcnv3_fwd_cm / _bwd_cm) instead of running on NHWC maps between two
        # transpositions, forward and backward (S2F_DCN_CM=0: the transposing route everywhere)
        self.DCN_CHANNEL_MAJOR = os.environ.get("S2F_DCN_CM", "1") != "0"

    def snapshot(self):
        """the settings a captured hipGraph depends on (scalars only)"""
        return {n: getattr(self, n) for n in self.FIELDS if n not in self.RUNTIME and n not in ("STRICT", "STRICT_GLUE")}          # (STRICT selects no launch)

    def launch_snapshot(self):
        """snapshot() plus the LAUNCH_FIELDS: everything that selects the launches a captured hipGraph bakes in"""
        return dict(self.snapshot(), **{n: getattr(self, n) for n in self.LAUNCH_FIELDS})


cfg = Config()
