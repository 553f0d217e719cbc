"""torch.autograd wrappers around the C ABI, by kernel family: neuron (lif.hip), bn (bn_lif.hip), gemm (pgemm / gemm / gemm_bf16),
conv (dwconv.hip + the k x k lowering), attention (sdsa.hip, dcnv3.hip), layout (transpose.hip, the fan-out sum), reduce (glue.hip's
sums and fill), resize (upsample.hip, resize.hip: differentiable), predict (resize.hip: inference post-processing; slide.hip), pipeline
(augment.hip), segeval (segmetric.hip, segdraw.hip), census (opcensus.hip), firingmap (firingmap.hip), maskloss (maskloss.hip, lsa.hip), trainstate
(trainstate.hip: the training loop's state copy and log ring; firinglog.hip: the firing log's row; gradlog.hip: the gradient log's
row), seglog (seglog.hip: the segmentation log's row), matchlog (matchlog.hip: the match log's row), ema (ema.hip: the weight average's update and swap); `wcache` holds the cached bf16 conversions of the weights that the matrix-core products multiply by, `core`
the shared plumbing and `config` the process-global switches that are left (ops.cfg: runtime objects, semantics, debugging aids and
the A/B switches the tests and bench.py set).  `ops.NAME` keeps working for every function and for every switch: reading or assigning
`ops.STRICT`, `ops.GRAD_SINKS`, ... goes to `ops.cfg`; assigning an ALL-CAPS name that is no switch raises instead of creating a
module attribute nothing reads."""
import sys
import types

from . import (attention, bn, census, config, conv, core, ema, firingmap, gemm, layout, maskloss, matchlog, neuron, pipeline, predict, reduce, resize,
               segeval, seglog, trainstate, wcache)
from .config import cfg
from . import glue_mode as glue  # noqa: F401  (the module: ops.glue.ROUTED / UNROUTED / HANDLERS)
from .glue_mode import GlueMode, glue_mode  # noqa: F401  (ops.glue_mode(): the context manager)

for _m in (core, layout, reduce, resize, predict, pipeline, segeval, census, firingmap, maskloss, neuron, attention, bn, wcache, gemm, conv,
           trainstate, seglog, matchlog, ema):
    for _k, _v in vars(_m).items():
        if not _k.startswith("__") and _k != "cfg" and not isinstance(_v, types.ModuleType):
            globals()[_k] = _v
del _m, _k, _v


class _OpsModule(types.ModuleType):
    """module attribute access for the switches forwards to ops.cfg (they are not module attributes)"""

    def __getattr__(self, name):
        if name in config.Config.FIELDS or name in config.Config.LAUNCH_FIELDS:
            return getattr(cfg, name)
        raise AttributeError(f"module 'spike2former_amd.ops' has no attribute {name!r}")

    def __setattr__(self, name, value):
        if name in config.Config.FIELDS or name in config.Config.LAUNCH_FIELDS:
            setattr(cfg, name, value)
        elif name.isupper() and name not in self.__dict__:
            raise AttributeError(f"module 'spike2former_amd.ops' has no switch {name!r}: the switches live in ops.cfg "
                                 f"(ops.cfg.FIELDS); a retired one is fixed at the value docs/EXPERIMENTS.md lists")
        else:
            super().__setattr__(name, value)


sys.modules[__name__].__class__ = _OpsModule
