"""spike2former_amd -- the Spike2Former data-parallel hot path on MI355X (gfx950).

Importing the package loads `libs2f_hip.so` (hand-written HIP kernels behind the C ABI of include/s2f.h) and fails
loudly when it is missing.  The modules register under the reference's MODELS type names."""
from . import _lib  # noqa: F401  (raises ImportError when the HIP library is not built)
from . import ops  # noqa: F401
from .backbone_sdtv2 import Spiking_vit_MetaFormer  # noqa: F401
from .backbone_sdtv3 import Multispike_norm, Spiking_vit_MetaFormerv2  # noqa: F401
from .configs import WORKLOADS, model_cfg  # noqa: F401
from .data_preprocessor import SegDataPreProcessor, SegDataSample  # noqa: F401
from .devring import DeviceRing  # noqa: F401
from .firing import FiringLog, FiringRead, FiringRecorder  # noqa: F401
from .firingmaps import FiringMapRead, FiringMaps  # noqa: F401
from .gradlog import GradLog, GradRead  # noqa: F401
from .energy import EnergyReport, OpCensus  # noqa: F401
from .loss import MaskFormerLoss, seg_to_instances  # noqa: F401
from .maskformer_head import MaskFormerHead  # noqa: F401
from .neuron import LIFNode, Q_IFNode, Quant, reset_net, set_keep_membrane  # noqa: F401
from .pixel_decoder import DCNTransformerEncoderPixelDecoder  # noqa: F401
from .registry import HOOKS, METRICS, MODELS, VISUALIZERS, ConfigDict, register_upstream  # noqa: F401
from . import reparam  # noqa: F401
from .graph import CapturePolicy, GraphedPredict  # noqa: F401
from .segmentor import EncoderDecoder, ResetModelHook, headline_loss  # noqa: F401
from .tta import SegTTAModel  # noqa: F401
from .metrics import ConfusionMatrix, IoUMetric, evaluate  # noqa: F401
from .seglog import SegLog, SegRead  # noqa: F401
from .matchlog import MatchLog, MatchRead  # noqa: F401
from .augment import TestAugment, TrainAugment  # noqa: F401
from .visualization import FiringMapHook, SegLocalVisualizer, SegVisualizationHook  # noqa: F401
from .train import LinearThenPoly, OptimWrapper, parse_losses, train_step  # noqa: F401
from .ema import WeightEMA  # noqa: F401
from .runner import CheckpointHook, EMAHook, LoggerHook, ParamSchedulerHook, TrainLog, TrainLoop, TrainState  # noqa: F401

__version__ = "0.1.0"
