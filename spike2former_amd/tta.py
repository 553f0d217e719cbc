"""Test-time augmentation: `SegTTAModel` (mmseg/models/segmentors/seg_tta.py:14-48 on mmengine's BaseTTAModel), built from
`dict(type='SegTTAModel', module=...)` as `configs/_base_/default_runtime.py:23` configures it, or wrapped around a model.

The views of one image (the reference's tta_pipeline: 6 scales x 2 flips, ade20k.py:28-43) arrive already resized by the data
pipeline, as in mmengine: `augment.TestAugment.from_cfg(tta_pipeline, data_preprocessor)` is that pipeline on the device (one copy
and one launch from the decoded picture to all the views, marked `preprocessed` so that `module.preprocess` passes them through);
views prepared elsewhere go through the module's data preprocessor as before.  Each view's seg logits are softmax-ed (one class: sigmoid) and summed in view order, the sum is divided
once by the number of views, and the arg-max (one class: the head's threshold) is the merged prediction.  On fp32 CUDA logits
`test_step` streams: every view's logits [K, Hp, Wp] go through ONE s2f_tta_accumulate pass -- padding crop, flip undone, bilinear
resize to `ori_shape`, softmax, += into a [K, H, W] accumulator -- so no view's full-resolution logits are kept, and
s2f_tta_finish divides and takes the arg-max.

Stated deviation: the membrane state is reset before EVERY view.  The reference resets the neurons once per
test iteration (ResetModelHook.before_test_iter), and a TTA iteration is all the views of an image: view 2 (same scale, flipped)
would integrate onto the membrane view 1 left behind, and view 3 (a new scale) fails in `self.v + x` on a shape mismatch
(Qtrick_architecture/clock_driven/neuron.py:459-460) -- the reference's TTA does not run as shipped.  Here each view is the
stateless inference of the training path."""
import torch

from . import ops
from .data_preprocessor import PixelData
from .neuron import reset_net
from .registry import MODELS


@MODELS.register_module()
class SegTTAModel(torch.nn.Module):
    def __init__(self, module, data_preprocessor=None):
        super().__init__()
        self.module = MODELS.build(module) if isinstance(module, dict) else module
        self.data_preprocessor = data_preprocessor

    @staticmethod
    def split_views(data):
        """mmengine BaseTTAModel.test_step's split: a dict of per-view lists -> one dict per view; a list of per-view batches
        (one list per field) -> one list per view"""
        if isinstance(data, dict):
            n = len(data[next(iter(data))])
            return [{k: v[i] for k, v in data.items()} for i in range(n)]
        if isinstance(data, (list, tuple)):
            return [[d[i] for d in data] for i in range(len(data[0]))]
        raise TypeError(f"data should be a dict or a list / tuple, but got {type(data)}")

    def _view_logits(self, view):
        """one view: reset the membranes, preprocess, infer -> (seg logits [B, K, Hp, Wp], the view's data samples)"""
        m = self.module
        reset_net(m)
        data = m.preprocess(view, False)
        inputs, samples = data["inputs"], data["data_samples"]
        if inputs.is_cuda:
            ops.begin_step(inputs.device)
        return m.inference(inputs, [d.metainfo for d in samples]), samples

    def test_step(self, data):
        """mmengine BaseTTAModel.test_step: the views' predictions merged per image (merge_preds' semantics); on fp32 CUDA the
        views stream through the accumulation kernels instead of being kept"""
        views = self.split_views(data)
        p = next(self.module.parameters())
        if not (p.is_cuda and p.dtype == torch.float32):
            return self.merge_preds(list(zip(*[self._predict_view(v) for v in views])))
        with torch.no_grad():
            for n, view in enumerate(views):
                logits, samples = self._view_logits(view)
                if n == 0:
                    firsts = samples
                    accs = [torch.empty(logits.shape[1], *tuple(d.metainfo["ori_shape"]), dtype=torch.float32, device=logits.device)
                            for d in samples]
                for i, d in enumerate(samples):
                    meta = d.metainfo
                    left, right, top, bottom = meta["img_padding_size"] if "img_padding_size" in meta else meta.get("padding_size", [0] * 4)
                    ops.tta_accumulate(accs[i], logits[i], n == 0, crop=(top, bottom, left, right),
                                       flip=meta.get("flip_direction") if meta.get("flip", None) else None,
                                       align_corners=self.module.align_corners, pre_sigmoid=logits.shape[1] == 1)
                if n == len(views) - 1:          # the merged sample is the last view's (seg_tta.py:39-46)
                    last = self.module.postprocess_result(logits, samples)
        threshold = getattr(self.module.decode_head, "threshold", 0.3)
        for i, d in enumerate(last):
            self._finish_sample(d, firsts[i], ops.tta_finish(accs[i], len(views), threshold))
        return last

    def _predict_view(self, view):
        reset_net(self.module)
        return self.module.test_step(view)

    @staticmethod
    def _finish_sample(d, first, seg_pred):
        d.pred_sem_seg = PixelData(seg_pred)
        if hasattr(first, "gt_sem_seg"):
            d.gt_sem_seg = first.gt_sem_seg
        d.set_metainfo({"img_path": first.metainfo.get("img_path")})

    def merge_preds(self, data_samples_list):
        """seg_tta.py:14-48: per image, the views' data samples (seg_logits at `ori_shape`) -> ONE sample -- the last view's, with
        the merged `pred_sem_seg` [1, H, W] (mmengine's PixelData stores a 2-D map as [1, H, W]) and the first view's `gt_sem_seg`
        (if present) and `img_path`.  One class: the post-processed seg_logits are already sigmoid and get a second sigmoid here, as in
        the reference.  fp32 CUDA logits: s2f_tta_accumulate / s2f_tta_finish; otherwise plain torch."""
        out_channels = self.module.out_channels
        threshold = getattr(self.module.decode_head, "threshold", 0.3)
        predictions = []
        for data_samples in data_samples_list:
            seg_logits = data_samples[0].seg_logits.data
            if seg_logits.is_cuda and seg_logits.dtype == torch.float32:
                acc = torch.empty(seg_logits.shape, dtype=torch.float32, device=seg_logits.device)
                for n, data_sample in enumerate(data_samples):
                    ops.tta_accumulate(acc, data_sample.seg_logits.data, n == 0)
                seg_pred = ops.tta_finish(acc, len(data_samples), threshold)
            else:
                logits = torch.zeros(seg_logits.shape).to(seg_logits)
                for data_sample in data_samples:
                    seg_logit = data_sample.seg_logits.data
                    logits += seg_logit.softmax(dim=0) if out_channels > 1 else seg_logit.sigmoid()
                logits /= len(data_samples)
                if out_channels == 1:
                    seg_pred = (logits > threshold).to(logits).squeeze(1)
                else:
                    seg_pred = logits.argmax(dim=0)[None]
            self._finish_sample(data_samples[-1], data_samples[0], seg_pred)
            predictions.append(data_samples[-1])
        return predictions
