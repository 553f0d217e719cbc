"""Thin callers of the hot path: `EncoderDecoder` -- extract_feat / _forward / loss / predict with
`inference`, `whole_inference`, `slide_inference` (mmseg/models/segmentors/encoder_decoder.py:118-350) and
`postprocess_result` (mmseg/models/segmentors/base.py:127-200) -- and `ResetModelHook`
(mmseg/engine/hooks/resetmodel_hook.py:9-37).  The post-processing arithmetic (bilinear resizes, softmax / sigmoid, the class
einsum, window averaging, argmax) is plain tensor glue around the kernels and is pinned against the reference's own files
by tests/golden/predict_a13.npz (oracle/gen_golden_a13.py); on fp32 CUDA tensors the resizes, the arg-max and the window averaging
of `slide_inference` (csrc/slide.hip) run on the package's kernels.  The runner is out of scope."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .data_preprocessor import PixelData, SegDataSample
from .neuron import reset_net
from .registry import HOOKS, MODELS, ConfigDict


def _axis_covered(size, extent, stride, count):
    """whether the `count` windows of one axis of ops.slide_grid (window i starts at min(i * stride, size - extent)) leave no
    coordinate uncovered: neighbours start at most one extent apart"""
    if count == 1:
        return True
    return (count < 3 or stride <= extent) and (size - extent) - (count - 2) * stride <= extent


@MODELS.register_module()
class EncoderDecoder(nn.Module):
    def __init__(self, backbone, decode_head, neck=None, auxiliary_head=None, train_cfg=None, test_cfg=None,
                 data_preprocessor=None, pretrained=None, init_cfg=None):
        super().__init__()
        if neck is not None or auxiliary_head is not None:
            raise NotImplementedError("neck / auxiliary_head are not used by the Spike2Former configs")
        self.data_preprocessor = MODELS.build(data_preprocessor) if isinstance(data_preprocessor, dict) else data_preprocessor
        self.backbone = MODELS.build(backbone)
        self.decode_head = MODELS.build(decode_head)
        self.align_corners = self.decode_head.align_corners
        self.num_classes = self.decode_head.num_classes
        self.out_channels = self.decode_head.out_channels
        self.train_cfg, self.test_cfg = train_cfg, test_cfg

    def extract_feat(self, inputs):
        return self.backbone(inputs)

    def _forward(self, inputs, data_samples=None):
        """mode='tensor': (all_cls_scores, all_mask_preds)."""
        return self.decode_head.forward(self.extract_feat(inputs), data_samples)

    def _encode_decode(self, inputs, batch_img_metas):
        return self.decode_head.predict(self.extract_feat(inputs), batch_img_metas, self.test_cfg)

    def encode_decode(self, inputs, batch_img_metas):
        """-> seg logits [N, K, H, W] (encoder_decoder.py:126-136).

        test_cfg['graph'] = True | dict(max_graphs=..., capture_after=..., warmup=...) (an addition; absent: every launch issued
        from here, as before): the pass goes through a graph.GraphedPredict kept on the segmentor -- a shape seen `capture_after`
        times is captured into a hipGraph and replayed from then on, as the STATELESS inference (membranes reset before the pass and
        left reset after it); inputs it cannot replay (CPU tensors, train mode, autograd on, neurons with counters or hooks, a live OpCensus) run
        the line below unchanged.  A replay returns the graph's static output: whatever leaves this class is cloned (`_own`)."""
        gp = self.graphed_predict()
        if gp is not None:
            return gp(inputs, batch_img_metas)
        return self._encode_decode(inputs, batch_img_metas)

    def graphed_predict(self):
        """the GraphedPredict of test_cfg['graph'] (built at first use; `.census` tells what it did), None without the option"""
        opt = (self.test_cfg or {}).get("graph")
        if not opt:
            return None
        gp = self.__dict__.get("_graphed_predict")
        if gp is None:
            from .graph import GraphedPredict
            gp = GraphedPredict(self, fn=self._encode_decode, **(dict(opt) if isinstance(opt, dict) else {}))
            self.__dict__["_graphed_predict"] = gp
        return gp

    def _own(self, seg_logits):
        """`seg_logits` as a tensor the caller may keep: a copy where it is a captured graph's static output"""
        gp = self.__dict__.get("_graphed_predict")
        return seg_logits.clone() if gp is not None and gp.is_static(seg_logits) else seg_logits

    # ---- inference (encoder_decoder.py:246-350)
    def whole_inference(self, inputs, batch_img_metas):
        return self.encode_decode(inputs, batch_img_metas)

    def slide_inference(self, inputs, batch_img_metas, route=None):
        """Overlapping windows of test_cfg.crop_size at test_cfg.stride, logits averaged by coverage (:246-296).

        Two routes give the same bits.  fp32 CUDA inputs whose `encode_decode` returns fp32 CUDA logits stay on the package's
        kernels: every group of windows is merged by ONE ops.slide_accumulate launch (no padded temporary, no count map, no final
        division pass).  Everything else -- CPU tensors, other dtypes, or `route="torch"` (the measurement baseline of
        tools/slide_probe.py) -- runs the reference's loop: F.pad, preds +=, count_mat += 1, preds / count_mat.

        test_cfg['window_batch'] = g (an addition; absent: the reference's protocol, one window per `encode_decode` call at batch
        B, the membranes carried from window to window): the windows run g at a time as one window-major batch [g B, 3, eh, ew]
        (the last group may be smaller), with the membranes reset before every group -- each window is then the stateless
        inference of the training path (the stated deviation of SegTTAModel's reset per view).

        The reference asserts after its loop that no pixel is left uncovered; coverage depends on the grid alone, so it is checked
        here before any window runs (the same AssertionError)."""
        assert route in (None, "torch"), f"route {route!r}: None or 'torch'"
        stride, crop = tuple(self.test_cfg["stride"]), tuple(self.test_cfg["crop_size"])
        (h_stride, w_stride), (h_crop, w_crop) = stride, crop
        batch_size, _, h_img, w_img = inputs.size()
        h_grids, w_grids, eh, ew = ops.slide_grid(h_img, w_img, crop, stride)
        assert _axis_covered(h_img, eh, h_stride, h_grids) and _axis_covered(w_img, ew, w_stride, w_grids)
        group = self.test_cfg.get("window_batch")
        if group is not None and (int(group) != group or group < 1):
            raise ValueError(f"test_cfg['window_batch'] = {group!r}: an integer >= 1")
        if group is None and self.test_cfg.get("graph"):
            raise ValueError("test_cfg['graph'] with mode='slide' needs test_cfg['window_batch']: without it the membranes are carried "
                             "from window to window, which the replay of a stateless pass cannot reproduce")
        boxes = []
        for h_idx in range(h_grids):
            for w_idx in range(w_grids):
                y1, x1 = h_idx * h_stride, w_idx * w_stride
                y2, x2 = min(y1 + h_crop, h_img), min(x1 + w_crop, w_img)
                boxes.append((max(y2 - h_crop, 0), y2, max(x2 - w_crop, 0), x2))
        ours = route is None and inputs.is_cuda and inputs.dtype == torch.float32
        preds = count_mat = None
        step = 1 if group is None else int(group)
        whole = inputs.contiguous() if ours and group is not None else inputs          # what ops.slide_windows cuts from
        for w0 in range(0, len(boxes), step):
            n = min(step, len(boxes) - w0)
            if group is None:
                y1, y2, x1, x2 = boxes[w0]
                crop_img = inputs[:, :, y1:y2, x1:x2]
            else:
                reset_net(self)
                if ours:
                    crop_img = ops.slide_windows(whole, crop, stride, w0, n).view(n * batch_size, -1, eh, ew)
                else:
                    crop_img = torch.cat([inputs[:, :, y1:y2, x1:x2] for y1, y2, x1, x2 in boxes[w0:w0 + n]])
            batch_img_metas[0]["img_shape"] = crop_img.shape[2:]          # as the reference: only the first meta
            crop_seg_logit = self.encode_decode(crop_img, batch_img_metas)
            if preds is None:
                ours = ours and crop_seg_logit.is_cuda and crop_seg_logit.dtype == torch.float32
                shape = (batch_size, self.out_channels, h_img, w_img)
                if ours:
                    preds = inputs.new_empty(shape)          # (every pixel is written: the grid covers the picture)
                else:
                    preds, count_mat = inputs.new_zeros(shape), inputs.new_zeros((batch_size, 1, h_img, w_img))
            if ours:
                ops.slide_accumulate(preds, crop_seg_logit.contiguous(), crop, stride, w0)
                continue
            for k, (y1, y2, x1, x2) in enumerate(boxes[w0:w0 + n]):
                preds += F.pad(crop_seg_logit[k * batch_size:(k + 1) * batch_size],
                               (int(x1), int(preds.shape[3] - x2), int(y1), int(preds.shape[2] - y2)))
                count_mat[:, :, y1:y2, x1:x2] += 1
        if ours:
            return preds
        assert (count_mat == 0).sum() == 0
        return preds / count_mat

    def inference(self, inputs, batch_img_metas):
        mode = (self.test_cfg or {}).get("mode", "whole")
        assert mode in ("slide", "whole"), f'Only "slide" or "whole" test mode are supported, but got {mode}.'
        if mode == "slide":
            return self.slide_inference(inputs, batch_img_metas)
        return self.whole_inference(inputs, batch_img_metas)

    def postprocess_result(self, seg_logits, data_samples=None):
        """Logits -> per-image results (base.py:127-200): padding removed, flip undone, resized to `ori_shape`
        (bilinear, the head's align_corners), arg-max (sigmoid threshold for one class).  fp32 CUDA logits: crop + flip + resize
        (+ the one-class sigmoid) are one s2f_resize_fwd pass and the arg-max / threshold one s2f_seg_argmax pass."""
        batch_size, C, H, W = seg_logits.shape
        only_prediction = data_samples is None
        if only_prediction:
            data_samples = [SegDataSample() for _ in range(batch_size)]
        ours = seg_logits.is_cuda and seg_logits.dtype == torch.float32
        if ours:
            seg_logits = seg_logits.contiguous()
        threshold = getattr(self.decode_head, "threshold", 0.3)
        # test_cfg['seg_logits'] = False (an addition; absent: as before): fp32 CUDA logits go straight to the label map, one
        # s2f_seg_label launch per image with no [K, H, W] planes at `ori_shape`, and the samples carry `pred_sem_seg` alone
        labels_only = ours and (self.test_cfg or {}).get("seg_logits", True) is False
        for i in range(batch_size):
            if not only_prediction:
                img_meta = data_samples[i].metainfo
                padding_size = img_meta["img_padding_size"] if "img_padding_size" in img_meta else img_meta.get("padding_size", [0] * 4)
                padding_left, padding_right, padding_top, padding_bottom = padding_size
                flip = img_meta.get("flip", None)
                if flip:
                    flip_direction = img_meta.get("flip_direction", None)
                    assert flip_direction in ["horizontal", "vertical"]
                if labels_only:
                    data_samples[i].pred_sem_seg = PixelData(ops.seg_label(
                        seg_logits[i], tuple(img_meta["ori_shape"]), crop=(padding_top, padding_bottom, padding_left, padding_right),
                        flip=flip_direction if flip else None, align_corners=self.align_corners, threshold=threshold))
                    continue
                if ours:
                    i_seg_logits = ops.resize_window(seg_logits[i], tuple(img_meta["ori_shape"]),
                                                     crop=(padding_top, padding_bottom, padding_left, padding_right),
                                                     flip=flip_direction if flip else None, align_corners=self.align_corners,
                                                     sigmoid=C == 1)
                    i_seg_pred = ops.seg_argmax(i_seg_logits, threshold, float_out=True)
                    data_samples[i].seg_logits = PixelData(i_seg_logits)
                    data_samples[i].pred_sem_seg = PixelData(i_seg_pred)
                    continue
                i_seg_logits = seg_logits[i:i + 1, :, padding_top:H - padding_bottom, padding_left:W - padding_right]
                if flip:
                    i_seg_logits = i_seg_logits.flip(dims=(3,)) if flip_direction == "horizontal" else i_seg_logits.flip(dims=(2,))
                i_seg_logits = F.interpolate(i_seg_logits, size=tuple(img_meta["ori_shape"]), mode="bilinear",
                                             align_corners=self.align_corners).squeeze(0)
            else:
                i_seg_logits = seg_logits[i]
            if ours and C > 1:
                i_seg_pred = ops.seg_argmax(i_seg_logits)
            elif ours:
                i_seg_logits = i_seg_logits.sigmoid()
                i_seg_pred = ops.seg_argmax(i_seg_logits, threshold, float_out=True)
            elif C > 1:
                i_seg_pred = i_seg_logits.argmax(dim=0, keepdim=True)
            else:
                i_seg_logits = i_seg_logits.sigmoid()
                i_seg_pred = (i_seg_logits > threshold).to(i_seg_logits)
            if not labels_only:
                data_samples[i].seg_logits = PixelData(i_seg_logits)
            data_samples[i].pred_sem_seg = PixelData(i_seg_pred)
        return data_samples

    def predict(self, inputs, data_samples=None):
        """-> list of SegDataSample with `seg_logits` / `pred_sem_seg` (encoder_decoder.py:190-223)."""
        if data_samples is not None:
            batch_img_metas = [d.metainfo for d in data_samples]
        else:
            batch_img_metas = [dict(ori_shape=inputs.shape[2:], img_shape=inputs.shape[2:], pad_shape=inputs.shape[2:],
                                    padding_size=[0, 0, 0, 0])] * inputs.shape[0]
        seg_logits = self.inference(inputs, batch_img_metas)
        if data_samples is None:          # the samples then carry views of the logits themselves
            seg_logits = self._own(seg_logits)
        return self.postprocess_result(seg_logits, data_samples)

    def preprocess(self, data, training=False):
        """data_preprocessor(data, training) -> dict(inputs, data_samples).  Without a data_preprocessor the inputs are only
        stacked (a list of [3, H, W]) and moved to the model's device.  A batch marked `preprocessed` (what augment.TestAugment
        returns: resized, normalised and padded on the device already) passes through untouched."""
        if not training and isinstance(data, dict) and data.get("preprocessed"):
            return dict(inputs=data["inputs"], data_samples=data["data_samples"])
        if self.data_preprocessor is not None:
            return self.data_preprocessor(data, training)
        if not isinstance(data, dict):
            data = dict(inputs=data[0], data_samples=data[1] if len(data) > 1 else None)
        inputs = data["inputs"]
        inputs = torch.stack(list(inputs)) if isinstance(inputs, (list, tuple)) else inputs
        return dict(inputs=inputs.to(next(self.parameters()).device).float(), data_samples=data.get("data_samples"))

    def test_step(self, data):
        """mmengine BaseModel.test_step: data_preprocessor(data, False), then mode='predict' -> list of SegDataSample."""
        return self(**self.preprocess(data, False), mode="predict")

    def forward(self, inputs, data_samples=None, mode="tensor"):
        """mode = 'tensor' | 'loss' | 'predict' as in the reference (base.py:86-124); 'logits' (an addition) stops after
        `inference`: the seg-logit tensor [N, K, H, W]."""
        if inputs.is_cuda:
            ops.begin_step(inputs.device)          # rewind + clear the per-step reduction-workspace arena
        if mode == "tensor":
            return self._forward(inputs, data_samples)
        if mode == "predict":
            return self.predict(inputs, data_samples)
        if mode == "logits":
            metas = ([d.metainfo if hasattr(d, "metainfo") else d for d in data_samples] if data_samples
                     else [dict(img_shape=tuple(inputs.shape[-2:]))] * inputs.shape[0])
            return self._own(self.inference(inputs, metas))
        if mode == "loss":
            return self.decode_head.loss(self.extract_feat(inputs), data_samples, self.train_cfg)
        raise RuntimeError(f'Invalid mode "{mode}". Only supports loss, predict and tensor mode')


@HOOKS.register_module()
class ResetModelHook:
    """Zero every neuron membrane before each train / val / test iteration (resetmodel_hook.py:17-37)."""

    def _reset(self, runner):
        torch.cuda.synchronize()
        reset_net(runner.model if hasattr(runner, "model") else runner)

    before_train_iter = before_val_iter = before_test_iter = lambda self, runner, *a, **k: self._reset(runner)


def headline_loss(all_cls_scores, all_mask_preds):
    """Scalar loss of the benchmark step: on-device, data-independent:
    all_cls_scores.float().mean() + all_mask_preds.float().mean()."""
    return ops.mean_all(all_cls_scores.float()) + ops.mean_all(all_mask_preds.float())
