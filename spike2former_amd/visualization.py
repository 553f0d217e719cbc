"""`SegLocalVisualizer` (mmseg/visualization/local_visualizer.py:16-231 on mmengine's Visualizer) and `SegVisualizationHook`
(mmseg/engine/hooks/visualization_hook.py:16-98) -- the `visualizer = dict(type='SegLocalVisualizer', vis_backends=[dict(type=
'LocalVisBackend')], name='visualizer')` and the `default_hooks.visualization` every shipped config builds.

Per image ONE `ops.seg_draw` launch (s2f_seg_draw, csrc/segdraw.hip) blends the class colours of the ground truth and of the
prediction into the decoded picture and writes the two panels side by side, where the reference runs np.unique, one full-image
masked write per class present, a float64 blend and a truncation on the host -- byte for byte the same panel.  Everything the
picture needs is in device memory at that moment (`TestAugment` staged the picture and its raw annotation there, the arg-max wrote
the prediction there); the panel stays a device tensor and is read back only when a file is written.

    vis = SegLocalVisualizer(save_dir=..., classes=..., palette=...)
    evaluate(SegTTAModel(model), batches, metric,
             hooks=[SegVisualizationHook(draw=True, interval=50, visualizer=vis, source=aug)])

Stated deviations: no window (`show`), no back end but LocalVisBackend, no palettes by data-set name, files
written with PIL; a negative label paints nothing."""
import os
import os.path as osp
import warnings

import numpy as np
import torch

from . import metrics, ops
from .registry import HOOKS, VISUALIZERS


def _tensor(x):
    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))


def _map(m):
    """a PixelData, an mmengine-style dict(data=...), a tensor or an array -> the tensor"""
    if m is None or torch.is_tensor(m) or isinstance(m, np.ndarray):
        return None if m is None else _tensor(m)
    return _tensor(m["data"] if isinstance(m, dict) else m.data)


def _has(sample, name):
    return sample is not None and ((name in sample) if isinstance(sample, dict) else hasattr(sample, name))


@VISUALIZERS.register_module()
class SegLocalVisualizer:
    """name / image / vis_backends / save_dir / classes / palette / dataset_name / alpha as the reference.  `vis_backends` may hold
    LocalVisBackend entries only, `dataset_name` needs `classes` and `palette` next to it (the reference's class_names.py tables
    are not shipped here), and nothing defaults to Cityscapes: drawing without a palette raises.  The palette is uploaded once per
    device after the meta is set."""
    _current = None

    def __init__(self, name="visualizer", image=None, vis_backends=None, save_dir=None, classes=None, palette=None, dataset_name=None,
                 alpha=0.8):
        self.name = name
        self._image = image
        for b in ([vis_backends] if isinstance(vis_backends, dict) else list(vis_backends or ())):
            kind = b.get("type") if isinstance(b, dict) else b
            kind = kind if isinstance(kind, str) else getattr(kind, "__name__", repr(kind))
            if kind.split(".")[-1] != "LocalVisBackend":
                raise NotImplementedError(f"SegLocalVisualizer: vis_backends entry {kind!r} is not implemented: files are written "
                                          f"by the LocalVisBackend rule only")
            extra = sorted(set(b) - {"type", "save_dir"}) if isinstance(b, dict) else []
            if extra:
                raise NotImplementedError(f"SegLocalVisualizer: vis_backends LocalVisBackend option(s) {extra} are not implemented")
            if isinstance(b, dict) and b.get("save_dir") is not None:
                save_dir = b["save_dir"] if save_dir is None else save_dir
        self.save_dir = save_dir
        self.alpha = float(alpha)
        self._meta, self._palette_dev = dict(classes=None, palette=None), {}
        self.set_dataset_meta(classes, palette, dataset_name)
        SegLocalVisualizer._current = self

    @classmethod
    def get_current_instance(cls):
        """the visualizer built last (mmengine's ManagerMixin rule, what the reference's hook looks up)"""
        if cls._current is None:
            raise RuntimeError("no SegLocalVisualizer has been built: build one, or pass visualizer= to the hook")
        return cls._current

    # ---- meta
    @property
    def dataset_meta(self):
        return self._meta

    @dataset_meta.setter
    def dataset_meta(self, meta):
        self.set_dataset_meta(meta.get("classes"), meta.get("palette"))

    def set_dataset_meta(self, classes=None, palette=None, dataset_name=None):
        if dataset_name is not None and not (classes and palette):
            raise NotImplementedError(f"SegLocalVisualizer: dataset_name={dataset_name!r}: the class and palette tables by data-set "
                                      f"name are not shipped: pass classes= and palette=, or set dataset_meta")
        if palette is not None and classes is None:
            classes = tuple(str(i) for i in range(len(palette)))
        if palette is not None:
            assert len(classes) == len(palette), "The length of classes should be equal to palette"
            p = np.asarray(palette)
            if p.ndim != 2 or p.shape[1] != 3 or p.min() < 0 or p.max() > 255:
                raise ValueError("palette: one RGB triple of 0 .. 255 per class")
        self._meta = dict(classes=classes, palette=palette)
        self._palette_dev = {}

    def _palette_on(self, device, palette):
        """uint8 [K, 3] on `device`; the meta's palette is uploaded once per device, any other one per call"""
        if palette is None:
            raise ValueError("SegLocalVisualizer: no palette: pass palette= (and classes=) or set dataset_meta = dict(classes=..., "
                             "palette=...) first")
        if palette is not self._meta["palette"]:
            return torch.from_numpy(np.asarray(palette, dtype=np.uint8).reshape(-1, 3)).to(device)
        device = torch.device(device)
        if device not in self._palette_dev:
            self._palette_dev[device] = torch.from_numpy(np.asarray(palette, dtype=np.uint8).reshape(-1, 3)).to(device)
        return self._palette_dev[device]

    # ---- drawing
    def _panel(self, image, gt, pred, palette, image_is_bgr=False, reduce_zero_label=False):
        maps = [_map(gt), _map(pred)]
        device = next(m.device for m in reversed(maps) if m is not None)          # the prediction's, else the ground truth's
        image = _tensor(image)
        if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
            raise ValueError("SegLocalVisualizer: image is uint8 [H, W, 3]")
        maps = [None if m is None else m.to(device, non_blocking=True) for m in maps]
        return ops.seg_draw(image.to(device, non_blocking=True), self._palette_on(device, palette), maps[0], maps[1], self.alpha,
                            bgr=image_is_bgr, reduce_zero_label=reduce_zero_label)

    def _draw_sem_seg(self, image, sem_seg, classes, palette, image_is_bgr=False):
        """image uint8 [H, W, 3] (numpy or tensor), sem_seg a PixelData or a [1, H, W] / [H, W] map -> the drawn picture, uint8
        [H, W, 3] RGB on the map's device"""
        assert palette is None or classes is None or len(classes) == len(palette), "The length of classes should be equal to palette"
        return self._panel(image, None, sem_seg, palette, image_is_bgr)

    def add_datasample(self, name, image, data_sample=None, draw_gt=True, draw_pred=True, show=False, wait_time=0, out_file=None,
                       step=0, image_is_bgr=False):
        """Draws the sample's gt_sem_seg (left) and pred_sem_seg (right) into `image` -- uint8 [H, W, 3], RGB as the reference's
        argument, or BGR with image_is_bgr -- and writes the panel to out_file, else, with a save_dir, to
        {save_dir}/vis_image/{name}_{step}.png.  The ground truth is mapped by the sample's `reduce_zero_label` meta (TestAugment
        hands on raw annotations).  -> the panel, uint8 [H, P W, 3] RGB on the maps' device, or None when nothing was drawn (no
        map to draw, or not the main process)."""
        if show:
            raise NotImplementedError("SegLocalVisualizer: show=True is not implemented: there is no display; write with out_file "
                                      "or save_dir")
        if not metrics._is_main_process():
            return None
        gt = metrics._field(data_sample, "gt_sem_seg") if draw_gt and _has(data_sample, "gt_sem_seg") else None
        pred = metrics._field(data_sample, "pred_sem_seg") if draw_pred and _has(data_sample, "pred_sem_seg") else None
        if gt is None and pred is None:
            return None
        drawn = self._panel(image, gt, pred, self._meta["palette"], image_is_bgr,
                            bool(metrics._meta(data_sample, "reduce_zero_label", False)))
        if out_file is None and self.save_dir is not None:
            out_file = osp.join(self.save_dir, "vis_image", f"{name}_{step}.png")
        if out_file is not None:
            from PIL import Image
            os.makedirs(osp.dirname(osp.abspath(out_file)), exist_ok=True)
            Image.fromarray(drawn.cpu().numpy()).save(out_file)
        return drawn


@HOOKS.register_module()
class SegVisualizationHook:
    """draw / interval / show / wait_time / backend_args as the reference; `visualizer`: the SegLocalVisualizer to draw with
    (default: the one built last); `source`: where the pictures come from -- an object with `sources()` (a TestAugment: the uint8
    pictures it staged, already in device memory) or a callable (data_batch, outputs) -> one picture per output; an object's
    `is_bgr` attribute says the pictures are BGR.  Without a source the file at the sample's `img_path` is decoded with PIL as RGB,
    where the reference decodes with mmcv (OpenCV): the distance between the two JPEG decoders has not been measured by anyone
    here (PNG is lossless in both).  `step` (default 0) goes into the file name, as the reference's runner.iter."""

    def __init__(self, draw=False, interval=50, show=False, wait_time=0., backend_args=None, visualizer=None, source=None):
        if show:
            raise NotImplementedError("SegVisualizationHook: show=True is not implemented: there is no display")
        if backend_args is not None:
            raise NotImplementedError("SegVisualizationHook: backend_args is not implemented: pictures are read from local files")
        self._visualizer = visualizer
        self.interval = int(interval)
        self.show = bool(show)
        self.wait_time = wait_time
        self.backend_args = None
        self.draw = draw
        self.source = source
        self.step = 0
        if not self.draw:
            warnings.warn("The draw is False, it means that the hook for visualization will not take effect. The results will NOT be "
                          "visualized or stored.")

    @property
    def visualizer(self):
        if self._visualizer is None:
            self._visualizer = SegLocalVisualizer.get_current_instance()
        return self._visualizer

    def _pictures(self, data_batch, outputs):
        """-> (one picture per output, whether they are BGR)"""
        if self.source is None:
            from PIL import Image
            return [np.array(Image.open(metrics._meta(o, "img_path")).convert("RGB")) for o in outputs], False
        pictures = self.source.sources() if hasattr(self.source, "sources") else self.source(data_batch, outputs)
        if len(pictures) != len(outputs):
            raise ValueError(f"SegVisualizationHook: {len(pictures)} source pictures for {len(outputs)} outputs")
        return pictures, bool(getattr(pictures, "is_bgr", getattr(self.source, "is_bgr", False)))

    def _after_iter(self, batch_idx, data_batch, outputs, mode="val"):
        """every `interval`-th iteration of a val / test loop (mmengine's every_n_inner_iters: (batch_idx + 1) % interval == 0), on
        the main process: one add_datasample per output, named {mode}_{basename(img_path)}"""
        if self.draw is False or mode == "train":
            return
        if self.interval <= 0 or (batch_idx + 1) % self.interval != 0 or not metrics._is_main_process():
            return
        pictures, bgr = self._pictures(data_batch, outputs)
        for picture, output in zip(pictures, outputs):
            name = f"{mode}_{osp.basename(metrics._meta(output, 'img_path'))}"
            self.visualizer.add_datasample(name, picture, data_sample=output, show=self.show, wait_time=self.wait_time,
                                           step=self.step, image_is_bgr=bgr)

    def after_val_iter(self, batch_idx, data_batch=None, outputs=None):
        self._after_iter(batch_idx, data_batch, outputs, "val")

    def after_test_iter(self, batch_idx, data_batch=None, outputs=None):
        self._after_iter(batch_idx, data_batch, outputs, "test")
