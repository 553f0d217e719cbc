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

`SegLocalVisualizer.draw_firing` and `FiringMapHook` draw the firing maps of firingmaps.FiringMaps the same way: one tile per
neuron, the picture under that neuron's heat map, ONE `ops.firing_draw` launch (s2f_firing_draw, csrc/firingmap.hip) per tile straight
into a grid panel, in integer arithmetic throughout.

Stated deviations: no window (`show`), no back end but LocalVisBackend, no palettes by data-set name, files
written with PIL; a negative label paints nothing; the firing maps' colour table and resampling are this package's own specification
(not OpenCV's applyColorMap / mmengine's draw_featmap) and carry no legend text."""
import json
import math
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


    # ---- firing maps
    @staticmethod
    def default_firing_lut():
        """uint8 [256, 3] RGB, blue -> cyan -> yellow -> red: for v = i / 255 and k = 3, 2, 1 for r, g, b the byte
        floor(255 clip(1.5 - |4 v - k|, 0, 1) + 0.5), in float64 on the host"""
        v = np.arange(256, dtype=np.float64)[:, None] / 255.0
        c = np.clip(1.5 - np.abs(4.0 * v - np.array([3.0, 2.0, 1.0])), 0.0, 1.0)
        return np.floor(255.0 * c + 0.5).astype(np.uint8)

    def _firing_lut_on(self, device, lut):
        """uint8 [256, 3] on `device`; the default table is built once and uploaded once per device, any other one per call"""
        if lut is not None:
            t = _tensor(lut)
            if t.dtype != torch.uint8 or tuple(t.shape) != (256, 3):
                raise ValueError("draw_firing: lut is uint8 [256, 3]")
            return t.to(device)
        cache = self.__dict__.setdefault("_firing_lut_dev", {})
        device = torch.device(device)
        if device not in cache:
            cache[device] = torch.from_numpy(self.default_firing_lut()).to(device)
        return cache[device]

    @staticmethod
    def firing_full(read, name, image, which="rate", vmax=None):
        """the plane value that maps to the last row of the colour table, an integer >= 1: the tile's own maximum (vmax None) or the
        plane value of the absolute rate / active share `vmax` -> (plane index, full)"""
        if which not in ("rate", "active"):
            raise ValueError(f"draw_firing: which={which!r}: 'rate' (plane 0) or 'active' (plane 1)")
        k = 0 if which == "rate" else 1
        if vmax is None:
            return k, max(1, int(read.planes[name][image, k].max()))
        T, C, D, passes = read.meta[name]
        return k, max(1, int(math.floor(float(vmax) * T * C * passes * (D if k == 0 else 1) + 0.5)))

    def draw_firing(self, picture, read, image=0, names=None, which="rate", arrangement=None, alpha=0.5, vmax=None, lut=None,
                    image_is_bgr=False, out_file=None, name="firing", step=0):
        """One tile per neuron of `read` (a firingmaps.FiringMapRead; `names`: a subset, in this order): `picture` -- uint8
        [H, W, 3], RGB or BGR with image_is_bgr -- under the heat map of image `image` of that neuron, plane 0 (`which="rate"`) or 1
        ("active") resampled to H x W.  The tiles fill a grid row by row: `arrangement=(rows, cols)`, default the smallest near-square
        one (cols = ceil(sqrt(n))); unused tiles stay black.  `vmax`: None -- every tile is scaled to its own maximum --, or one
        absolute rate (share, for "active") for all tiles, so that layers and pictures compare.  `lut`: uint8 [256, 3] RGB (default:
        default_firing_lut).  ONE ops.firing_draw launch per tile, written straight into the panel.  The panel goes to out_file, else,
        with a save_dir, to {save_dir}/vis_image/{name}_{step}.png.  -> the panel, uint8 [rows H, cols W, 3] RGB on the device."""
        names = list(read.names if names is None else names)
        if not names:
            raise ValueError("draw_firing: no neuron to draw (the read holds no map)")
        missing = [n for n in names if n not in read.planes]
        if missing:
            raise KeyError(f"draw_firing: no map of {missing[0]!r} in the read")
        picture = _tensor(picture)
        if picture.dtype != torch.uint8 or picture.dim() != 3 or picture.shape[2] != 3:
            raise ValueError("draw_firing: picture is uint8 [H, W, 3]")
        if not picture.is_cuda and torch.cuda.is_available():
            picture = picture.cuda(non_blocking=True)
        device, (H, W) = picture.device, picture.shape[:2]
        n = len(names)
        if arrangement is None:
            cols = int(math.ceil(math.sqrt(n)))
            rows = (n + cols - 1) // cols
        else:
            rows, cols = (int(v) for v in arrangement)
            if rows < 1 or cols < 1 or rows * cols < n:
                raise ValueError(f"draw_firing: arrangement {tuple(arrangement)} holds fewer than {n} tiles")
        table = self._firing_lut_on(device, lut)
        panel = torch.zeros(rows * H, cols * W, 3, dtype=torch.uint8, device=device)
        for i, neuron in enumerate(names):
            k, full = self.firing_full(read, neuron, image, which, vmax)
            plane = torch.from_numpy(np.ascontiguousarray(read.planes[neuron][image, k])).to(device, non_blocking=True)
            r, c = divmod(i, cols)
            ops.firing_draw(picture, plane, full, table, alpha, bgr=image_is_bgr, out=panel[r * H:(r + 1) * H, c * W:(c + 1) * W])
        if out_file is None and self.save_dir is not None:
            out_file = osp.join(self.save_dir, "vis_image", f"{name}_{step}.png")
        if out_file is not None:
            from PIL import Image
            os.makedirs(osp.dirname(osp.abspath(out_file)), exist_ok=True)
            Image.fromarray(panel.cpu().numpy()).save(out_file)
        return panel


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


@HOOKS.register_module()
class FiringMapHook:
    """For `evaluate(..., hooks=[...])`: the firing maps of `maps` (a firingmaps.FiringMaps) of every batch with (batch_idx + 1) %
    interval == 0, as SegVisualizationHook picks its batches -- per sample one `draw_firing` panel named {mode}_{basename}_firing
    (draw=False: none), the pictures taken from `source` by SegVisualizationHook's rules, and one line of the read's `summary()` per
    drawn batch appended to {save_dir}/vis_data/firing_maps.jsonl; then the maps are cleared.  The neurons are hooked ONLY for the
    batches that will be drawn: the hook attaches `maps` after the batch in front of a due one (at construction when the first batch
    is due) and detaches it after drawing, so every other batch runs the fast routes and GraphedPredict's replays.  `draw_kwargs` go to
    `draw_firing` (names, which, arrangement, alpha, vmax, lut)."""

    def __init__(self, maps, interval=50, visualizer=None, source=None, draw=True, **draw_kwargs):
        self.maps, self.interval, self.draw, self.source = maps, int(interval), bool(draw), source
        self._visualizer = visualizer
        self.draw_kwargs = draw_kwargs
        self.step = 0
        if self.interval < 1:
            raise ValueError(f"FiringMapHook: interval {interval} is at least 1")
        if self._due(0):
            maps.attach()
        else:
            maps.detach()

    visualizer = SegVisualizationHook.visualizer
    _pictures = SegVisualizationHook._pictures

    def _due(self, batch_idx):
        return (batch_idx + 1) % self.interval == 0

    def _after_iter(self, batch_idx, data_batch, outputs, mode):
        if self._due(batch_idx) and self.maps.attached:
            read = self.maps.read()
            main = metrics._is_main_process() and bool(read.names)
            if main and self.draw:
                pictures, bgr = self._pictures(data_batch, outputs)          # (the source sees the neurons still hooked)
            self.maps.detach()
            self.maps.clear()
            if main:
                vis = self.visualizer
                names = [f"{mode}_{osp.basename(metrics._meta(o, 'img_path'))}_firing" for o in outputs]
                if self.draw:
                    for i, (picture, name) in enumerate(zip(pictures, names)):
                        vis.draw_firing(picture, read, image=i, image_is_bgr=bgr, name=name, step=self.step, **self.draw_kwargs)
                if vis.save_dir is not None:
                    path = osp.join(vis.save_dir, "vis_data", "firing_maps.jsonl")
                    os.makedirs(osp.dirname(path), exist_ok=True)
                    with open(path, "a") as f:
                        f.write(json.dumps(dict(batch=batch_idx, step=self.step, samples=names, maps=read.summary())) + "\n")
        if self._due(batch_idx + 1):
            self.maps.clear()
            self.maps.attach()

    def after_val_iter(self, batch_idx, data_batch=None, outputs=None):
        self._after_iter(batch_idx, data_batch, outputs, "val")

    def after_test_iter(self, batch_idx, data_batch=None, outputs=None):
        self._after_iter(batch_idx, data_batch, outputs, "test")
