"""`TrainAugment`: the shipped configs' `train_pipeline` -- a resize -> RandomCrop(cat_max_ratio) -> RandomFlip ->
PhotoMetricDistortion (mmseg/datasets/transforms/transforms.py:215-331, 575-737) -- and the training branch of
`SegDataPreProcessor` as two HIP launches (csrc/augment.hip) from the decoded uint8 pictures of a batch to the [B, 3, Hc, Wc] fp32 /
[B, Hc, Wc] uint8 tensors a training step replays on.  File loading is not here: the caller hands in decoded
BGR pictures and raw annotations.

The configs ship two resize rules, and the kernels, functions of the table's (h0, w0, H, W), serve both; only `draw` differs:
  * RandomResize(scale, ratio_range=(0.5, 2.0), keep_ratio=True), mmcv's: a continuous ratio on a (long, short) box
    (`resized_size`).  The pipeline of configs/_base_/datasets/*.py, which the two VOC and the two FPN configs under
    configs/Spike2Former/ keep.
  * RandomChoiceResize(scales, resize_type='ResizeShortestEdge', max_size), mmcv's choice among mmseg's ResizeShortestEdge
    (transforms.py:1373-1404): one of 16 short-edge lengths, uniformly, under a cap on the long edge (`shortest_edge_size`).  The
    pipeline the six MaskFormer / Spike2former configs for ADE20K, Cityscapes and COCO-Stuff set for themselves (320 .. 1280
    under 2560; Cityscapes 512 .. 2048 under 4096).

    aug = TrainAugment.from_cfg(train_pipeline, data_preprocessor, batch_size=2, seed=0)
    step = GraphedHungarianStep(model, example_in, example_seg, red, assign="device")
    for images, segs in loader:                                   # lists of uint8 [h0, w0, 3] BGR / [h0, w0] arrays
        aug(images, segs, out=(step.static_in, step.static_seg))  # one H2D copy + two launches, queued; nothing waits for the GPU
        losses = step()

The host draws the random numbers (`draw`), the kernels are functions of the parameter table.  Two deliberate differences from the
reference's stream of random numbers, neither of which changes a distribution:
  * `draw` always consumes the SAME number of variates per image (the ratio or the choice among the scales, eleven crop origins,
    the flip and every photometric switch and value, used or not), where the reference draws a new crop origin only after a
    refused one and a photometric value only behind its switch.  The eleven origins are independent and identically distributed
    and the chosen one is the first that passes among the first ten, else the eleventh: the distribution of the chosen crop is
    the reference's.
  * the generator is a `numpy.random.Generator` seeded from (seed, rank), not mmcv's use of the global `numpy.random` state: a run
    here does not reproduce the reference's sequence of augmentations, only its distribution.

`TestAugment` (below) is the test-time counterpart: the configs' `test_pipeline` / `tta_pipeline` and the pre-processor's test branch
as one H2D copy and ONE launch, from decoded pictures to the metric in three lines:

    aug = TestAugment.from_cfg(cfg.tta_pipeline, cfg.model.data_preprocessor, reduce_zero_label=True)
    metric = IoUMetric(label_reduce_zero=aug.reduce_zero_label); metric.dataset_meta = dict(classes=...)
    evaluate(SegTTAModel(model), (aug([img], [seg], [path]) for img, seg, path in pictures), metric)"""
import os

import numpy as np
import torch

from . import ops

CANDIDATES = ops.AUG_CANDIDATES
PARAM_DTYPE, VIEW_PARAM_DTYPE = ops.PARAM_DTYPE, ops.VIEW_PARAM_DTYPE          # include/s2f.h S2fAugParams, S2fViewParams
VARIATES_PER_IMAGE = 2 * CANDIDATES + 11

PHOTOMETRIC_DEFAULTS = dict(brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18)
_PIPELINE_ORDER = ("LoadImageFromFile", "LoadAnnotations", ("RandomResize", "RandomChoiceResize", "ResizeShortestEdge"), "RandomCrop",
                   "RandomFlip", "PhotoMetricDistortion", "PackSegInputs")
_TEST_ORDER = ("LoadImageFromFile", "Resize", "LoadAnnotations", "PackSegInputs")
_TTA_ORDER = ("Resize", "RandomFlip", "LoadAnnotations", "PackSegInputs")


def _rescaled(h0, w0, s):
    """mmcv Resize(scale=s, keep_ratio=True) on an h0 x w0 picture -> (H, W): f = min(max(s) / max(h0, w0), min(s) / min(h0, w0)),
    (int(h0 f + 0.5), int(w0 f + 0.5)) (mmcv.image.geometric.rescale_size) -- the step every resize rule below ends in"""
    f = min(max(s) / max(h0, w0), min(s) / min(h0, w0))
    return int(h0 * f + 0.5), int(w0 * f + 0.5)


def resized_size(h0, w0, scale, ratio):
    """mmcv RandomResize(scale, ratio_range, keep_ratio=True) at the drawn ratio -> (H, W): scale = (int(s0 r), int(s1 r)), then
    the keep-ratio rescale to it (`_rescaled`)"""
    return _rescaled(h0, w0, (int(scale[0] * ratio), int(scale[1] * ratio)))


def scale_factor_size(h0, w0, ratio):
    """mmcv Resize(scale_factor=ratio, keep_ratio=True) -> (H, W): first scale = (int(w0 r + 0.5), int(h0 r + 0.5)) (_scale_size),
    then the keep-ratio rescale TO that size (`_rescaled`).  (512 x 683 at 1.5 -> 768 x 1025: the width is rounded twice.)"""
    return _rescaled(h0, w0, (int(w0 * ratio + 0.5), int(h0 * ratio + 0.5)))


def shortest_edge_scale(h0, w0, scale, max_size):
    """mmseg ResizeShortestEdge._get_output_shape (mmseg/datasets/transforms/transforms.py:1373-1400), operation for operation in
    Python floats -> (new_w, new_h): the short edge to `scale` (an int, or the minimum of a tuple), the long edge in proportion;
    both scaled down once more if the long edge exceeds max_size; each int(v + 0.5).  A square picture takes the second branch."""
    size = float(scale) if isinstance(scale, int) else float(min(scale))
    r = size / min(h0, w0)
    new_h, new_w = (size, r * w0) if h0 < w0 else (r * h0, size)
    if max(new_h, new_w) > max_size:
        r = max_size * 1.0 / max(new_h, new_w)
        new_h *= r
        new_w *= r
    return int(new_w + 0.5), int(new_h + 0.5)


def shortest_edge_size(h0, w0, scale, max_size):
    """mmseg ResizeShortestEdge(scale, max_size) -> (H, W) of the picture after it: `transform` (transforms.py:1402-1404) hands
    `shortest_edge_scale` to a keep-ratio Resize as its scale, so the size is rounded a second time (`_rescaled`).  (256 x 1000 at
    1280 under a cap of 2560 -> 655 x 2559: the long edge ends one short of the cap.)"""
    return _rescaled(h0, w0, shortest_edge_scale(h0, w0, scale, max_size))


def _pick(u, n):
    """a uniform variate u in [0, 1) -> an integer in [0, n)"""
    return min(int(u * n), n - 1)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _checked_scale(s, pairs_only):
    """one entry of RandomChoiceResize's `scales` -> a positive int or a 2-tuple of positive ints (pairs_only: the latter)"""
    if _is_int(s) and s > 0 and not pairs_only:
        return int(s)
    if isinstance(s, (tuple, list)) and len(s) == 2 and all(_is_int(v) and v > 0 for v in s):
        return int(s[0]), int(s[1])
    raise ValueError(f"scales holds {'2-tuples of positive ints' if pairs_only else 'positive ints or 2-tuples of them'}, got {s!r}")


def _default_rank():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank()
    return int(os.environ.get("RANK", "0"))


# ---------------------------------------------------------------------------------------------------- reading a configuration
def _only(cfg, allowed, what, who):
    extra = sorted(set(cfg) - set(allowed) - {"type"})
    if extra:
        raise NotImplementedError(f"{who}: {what} option(s) {extra} are not implemented on the device")


def _in_order(items, order, who):
    """items: (kind, payload) pairs of a pipeline -> the same pairs, each after the check that its kind is one of `order` and
    stands behind its predecessor's.  A slot of `order` is a name, or a tuple of names of which a pipeline holds at most one."""
    slots = [(s,) if isinstance(s, str) else s for s in order]
    place = {kind: i for i, s in enumerate(slots) for kind in s}
    last = None
    for kind, payload in items:
        if kind not in place:
            raise NotImplementedError(f"{who}: transform {kind!r} is not implemented on the device")
        if last is not None and place[kind] <= place[last]:
            raise NotImplementedError(f"{who}: {kind} after {last}: the device applies the transforms in the order "
                                      f"{' -> '.join(' | '.join(s) for s in slots)}")
        last = kind
        yield kind, payload


def _preprocessor(cfg, who):
    """the model's SegDataPreProcessor dictionary -> (mean, std, bgr_to_rgb and pad_val as both classes take them, the checked
    dictionary for what one side reads: `size`, `size_divisor`, `seg_pad_val` the training branch, `test_cfg` the test branch)"""
    p = dict(cfg)
    if p.pop("type", "SegDataPreProcessor") != "SegDataPreProcessor":
        raise NotImplementedError(f"{who}: the data preprocessor is a SegDataPreProcessor")
    _only(p, ("mean", "std", "bgr_to_rgb", "rgb_to_bgr", "pad_val", "seg_pad_val", "size", "test_cfg", "batch_augments",
              "size_divisor"), "SegDataPreProcessor", who)
    if p.get("batch_augments") is not None:
        raise NotImplementedError(f"{who}: SegDataPreProcessor batch_augments are not implemented on the device")
    if p.get("bgr_to_rgb") and p.get("rgb_to_bgr"):
        raise ValueError("`bgr2rgb` and `rgb2bgr` cannot be set to True at the same time")
    return dict(mean=p.get("mean"), std=p.get("std"), bgr_to_rgb=bool(p.get("bgr_to_rgb") or p.get("rgb_to_bgr")),
                pad_val=p.get("pad_val", 0)), p


# ---------------------------------------------------------------------------------------------------- staging
class _Staged:
    """What TrainAugment and TestAugment share: SegDataPreProcessor's constants, the checks of the decoded pictures, and the pinned
    staging buffer with its twin in device memory -- the parameter table first (its room is a multiple of 16 bytes: the packed
    bytes behind it start aligned), then batch_size pictures of max_source_pixels pixels with their annotations (4 bytes per
    pixel) -- filled and sent by ONE host-to-device copy (`_copy_in`)."""
    __test__ = False          # (pytest: a class named Test* imported into a test module is not a test)

    def __init__(self, entry_dtype, entries_per_picture, mean, std, bgr_to_rgb, pad_val, batch_size, max_source_pixels, device):
        self.mean, self.std = (None, None) if mean is None and std is None else ops._mean_std(mean, std)
        self.bgr_to_rgb, self.pad_val = bool(bgr_to_rgb), float(pad_val)
        self.batch_size, self.max_source_pixels = int(batch_size), int(max_source_pixels)
        if self.batch_size <= 0 or self.max_source_pixels <= 0:
            raise ValueError("batch_size and max_source_pixels are positive")
        self.device = torch.device(device)
        self._table_cap = (entries_per_picture * self.batch_size * entry_dtype.itemsize + 15) // 16 * 16
        self._data_cap = self.batch_size * self.max_source_pixels * 4
        self._pin = self._dev = self._copied = None

    def _allocate(self):
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs on the GPU only (HIP kernels): there is no host route")
        n = self._table_cap + self._data_cap
        self._pin = torch.empty(n, dtype=torch.uint8).pin_memory()
        self._dev = torch.zeros(n, dtype=torch.uint8, device=self.device)
        self._copied = torch.cuda.Event()

    def _pictures(self, images, segs, one_size=False):
        """-> (images, segs) as contiguous numpy arrays: 1 .. batch_size uint8 [h0, w0, 3] pictures of at most max_source_pixels
        pixels (one_size: all of the first one's size), and for each, unless segs is None, a uint8 [h0, w0] annotation"""
        B = len(images)
        if not 0 < B <= self.batch_size or (segs is not None and len(segs) != B):
            raise ValueError(f"{B} pictures, {'no' if segs is None else len(segs)} annotations for a batch size of {self.batch_size}")
        images = [np.ascontiguousarray(np.asarray(i)) for i in images]
        segs = None if segs is None else [np.ascontiguousarray(np.asarray(s)) for s in segs]
        for k, i in enumerate(images):
            if i.dtype != np.uint8 or i.ndim != 3 or i.shape[2] != 3 or (one_size and i.shape != images[0].shape):
                raise ValueError("pictures are uint8 [h0, w0, 3]" + (" of ONE size (the reference's test branch asserts equal sizes)"
                                                                     if one_size else ""))
            if segs is not None and (segs[k].dtype != np.uint8 or segs[k].shape != i.shape[:2]):
                raise ValueError("annotations are uint8 [h0, w0] of their picture's size")
            h0, w0 = i.shape[:2]
            if h0 * w0 > self.max_source_pixels or h0 * w0 == 0:
                raise ValueError(f"a {h0} x {w0} picture does not fit max_source_pixels = {self.max_source_pixels}")
        return images, segs

    def _copy_in(self, table, pieces):
        """The table and the pieces [(byte offset behind the table's room, array)] into the pinned buffer, then ONE host-to-device
        copy of what they span, queued on the current stream."""
        if self._pin is None:
            self._allocate()
        self._copied.synchronize()          # the previous copy has left the staging buffer (a copy, not the step, is waited for)
        pin = self._pin.numpy()
        pin[:table.nbytes] = table.view(np.uint8)
        n = d0 = self._table_cap
        for off, a in pieces:
            pin[d0 + off:d0 + off + a.size] = a.reshape(-1)
            n = max(n, d0 + off + a.size)
        self._dev[:n].copy_(self._pin[:n], non_blocking=True)
        self._copied.record()


class TrainAugment(_Staged):
    def __init__(self, scale=(2048, 512), ratio_range=(0.5, 2.0), crop_size=(512, 512), cat_max_ratio=0.75, flip_prob=0.5,
                 photometric=True, reduce_zero_label=False, ignore_index=255, mean=None, std=None, bgr_to_rgb=False, pad_val=0,
                 seg_pad_val=255, batch_size=2, max_source_pixels=2048 * 1024, device="cuda", seed=0, rank=None, scales=None,
                 resize_type="ResizeShortestEdge", max_size=None):
        """scale / ratio_range: RandomResize's (scale None: no resize; ratio_range None: ratio 1); scales / resize_type / max_size:
        RandomChoiceResize's, INSTEAD of scale (say scale=None): one of `scales` per picture, uniformly -- short-edge lengths (ints,
        or tuples whose minimum counts) under the cap max_size on the long edge for resize_type "ResizeShortestEdge", (long, short)
        tuples for the keep-ratio "Resize"; crop_size (h, w), cat_max_ratio, ignore_index: RandomCrop's; flip_prob: RandomFlip's
        (horizontal); photometric: True (PhotoMetricDistortion's defaults), a dictionary of its arguments, or None / False;
        reduce_zero_label: LoadAnnotations'; mean, std, bgr_to_rgb, pad_val, seg_pad_val: SegDataPreProcessor's (its `size` is
        crop_size).  batch_size images of at most max_source_pixels pixels each fit the staging buffers (4 bytes per pixel: the
        picture and its annotation).  rank: the data-parallel rank the generator is seeded with next to `seed` (default: the
        process group's, else $RANK, else 0)."""
        self.scales, self.resize_type, self.max_size = None, None, None
        if scales is not None:
            if scale is not None:
                raise ValueError("one resize rule: scale (RandomResize) or scales (RandomChoiceResize), not both; with scales, "
                                 "say scale=None")
            if resize_type not in ("ResizeShortestEdge", "Resize"):
                raise ValueError(f"resize_type {resize_type!r}: 'ResizeShortestEdge' or 'Resize'")
            pairs_only = resize_type == "Resize"
            self.scales = tuple(_checked_scale(s, pairs_only) for s in scales)
            if not self.scales:
                raise ValueError("scales is a non-empty list")
            self.resize_type = resize_type
            if pairs_only and max_size is not None:
                raise ValueError("max_size is ResizeShortestEdge's: resize_type 'Resize' takes none")
            if not pairs_only:
                if not _is_int(max_size) or max_size <= 0:
                    raise ValueError(f"resize_type 'ResizeShortestEdge' needs a positive int max_size, got {max_size!r}")
                self.max_size = int(max_size)
        self.scale = None if scale is None else (int(scale[0]), int(scale[1]))
        self.ratio_range = None if ratio_range is None else (float(ratio_range[0]), float(ratio_range[1]))
        self.crop_size = (int(crop_size), int(crop_size)) if isinstance(crop_size, int) else (int(crop_size[0]), int(crop_size[1]))
        if not (0 < self.crop_size[0] <= ops.AUG_MAX_CROP and 0 < self.crop_size[1] <= ops.AUG_MAX_CROP):
            raise ValueError(f"crop_size {self.crop_size} outside 1 .. {ops.AUG_MAX_CROP}")
        self.cat_max_ratio, self.flip_prob = float(cat_max_ratio), float(flip_prob or 0.0)
        if photometric is True:
            photometric = {}
        self.photometric = None if photometric in (None, False) else {**PHOTOMETRIC_DEFAULTS, **photometric}
        if self.photometric is not None:
            _only(self.photometric, PHOTOMETRIC_DEFAULTS, "PhotoMetricDistortion", "TrainAugment")
        self.reduce_zero_label, self.ignore_index, self.seg_pad_val = bool(reduce_zero_label), int(ignore_index), int(seg_pad_val)
        super().__init__(PARAM_DTYPE, 1, mean, std, bgr_to_rgb, pad_val, batch_size, max_source_pixels, device)
        self.seed, self.rank = int(seed), int(_default_rank() if rank is None else rank)
        self.rng = np.random.default_rng(np.random.SeedSequence([self.seed, self.rank]))
        self._flags = self._inputs = self._seg = None
        self._staged = 0

    # ------------------------------------------------------------------------------------------------ configuration
    @classmethod
    def from_cfg(cls, train_pipeline, data_preprocessor, **kwargs):
        """train_pipeline: the list of transform dictionaries of an mmseg config (LoadImageFromFile, LoadAnnotations, a resize,
        RandomCrop, RandomFlip, PhotoMetricDistortion, PackSegInputs, in this order; LoadImageFromFile only marks where the caller's
        decoded pictures enter); data_preprocessor: the model's SegDataPreProcessor dictionary.  The resize is at most one of
        RandomResize(scale, ratio_range, keep_ratio=True) (the _base_ data sets' pipeline: the VOC and FPN configs),
        RandomChoiceResize(scales, resize_type, max_size | keep_ratio=True) (with resize_type='ResizeShortestEdge': the ADE20K,
        Cityscapes and COCO-Stuff MaskFormer configs' own pipeline) and a stand-alone ResizeShortestEdge(scale, max_size).  Any other
        transform, order or option raises NotImplementedError.  kwargs: batch_size, max_source_pixels, device, seed, rank."""
        who = "TrainAugment"
        a = dict(scale=None, ratio_range=None, cat_max_ratio=1.0, flip_prob=0.0, photometric=None)
        for kind, t in _in_order(((t.get("type"), t) for t in train_pipeline), _PIPELINE_ORDER, who):
            if kind in ("LoadImageFromFile", "PackSegInputs"):
                _only(t, (), kind, who)
            elif kind == "LoadAnnotations":
                _only(t, ("reduce_zero_label",), kind, who)
                a["reduce_zero_label"] = bool(t.get("reduce_zero_label", False))
            elif kind == "RandomResize":
                _only(t, ("scale", "ratio_range", "keep_ratio"), kind, who)
                if not t.get("keep_ratio", False) or not isinstance(t.get("scale"), (tuple, list)) or len(t["scale"]) != 2 \
                        or not all(isinstance(v, int) for v in t["scale"]):
                    raise NotImplementedError("TrainAugment: RandomResize needs keep_ratio=True and one (long, short) scale")
                a["scale"], a["ratio_range"] = tuple(t["scale"]), t.get("ratio_range")
            elif kind == "RandomChoiceResize":          # (mmcv: every option but `scales` goes to the transform `resize_type` names)
                _only(t, ("scales", "resize_type", "max_size", "keep_ratio"), kind, who)
                rtype = t.get("resize_type", "Resize")
                if rtype not in ("Resize", "ResizeShortestEdge"):
                    raise NotImplementedError(f"TrainAugment: RandomChoiceResize resize_type={rtype!r} is not implemented on the "
                                              f"device")
                if not t.get("scales"):
                    raise NotImplementedError("TrainAugment: RandomChoiceResize needs scales")
                if rtype == "Resize" and (not t.get("keep_ratio", False) or "max_size" in t):
                    raise NotImplementedError("TrainAugment: RandomChoiceResize with resize_type='Resize' needs keep_ratio=True "
                                              "and takes no max_size")
                if rtype == "ResizeShortestEdge" and ("keep_ratio" in t or "max_size" not in t):
                    raise NotImplementedError("TrainAugment: RandomChoiceResize with resize_type='ResizeShortestEdge' needs "
                                              "max_size and takes no keep_ratio")
                a.update(scales=list(t["scales"]), resize_type=rtype, max_size=t.get("max_size"))
            elif kind == "ResizeShortestEdge":
                _only(t, ("scale", "max_size"), kind, who)
                if "scale" not in t or "max_size" not in t:
                    raise NotImplementedError("TrainAugment: ResizeShortestEdge needs scale and max_size")
                a.update(scales=[t["scale"]], resize_type=kind, max_size=t["max_size"])
            elif kind == "RandomCrop":
                _only(t, ("crop_size", "cat_max_ratio", "ignore_index"), kind, who)
                a["crop_size"] = t["crop_size"]
                a["cat_max_ratio"], a["ignore_index"] = t.get("cat_max_ratio", 1.0), t.get("ignore_index", 255)
            elif kind == "RandomFlip":
                _only(t, ("prob", "direction"), kind, who)
                if t.get("direction", "horizontal") != "horizontal" or isinstance(t.get("prob"), (list, tuple)):
                    raise NotImplementedError("TrainAugment: RandomFlip is implemented for one probability, horizontal")
                a["flip_prob"] = t.get("prob") or 0.0
            elif kind == "PhotoMetricDistortion":
                _only(t, PHOTOMETRIC_DEFAULTS, kind, who)
                a["photometric"] = {k: v for k, v in t.items() if k != "type"}
        if "crop_size" not in a:
            raise NotImplementedError("TrainAugment: a train_pipeline without RandomCrop has no fixed output size")
        common, p = _preprocessor(data_preprocessor, who)
        if p.get("size_divisor") is not None:
            raise NotImplementedError("TrainAugment: SegDataPreProcessor size_divisor is not implemented on the device")
        crop = a["crop_size"]
        crop = (crop, crop) if isinstance(crop, int) else tuple(crop)
        if p.get("size") is not None and tuple(p["size"]) != crop:
            raise NotImplementedError(f"TrainAugment: SegDataPreProcessor size {tuple(p['size'])} is not the crop size {crop}")
        return cls(**a, **common, seg_pad_val=p.get("seg_pad_val", 255), **kwargs)

    # ------------------------------------------------------------------------------------------------ random numbers
    def draw(self, shapes):
        """shapes: [(h0, w0)] of the batch's pictures -> their parameter table, a numpy array of PARAM_DTYPE (the offsets are filled
        in by `stage`).  VARIATES_PER_IMAGE uniform variates per image, whatever the configuration uses of them."""
        params = np.zeros(len(shapes), PARAM_DTYPE)
        Hc, Wc = self.crop_size
        ph = self.photometric
        for p, (h0, w0) in zip(params, shapes):
            u = self.rng.random(VARIATES_PER_IMAGE)
            h0, w0 = int(h0), int(w0)
            if self.scales is not None:          # RandomChoiceResize._random_select: numpy.random.randint(len(scales))
                s = self.scales[_pick(u[0], len(self.scales))]
                H, W = resized_size(h0, w0, s, 1.0) if self.resize_type == "Resize" else shortest_edge_size(h0, w0, s, self.max_size)
            elif self.scale is None:
                H, W = h0, w0
            else:
                lo, hi = self.ratio_range or (1.0, 1.0)
                H, W = resized_size(h0, w0, self.scale, u[0] * (hi - lo) + lo)          # RandomResize._random_scale
            p["h0"], p["w0"], p["H"], p["W"] = h0, w0, H, W
            my, mx = max(H - Hc, 0), max(W - Wc, 0)
            for c in range(CANDIDATES):          # generate_crop_bbox: randint(0, margin + 1) for the row, then for the column
                p["crop_y"][c], p["crop_x"][c] = _pick(u[1 + 2 * c], my + 1), _pick(u[2 + 2 * c], mx + 1)
            v = u[1 + 2 * CANDIDATES:]
            p["flip"] = int(v[0] < self.flip_prob)
            if ph is not None:          # random.randint(2) switches, uniform values; hue: randint(-delta, delta), upper end open
                p["bright_on"], p["bright_beta"] = _pick(v[1], 2), (2 * v[2] - 1) * ph["brightness_delta"]
                p["mode"] = _pick(v[3], 2)
                lo, hi = ph["contrast_range"]
                p["contrast_on"], p["contrast_alpha"] = _pick(v[4], 2), lo + v[5] * (hi - lo)
                lo, hi = ph["saturation_range"]
                p["sat_on"], p["sat_alpha"] = _pick(v[6], 2), lo + v[7] * (hi - lo)
                d = int(ph["hue_delta"])
                p["hue_on"], p["hue_delta"] = _pick(v[8], 2), (-d + _pick(v[9], 2 * d)) if d > 0 else 0
        return params

    # ------------------------------------------------------------------------------------------------ device side
    def _allocate(self):
        super()._allocate()
        self._flags = torch.zeros(self.batch_size, CANDIDATES, dtype=torch.int32, device=self.device)

    def stage(self, images, segs, params=None):
        """Packs the pictures, the annotations and the table into the pinned staging buffer and queues ONE host-to-device copy on the
        current stream.  images: uint8 [h0, w0, 3] BGR arrays (numpy or CPU tensors); segs: uint8 [h0, w0].  -> params as staged."""
        images, segs = self._pictures(images, segs)
        B = len(images)
        params = self.draw([i.shape[:2] for i in images]) if params is None else np.array(params, dtype=PARAM_DTYPE)
        if params.shape != (B,):
            raise ValueError(f"{params.shape} parameter entries for {B} pictures")
        Hc, Wc = self.crop_size
        off, pieces = 0, []
        for i, s, p in zip(images, segs, params):
            h0, w0 = s.shape
            if (p["h0"], p["w0"]) != (h0, w0) or p["H"] <= 0 or p["W"] <= 0:
                raise ValueError(f"parameter entry for a {p['h0']} x {p['w0']} picture resized to {p['H']} x {p['W']}, picture {h0} x {w0}")
            my, mx = max(int(p["H"]) - Hc, 0), max(int(p["W"]) - Wc, 0)
            if p["crop_y"].min() < 0 or p["crop_y"].max() > my or p["crop_x"].min() < 0 or p["crop_x"].max() > mx:
                raise ValueError("a candidate crop origin lies outside [0, margin]")
            p["img_off"], p["seg_off"] = off, off + 3 * h0 * w0
            pieces += [(off, i), (off + 3 * h0 * w0, s)]
            off += 4 * h0 * w0
        self._copy_in(params, pieces)
        self._staged = B
        return params

    def launch(self, out=None, batch=None):
        """The two launches on the current stream (one when cat_max_ratio >= 1) over what `stage` last copied; capturable in a
        hipGraph (the table and the pixels are read from their static device buffers at replay time).  out = (inputs [B, 3, Hc, Wc]
        fp32, seg [B, Hc, Wc] uint8) is written in place -- e.g. a step's (static_in, static_seg); None: persistent buffers of this
        object.  -> (inputs, seg)."""
        B = int(batch or self._staged)
        if not 0 < B <= self.batch_size or self._dev is None:
            raise RuntimeError("TrainAugment.launch before stage")
        if out is None:
            if self._inputs is None:
                self._inputs = torch.empty(self.batch_size, 3, *self.crop_size, dtype=torch.float32, device=self.device)
                self._seg = torch.empty(self.batch_size, *self.crop_size, dtype=torch.uint8, device=self.device)
            out = (self._inputs[:B], self._seg[:B])
        inputs, seg = out
        if tuple(inputs.shape) != (B, 3, *self.crop_size) or tuple(seg.shape) != (B, *self.crop_size):
            raise ValueError(f"out is {tuple(inputs.shape)} / {tuple(seg.shape)} for {B} pictures cropped to {self.crop_size}")
        table, data = self._dev[:B * PARAM_DTYPE.itemsize], self._dev[self._table_cap:]
        flags = None
        if self.cat_max_ratio < 1.0:
            flags = ops.aug_crop_stats(data, table, self._flags[:B], self.crop_size, self.ignore_index, self.reduce_zero_label,
                                       self.cat_max_ratio)
        return ops.aug_apply(data, table, flags, inputs, seg, self.mean, self.std, self.bgr_to_rgb, self.pad_val, self.seg_pad_val,
                             self.reduce_zero_label)

    def __call__(self, images, segs, params=None, out=None):
        self.stage(images, segs, params)
        return self.launch(out)


# ---------------------------------------------------------------------------------------------------- the test pipeline
def _resize_args(t, what):
    _only(t, ("scale", "scale_factor", "keep_ratio"), what, "TestAugment")
    if not t.get("keep_ratio", False):
        raise NotImplementedError(f"TestAugment: {what} with keep_ratio=False is not implemented on the device")
    if ("scale" in t) == ("scale_factor" in t):
        raise NotImplementedError(f"TestAugment: {what} takes one of scale=(long, short) and scale_factor=r")
    if "scale" in t:
        s = t["scale"]
        if not isinstance(s, (tuple, list)) or len(s) != 2 or not all(isinstance(v, int) for v in s):
            raise NotImplementedError(f"TestAugment: {what} needs one (long, short) scale, got {s!r}")
        return tuple(s), None
    r = t["scale_factor"]
    if isinstance(r, (tuple, list)) or not r > 0:
        raise NotImplementedError(f"TestAugment: {what} needs one positive scale_factor, got {r!r}")
    return None, float(r)


class TestAugment(_Staged):
    """The shipped configs' `test_pipeline` / `tta_pipeline` -- Resize(keep_ratio=True) [x RandomFlip(prob 0 | 1)] -- and the test
    branch of `SegDataPreProcessor` (channel swap, (x - mean) / std, padding by test_cfg's size / size_divisor) as ONE H2D copy and
    ONE HIP launch (s2f_test_views, csrc/augment.hip) from the decoded uint8 pictures of an iteration to every view of it: the
    test-time counterpart of `TrainAugment`, with the bilinear arithmetic the training pictures were resized by (the kernel shares
    the sampling code with s2f_aug_apply).  File loading is not here: the caller hands in decoded BGR pictures.

        aug = TestAugment.from_cfg(cfg.tta_pipeline, cfg.model.data_preprocessor, reduce_zero_label=True)
        metric = IoUMetric(label_reduce_zero=aug.reduce_zero_label); metric.dataset_meta = dict(classes=...)
        evaluate(SegTTAModel(model), (aug([img], [seg], [path]) for img, seg, path in pictures), metric)

    (`cfg.test_pipeline` and the plain model alike.)  The annotations are NOT transformed: as in the reference, where LoadAnnotations
    comes after the resize and the flips, `gt_sem_seg` is the raw map at the picture's own size, and the label reduction is the
    metric's (`IoUMetric(label_reduce_zero=aug.reduce_zero_label)`).

    The sizes follow mmcv 2.x (Resize.transform, _scale_size, rescale_size: `view_sizes`) and mmseg's stack_batch; mmcv is not
    available to this project, the rule is restated from its source.  The resize itself is OpenCV's in the reference; here it is
    the fp32 bilinear kernel of the training path (the distance between the two has not been measured).

    What a call returns -- the views and the annotations -- lives in persistent device buffers of this object and is valid until
    the next call."""

    def __init__(self, scale=(2048, 512), scale_factors=None, flips=(False,), reduce_zero_label=False, mean=None, std=None,
                 bgr_to_rgb=False, pad_val=0, size=None, size_divisor=None, batch_size=1, max_source_pixels=2048 * 1024, device="cuda",
                 tta=None):
        """scale: Resize's (long, short), or None; scale_factors: the ratios of TestTimeAug's Resize(scale_factor=r) list, or None
        (at most one of the two; neither: no resize); flips: the horizontal flips of every size, in order; reduce_zero_label:
        LoadAnnotations' (recorded in the metainfo and for the metric: the kernel does not touch annotations); mean, std,
        bgr_to_rgb, pad_val: SegDataPreProcessor's; size (h, w) / size_divisor: its test_cfg's (at most one).  batch_size pictures of
        at most max_source_pixels pixels fit the staging buffers (4 bytes per pixel: the picture and its annotation).  tta: whether a
        call returns the dict-of-per-view-lists SegTTAModel takes or the one batch a model's test_step takes (one view only);
        default: the TTA form iff scale_factors or more than one flip is given."""
        if scale is not None and scale_factors is not None:
            raise ValueError("one Resize: scale or scale_factors, not both")
        self.scale = None if scale is None else (int(scale[0]), int(scale[1]))
        self.scale_factors = None if scale_factors is None else tuple(float(r) for r in scale_factors)
        self.flips = tuple(bool(f) for f in flips)
        if not self.flips or (self.scale_factors is not None and not self.scale_factors):
            raise ValueError("at least one view")
        self.tta = bool(self.scale_factors is not None or len(self.flips) > 1) if tta is None else bool(tta)
        self.n_views = len(self.scale_factors or (None,)) * len(self.flips)
        if not self.tta and self.n_views != 1:
            raise ValueError(f"{self.n_views} views need the TTA form")
        self.reduce_zero_label = bool(reduce_zero_label)
        if size is not None and size_divisor is not None:
            raise ValueError("only one of size and size_divisor should be valid")
        self.size = None if size is None else (int(size[0]), int(size[1]))
        self.size_divisor = None if size_divisor is None else int(size_divisor)
        super().__init__(VIEW_PARAM_DTYPE, self.n_views, mean, std, bgr_to_rgb, pad_val, batch_size, max_source_pixels, device)
        self._out = self._staged = None

    # ------------------------------------------------------------------------------------------------ configuration
    @classmethod
    def from_cfg(cls, pipeline, data_preprocessor, reduce_zero_label=False, **kwargs):
        """pipeline: an mmseg config's `test_pipeline` (LoadImageFromFile, Resize(scale=(long, short), keep_ratio=True),
        LoadAnnotations, PackSegInputs) or `tta_pipeline` (LoadImageFromFile, TestTimeAug(transforms=[[Resize(scale_factor=r,
        keep_ratio=True) ...], [RandomFlip(prob=0. | 1., direction='horizontal') ...], [LoadAnnotations], [PackSegInputs]]): the
        views are ordered as itertools.product orders them, ratio slowest, flip fastest); data_preprocessor: the model's
        SegDataPreProcessor dictionary (mean, std, bgr_to_rgb, pad_val and test_cfg's size / size_divisor are used).  Any other
        transform, order or option raises NotImplementedError.  reduce_zero_label: what a LoadAnnotations without the option takes
        (in mmseg: the data set's).  kwargs: batch_size, max_source_pixels, device."""
        who = "TestAugment"
        kinds = [t.get("type") for t in pipeline]
        a = dict(scale=None, scale_factors=None, flips=(False,), reduce_zero_label=bool(reduce_zero_label), tta="TestTimeAug" in kinds)

        def annotations(t):
            _only(t, ("reduce_zero_label",), "LoadAnnotations", who)
            a["reduce_zero_label"] = bool(t.get("reduce_zero_label", reduce_zero_label))

        def group_kind(group):
            names = sorted({t.get("type") for t in group})
            if len(names) != 1:
                raise NotImplementedError(f"TestAugment: one kind of transform per TestTimeAug list, got {names}")
            return names[0]

        if a["tta"]:
            if kinds != ["LoadImageFromFile", "TestTimeAug"]:
                raise NotImplementedError(f"TestAugment: a tta_pipeline is LoadImageFromFile, TestTimeAug; got {kinds}")
            _only(pipeline[0], (), "LoadImageFromFile", who)
            _only(pipeline[1], ("transforms",), "TestTimeAug", who)
            groups = [[g] if isinstance(g, dict) else list(g) for g in pipeline[1]["transforms"]]
            kind = None
            for kind, group in _in_order(((group_kind(g), g) for g in groups), _TTA_ORDER, who):
                if kind == "Resize":
                    args = [_resize_args(t, "Resize") for t in group]
                    if any(s is not None for s, _ in args):
                        raise NotImplementedError("TestAugment: TestTimeAug's Resize list takes scale_factor=r entries")
                    a["scale_factors"] = tuple(r for _, r in args)
                elif kind == "RandomFlip":
                    flips = []
                    for t in group:
                        _only(t, ("prob", "direction"), "RandomFlip", who)
                        if t.get("direction", "horizontal") != "horizontal":
                            raise NotImplementedError(f"TestAugment: RandomFlip direction={t['direction']!r}: only 'horizontal' is "
                                                      f"implemented on the device")
                        prob = t.get("prob")
                        if isinstance(prob, (list, tuple)) or prob is None or float(prob) not in (0.0, 1.0):
                            raise NotImplementedError(f"TestAugment: RandomFlip prob={prob!r}: a test-time flip is certain (prob 0 or 1)")
                        flips.append(float(prob) == 1.0)
                    a["flips"] = tuple(flips)
                elif len(group) != 1:
                    raise NotImplementedError(f"TestAugment: one {kind}")
                elif kind == "LoadAnnotations":
                    annotations(group[0])
                else:
                    _only(group[0], (), "PackSegInputs", who)
            if kind != "PackSegInputs":
                raise NotImplementedError("TestAugment: TestTimeAug's transforms end in [PackSegInputs]")
        else:
            for kind, t in _in_order(zip(kinds, pipeline), _TEST_ORDER, who):
                if kind in ("LoadImageFromFile", "PackSegInputs"):
                    _only(t, (), kind, who)
                elif kind == "LoadAnnotations":
                    annotations(t)
                else:
                    scale, ratio = _resize_args(t, "Resize")
                    a["scale"], a["scale_factors"] = scale, None if ratio is None else (ratio,)
        common, p = _preprocessor(data_preprocessor, who)
        test_cfg = dict(p.get("test_cfg") or {})          # (size / size_divisor OUTSIDE test_cfg are the training branch's)
        _only(test_cfg, ("size", "size_divisor"), "SegDataPreProcessor test_cfg", who)
        return cls(**a, **common, size=test_cfg.get("size"), size_divisor=test_cfg.get("size_divisor"), **kwargs)

    # ------------------------------------------------------------------------------------------------ geometry
    def padded_size(self, H, W):
        """mmseg stack_batch on pictures of one size: `size`: max(size - dim, 0) of padding; `size_divisor`: rounded up; else none"""
        if self.size is not None:
            return H + max(self.size[0] - H, 0), W + max(self.size[1] - W, 0)
        if self.size_divisor is not None and self.size_divisor > 1:
            d = self.size_divisor
            return (H + d - 1) // d * d, (W + d - 1) // d * d
        return H, W

    def view_sizes(self, h0, w0):
        """-> [(H, W, Hp, Wp, flip)] of the views of an h0 x w0 picture, in view order (ratio slowest, flip fastest).  Pure host
        arithmetic, restated from mmcv 2.x: Resize(scale) is `resized_size(h0, w0, scale, 1.0)`, Resize(scale_factor=r) is
        `scale_factor_size` (both mmcv.image.geometric.rescale_size on a size from _scale_size); the padding is stack_batch's."""
        h0, w0 = int(h0), int(w0)
        views = []
        for r in self.scale_factors or (None,):
            if r is not None:
                H, W = scale_factor_size(h0, w0, r)
            elif self.scale is not None:
                H, W = resized_size(h0, w0, self.scale, 1.0)
            else:
                H, W = h0, w0
            views += [(H, W, *self.padded_size(H, W), f) for f in self.flips]
        return views

    def table(self, h0, w0, B=1, views=None):
        """-> (the V * B table entries of VIEW_PARAM_DTYPE in (view, image) order, the elements of `out` they span).  Picture b lies
        at byte 3 h0 w0 b of data; the blocks are packed in entry order, each starting at a multiple of 4 elements (16 bytes)."""
        views = self.view_sizes(h0, w0) if views is None else [tuple(int(x) for x in v[:4]) + (bool(v[4]),) for v in views]
        t = np.zeros(len(views) * B, VIEW_PARAM_DTYPE)
        off = 0
        for v, (H, W, Hp, Wp, flip) in enumerate(views):
            for b in range(B):
                p = t[v * B + b]
                p["img_off"], p["out_off"] = 3 * h0 * w0 * b, off
                p["h0"], p["w0"], p["H"], p["W"], p["Hp"], p["Wp"], p["flip"] = h0, w0, H, W, Hp, Wp, int(flip)
                off = (off + 3 * Hp * Wp + 3) // 4 * 4
        return t, off

    # ------------------------------------------------------------------------------------------------ device side
    def stage(self, images, segs=None, img_paths=None, views=None):
        """Packs the table, the pictures and (if given) the raw annotations into the pinned staging buffer and queues ONE
        host-to-device copy on the current stream; grows the packed output buffer if this iteration's views need more than any
        before.  images: B <= batch_size uint8 [h0, w0, 3] BGR arrays of ONE size (numpy or CPU tensors); segs: uint8 [h0, w0];
        views: [(H, W, Hp, Wp, flip)] instead of `view_sizes` (any sizes: what the tests of the kernel use).  -> the table."""
        images, segs = self._pictures(images, segs, one_size=True)
        B = len(images)
        if img_paths is not None and len(img_paths) != B:
            raise ValueError(f"{len(img_paths)} paths for {B} pictures")
        h0, w0 = images[0].shape[:2]
        if views is not None and len(views) > self.n_views:
            raise ValueError(f"{len(views)} views, the staging buffer holds the table of {self.n_views}")
        table, out_elems = self.table(h0, w0, B, views)
        n_img = 3 * h0 * w0 * B
        ops.check_view_table(table, n_img, out_elems)
        self._copy_in(table, [(3 * h0 * w0 * b, i) for b, i in enumerate(images)]
                      + [(n_img + h0 * w0 * b, s) for b, s in enumerate(segs or ())])
        if self._out is None or self._out.numel() < out_elems:          # a new high-water mark (not inside a graph capture)
            self._out = torch.empty(out_elems, dtype=torch.float32, device=self.device)
        self._staged = dict(table=table, B=B, shape=(h0, w0), n_img=n_img, segs=segs is not None, out_elems=out_elems,
                            paths=list(img_paths) if img_paths is not None else [None] * B, tta=self.tta or views is not None)
        return table

    def launch(self):
        """The ONE launch on the current stream over what `stage` last copied (capturable in a hipGraph: the table and the pixels
        are read from their static device buffers at replay time), and the data the consumers take.  One batch (`tta` False):
        dict(inputs=[B, 3, Hp, Wp], data_samples=[SegDataSample] * B, preprocessed=True); the TTA form: the same three keys, each a
        list with one item per view -- what SegTTAModel.split_views splits.  `preprocessed` makes EncoderDecoder.preprocess pass
        the batch through.  The tensors are views of this object's buffers: valid until the next call.  (B > 1 with 3 Hp Wp no
        multiple of 4 -- odd sizes without a test_cfg: the blocks of a view cannot be both adjacent and 16-byte aligned; the view
        is then a tensor whose batch stride is rounded up to 4 elements, not a contiguous one.)"""
        from .data_preprocessor import PixelData, SegDataSample
        st = self._staged
        if st is None or self._dev is None:
            raise RuntimeError("TestAugment.launch before stage")
        table, B, (h0, w0) = st["table"], st["B"], st["shape"]
        d0 = self._table_cap
        ops.test_views(self._dev[d0:d0 + st["n_img"]], table, self._out[:st["out_elems"]], self.mean, self.std, self.bgr_to_rgb,
                       self.pad_val, table_dev=self._dev[:table.nbytes])
        gts = None
        if st["segs"]:
            gts = self._dev[d0 + st["n_img"]:d0 + st["n_img"] + h0 * w0 * B].view(B, 1, h0, w0)
        inputs, samples = [], []
        for v in range(len(table) // B):
            p = table[v * B]
            H, W, Hp, Wp, flip = int(p["H"]), int(p["W"]), int(p["Hp"]), int(p["Wp"]), bool(p["flip"])
            stride = int(table[v * B + 1]["out_off"] - p["out_off"]) if B > 1 else 3 * Hp * Wp
            inputs.append(self._out.as_strided((B, 3, Hp, Wp), (stride, Hp * Wp, Wp, 1), int(p["out_off"])))
            meta = dict(ori_shape=(h0, w0), img_shape=(H, W), pad_shape=(Hp, Wp), scale_factor=(W / w0, H / h0), flip=flip,
                        flip_direction="horizontal" if flip else None, reduce_zero_label=self.reduce_zero_label)
            if self.size is not None or self.size_divisor is not None:
                meta["img_padding_size"] = (0, Wp - W, 0, Hp - H)
            samples.append([SegDataSample(gt_sem_seg=None if gts is None else PixelData(gts[b]),
                                          metainfo=dict(meta, img_path=st["paths"][b])) for b in range(B)])
        if st["tta"]:
            return dict(inputs=inputs, data_samples=samples, preprocessed=[True] * len(inputs))
        return dict(inputs=inputs[0], data_samples=samples[0], preprocessed=True)

    def sources(self):
        """-> the pictures `stage` last copied as they lie in device memory: a uint8 [B, h0, w0, 3] BGR view of the staging twin
        (`is_bgr` is True on it), valid until the next `stage` -- what a SegVisualizationHook(source=aug) draws into."""
        st = self._staged
        if st is None or self._dev is None:
            raise RuntimeError("TestAugment.sources before stage")
        d0, (h0, w0) = self._table_cap, st["shape"]
        pictures = self._dev[d0:d0 + st["n_img"]].view(st["B"], h0, w0, 3)
        pictures.is_bgr = True
        return pictures

    def __call__(self, images, segs=None, img_paths=None, views=None):
        self.stage(images, segs, img_paths, views)
        return self.launch()
