"""`IoUMetric` (mmseg/evaluation/metrics/iou_metric.py:18-291 on mmengine's BaseMetric) and the evaluation loop around it
(mmengine TestLoop / ValLoop with ResetModelHook.before_test_iter) -- the `val_evaluator = dict(type='IoUMetric', ...)` every shipped
config ends in.

Per image ONE `ops.seg_hist` launch adds the class histograms {intersection, prediction areas, label areas} into an int64 [3, K]
accumulator on the prediction's device; nothing leaves the device until `evaluate()` reads the accumulator back once.  Stated
deviations: the totals are summed as int64, not as float32 tensors (exact beyond 2^24 pixels per class), and
the ranks' totals are all-reduced instead of gathering per-image results -- a sum cannot drop the samples a padding
DistributedSampler duplicates, so `evaluate` below shards the batches without padding.

`ConfusionMatrix` keeps the full class-pair table [K, K] of the same pixels in the same way (one `ops.seg_confusion` launch per
image); IoUMetric's three rows are its diagonal, column sums and row sums."""
import logging
import os.path as osp
from collections import OrderedDict

import numpy as np
import torch

from . import ops
from .neuron import reset_net
from .registry import METRICS

_ALLOWED = ("mIoU", "mDice", "mFscore")


def _field(sample, name):
    """`sample.<name>.data` of a SegDataSample-like object or `sample[name]['data']` of an mmengine-style dict"""
    v = sample[name] if isinstance(sample, dict) else getattr(sample, name)
    return v["data"] if isinstance(v, dict) else v.data


def _meta(sample, key, default=None):
    if isinstance(sample, dict):
        return sample.get(key, default)
    return getattr(sample, "metainfo", {}).get(key, default)


def _nanmean(values):
    """np.nanmean without its warning on an empty / all-NaN input (NaN there, as the reference)"""
    a = np.asarray(values, dtype=np.float64).reshape(-1)
    a = a[~np.isnan(a)]
    return float(a.mean()) if a.size else float("nan")


@METRICS.register_module()
class IoUMetric:
    """ignore_index / iou_metrics ('mIoU', 'mDice', 'mFscore') / nan_to_num / beta / output_dir / format_only / prefix as the
    reference; `collect_device` is accepted and unused (the totals are all-reduced where they live).  `dataset_meta['classes']`
    gives the number of classes.  `label_reduce_zero=True` (an addition): the ground-truth maps are raw annotations and get
    LoadAnnotations' reduce_zero_label mapping inside the kernel."""
    default_prefix = None

    def __init__(self, ignore_index=255, iou_metrics=["mIoU"], nan_to_num=None, beta=1, collect_device="cpu", output_dir=None,
                 format_only=False, prefix=None, label_reduce_zero=False, **kwargs):
        self.ignore_index = ignore_index
        self.metrics = [iou_metrics] if isinstance(iou_metrics, str) else list(iou_metrics)
        self.nan_to_num = nan_to_num
        self.beta = beta
        self.collect_device = collect_device
        self.output_dir = output_dir
        if self.output_dir and _is_main_process():
            import os
            os.makedirs(self.output_dir, exist_ok=True)
        self.format_only = format_only
        self.prefix = prefix or self.default_prefix
        self.label_reduce_zero = bool(label_reduce_zero)
        self.dataset_meta = None
        self._totals = None

    # ---- accumulation
    @property
    def num_classes(self):
        assert self.dataset_meta is not None and "classes" in self.dataset_meta, "set dataset_meta = dict(classes=[...]) first"
        return len(self.dataset_meta["classes"])

    def totals(self, device):
        """the int64 [3, K] accumulator {intersection, prediction areas, label areas}, created on first use"""
        if self._totals is None or self._totals.device != torch.device(device) or self._totals.shape[1] != self.num_classes:
            assert self._totals is None or not bool(self._totals.any()), "the predictions moved to another device mid-evaluation"
            self._totals = torch.zeros(3, self.num_classes, dtype=torch.int64, device=device)
        return self._totals

    def reset(self):
        if self._totals is not None:
            self._totals.zero_()

    def process(self, data_batch, data_samples):
        for sample in data_samples:
            pred = _field(sample, "pred_sem_seg")
            if not self.format_only:
                label = _field(sample, "gt_sem_seg")
                if label.device != pred.device:
                    label = label.to(pred.device, non_blocking=True)
                ops.seg_hist(pred, label, self.totals(pred.device), self.ignore_index, self.label_reduce_zero)
            if self.output_dir is not None:
                from PIL import Image
                basename = osp.splitext(osp.basename(_meta(sample, "img_path")))[0]
                mask = pred.squeeze().cpu().numpy()
                if _meta(sample, "reduce_zero_label", False):          # the data set's indices start at 1 (ADE20K's 1 .. 150)
                    mask = mask + 1
                Image.fromarray(mask.astype(np.uint8)).save(osp.abspath(osp.join(self.output_dir, f"{basename}.png")))

    @staticmethod
    def intersect_and_union(pred_label, label, num_classes, ignore_index):
        """-> (area_intersect, area_union, area_pred_label, area_label) of one image, int64 [num_classes] on the maps' device"""
        t = ops.seg_hist(pred_label, label.to(pred_label.device), torch.zeros(3, num_classes, dtype=torch.int64, device=pred_label.device),
                         ignore_index)
        return t[0], t[1] + t[2] - t[0], t[1], t[2]

    # ---- metrics
    @staticmethod
    def total_area_to_metrics(total_area_intersect, total_area_union, total_area_pred_label, total_area_label, metrics=["mIoU"],
                              nan_to_num=None, beta=1):
        """-> OrderedDict: 'aAcc' (scalar) and per class 'IoU' / 'Acc', 'Dice' / 'Acc', 'Fscore' / 'Precision' / 'Recall' (float64
        arrays; a class absent from a denominator is NaN unless nan_to_num replaces it).  Integer totals in, float64 arithmetic."""
        metrics = [metrics] if isinstance(metrics, str) else list(metrics)
        if not set(metrics).issubset(_ALLOWED):
            raise KeyError(f"metrics {metrics} is not supported")
        inter, union, pred, label = (np.asarray(a.cpu() if torch.is_tensor(a) else a).astype(np.float64)
                                     for a in (total_area_intersect, total_area_union, total_area_pred_label, total_area_label))
        with np.errstate(divide="ignore", invalid="ignore"):
            ret = OrderedDict(aAcc=np.float64(inter.sum()) / np.float64(label.sum()))
            for metric in metrics:
                if metric == "mIoU":
                    ret["IoU"], ret["Acc"] = inter / union, inter / label
                elif metric == "mDice":
                    ret["Dice"], ret["Acc"] = 2 * inter / (pred + label), inter / label
                else:
                    precision, recall = inter / pred, inter / label
                    ret["Fscore"] = (1 + beta ** 2) * (precision * recall) / ((beta ** 2 * precision) + recall)
                    ret["Precision"], ret["Recall"] = precision, recall
        if nan_to_num is not None:
            ret = OrderedDict((k, np.nan_to_num(v, nan=nan_to_num)) for k, v in ret.items())
        return ret

    def compute_metrics(self, totals):
        """totals: int64 [3, K] {intersection, prediction areas, label areas} summed over the data set -> {'aAcc', 'mIoU', 'mAcc',
        ...}: round(nanmean * 100, 2); the per-class table goes to the log"""
        if self.format_only:
            logging.getLogger("spike2former_amd").info("results are saved to %s", osp.dirname(self.output_dir or ""))
            return OrderedDict()
        t = np.asarray(totals.cpu() if torch.is_tensor(totals) else totals)
        assert t.ndim == 2 and t.shape[0] == 3 and t.dtype.kind in "iu", "totals: an integer [3, K] array"
        t = t.astype(np.int64)
        ret = self.total_area_to_metrics(t[0], t[1] + t[2] - t[0], t[1], t[2], self.metrics, self.nan_to_num, self.beta)
        out = OrderedDict()
        for k, v in ret.items():
            out[k if k == "aAcc" else "m" + k] = round(_nanmean(v) * 100, 2)
        ret.pop("aAcc")
        names = list(self.dataset_meta["classes"]) if self.dataset_meta and "classes" in self.dataset_meta else [str(i) for i in range(t.shape[1])]
        width = max([len("Class")] + [len(str(n)) for n in names])
        lines = ["per class results:", "  ".join(["Class".ljust(width)] + [k.rjust(9) for k in ret])]
        for i, n in enumerate(names):
            lines.append("  ".join([str(n).ljust(width)] + [f"{float(v[i]) * 100:9.2f}" for v in ret.values()]))
        logging.getLogger("spike2former_amd").info("\n".join(lines))
        return out

    def evaluate(self, size=None):
        """Sum the ranks' totals (one int64 all-reduce over the default process group when one is initialised), read them back
        once, -> compute_metrics (keys 'prefix/name' with a prefix); the accumulator is zeroed for the next evaluation.  `size`
        (mmengine: the data set's length, to drop padded duplicates) is accepted and unused: see the module docstring."""
        import torch.distributed as dist
        t = self._totals if self._totals is not None else torch.zeros(3, self.num_classes, dtype=torch.int64)
        if not self.format_only and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            t = t.clone() if not (t.is_cuda and dist.get_backend() == "gloo") else t.cpu()
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
        out = self.compute_metrics(t.cpu())
        self.reset()
        if self.prefix:
            out = OrderedDict((f"{self.prefix}/{k}", v) for k, v in out.items())
        return out


@METRICS.register_module()
class ConfusionMatrix:
    """The class-pair table of an evaluation: matrix[label][prediction] in pixels (the reference's
    tools/analysis_tools/confusion_matrix.py:46-65, there a host-side bincount per image) -- which class the missed pixels of a bad
    IoU row went to.  Per image ONE `ops.seg_confusion` launch into an int64 [K, K] accumulator on the prediction's device, one
    all-reduce and one read-back in `evaluate()`, as IoUMetric.  ignore_index / prefix / collect_device (accepted and unused) /
    label_reduce_zero as IoUMetric; a pixel counts iff its label is not ignore_index and both its label and its prediction are
    classes (the reference's tool has no ignore_index and fails on a 255 label).  IoUMetric's three rows are this table's diagonal,
    column sums and row sums -- `totals()` -- so `evaluate()` returns the same aAcc / mIoU / mAcc."""
    default_prefix = None

    def __init__(self, ignore_index=255, label_reduce_zero=False, prefix=None, collect_device="cpu", **kwargs):
        self.ignore_index = ignore_index
        self.label_reduce_zero = bool(label_reduce_zero)
        self.prefix = prefix or self.default_prefix
        self.collect_device = collect_device
        self.dataset_meta = None
        self._acc = None
        self.matrix = None          # numpy int64 [K, K] of the last evaluate()

    @property
    def num_classes(self):
        assert self.dataset_meta is not None and "classes" in self.dataset_meta, "set dataset_meta = dict(classes=[...]) first"
        return len(self.dataset_meta["classes"])

    def accumulator(self, device):
        """the int64 [K, K] accumulator, created on first use (the rules of IoUMetric.totals)"""
        if self._acc is None or self._acc.device != torch.device(device) or self._acc.shape[0] != self.num_classes:
            assert self._acc is None or not bool(self._acc.any()), "the predictions moved to another device mid-evaluation"
            self._acc = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64, device=device)
        return self._acc

    def reset(self):
        if self._acc is not None:
            self._acc.zero_()

    def process(self, data_batch, data_samples):
        for sample in data_samples:
            pred = _field(sample, "pred_sem_seg")
            label = _field(sample, "gt_sem_seg")
            if label.device != pred.device:
                label = label.to(pred.device, non_blocking=True)
            ops.seg_confusion(pred, label, self.accumulator(pred.device), self.ignore_index, self.label_reduce_zero)

    # ---- views of the last evaluated matrix
    def _evaluated(self):
        assert self.matrix is not None, "evaluate() first"
        return self.matrix

    def _names(self):
        return [str(n) for n in self.dataset_meta["classes"]]

    def totals(self):
        """-> int64 [3, K] {diagonal, column sums, row sums} = IoUMetric's {intersection, prediction areas, label areas}"""
        m = self._evaluated()
        return np.stack([np.diagonal(m), m.sum(axis=0), m.sum(axis=1)]).astype(np.int64)

    def normalized(self):
        """-> float64 [K, K]: every row in percent of its sum (confusion_matrix.py:85-88); an empty row is NaN"""
        m = self._evaluated().astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return m / m.sum(axis=1, keepdims=True) * 100

    def top_confusions(self, n=10):
        """-> the n largest off-diagonal entries as (label name, prediction name, pixels, percent of the label's row), by pixels
        (descending), then by label and prediction index (ties are deterministic); the percent of an empty row is NaN"""
        m = self._evaluated()
        K = m.shape[0]
        idx = np.flatnonzero(~np.eye(K, dtype=bool).reshape(-1))
        idx = idx[np.argsort(-m.reshape(-1)[idx], kind="stable")][:max(int(n), 0)]          # stable: ties stay in index order
        names, pct = self._names(), self.normalized()
        return [(names[i // K], names[i % K], int(m.flat[i]), float(pct.flat[i])) for i in (int(i) for i in idx)]

    def save(self, path):
        """the int64 matrix as .npy, or as .csv with the class names as the header line"""
        m = self._evaluated()
        ext = osp.splitext(path)[1].lower()
        if ext == ".npy":
            np.save(path, m)
        elif ext == ".csv":
            with open(path, "w") as f:
                f.write(",".join(self._names()) + "\n")
                for row in m:
                    f.write(",".join(str(int(v)) for v in row) + "\n")
        else:
            raise ValueError(f"{path}: .npy or .csv")

    def evaluate(self, size=None, n=10):
        """Sum the ranks' matrices (one int64 all-reduce over the default process group when one is initialised), read the sum back
        once into `self.matrix`, zero the accumulator -> {'aAcc', 'mIoU', 'mAcc'} of the matrix through IoUMetric's arithmetic
        (keys 'prefix/name' with a prefix).  The per-class table and the `n` largest confusions go to the log.  `size` is accepted
        and unused, as in IoUMetric.evaluate."""
        import torch.distributed as dist
        t = self._acc if self._acc is not None else torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            t = t.clone() if not (t.is_cuda and dist.get_backend() == "gloo") else t.cpu()
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
        self.matrix = t.cpu().numpy().astype(np.int64, copy=True)
        self.reset()
        scorer = IoUMetric(ignore_index=self.ignore_index, iou_metrics=["mIoU"])
        scorer.dataset_meta = self.dataset_meta
        out = scorer.compute_metrics(self.totals())
        top = [t for t in self.top_confusions(n) if t[2] > 0]
        if top:
            lines = ["largest confusions (label -> prediction: pixels, % of the label's row):"]
            lines += [f"  {a} -> {b}: {px}, {pct:.2f}" for a, b, px, pct in top]
            logging.getLogger("spike2former_amd").info("\n".join(lines))
        if self.prefix:
            out = OrderedDict((f"{self.prefix}/{k}", v) for k, v in out.items())
        return out


def _is_main_process():
    import torch.distributed as dist
    return not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0


def evaluate(model, batches, metric, *, rank=0, world_size=1, hooks=()):
    """mmengine's TestLoop with ResetModelHook.before_test_iter for one rank: every `world_size`-th batch starting at `rank` (no
    padding: see the module docstring) -- membranes reset, `model.test_step(batch)` (an EncoderDecoder or a SegTTAModel),
    `metric.process` -- then `metric.evaluate()`.  Nothing inside the loop reads the device back.  `metric` may be a list or tuple
    of metrics: each processes every batch's samples, and their dictionaries are merged in order.  `hooks`: after the metrics have
    processed a batch, every hook's `after_test_iter(i_local, batch, samples)` runs (a SegVisualizationHook), i_local counting the
    batches THIS rank ran, from 0."""
    metrics = list(metric) if isinstance(metric, (list, tuple)) else [metric]
    hooks, i_local = tuple(hooks), 0
    model.eval()
    with torch.no_grad():
        for i, batch in enumerate(batches):
            if i % world_size != rank:
                continue
            reset_net(model)
            samples = model.test_step(batch)
            for m in metrics:
                m.process(batch, samples)
            for h in hooks:
                h.after_test_iter(i_local, batch, samples)
            i_local += 1
    if not isinstance(metric, (list, tuple)):
        return metric.evaluate()
    out = OrderedDict()
    for m in metrics:
        out.update(m.evaluate())
    return out
