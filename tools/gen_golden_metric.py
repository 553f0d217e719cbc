"""Fixture generator (test infrastructure, never imported by the package, the GPU tests, smoke() or bench.py): runs the REFERENCE's own
mmseg/evaluation/metrics/iou_metric.py on CPU and records DATA ONLY -> tests/golden/metric_iou.npz

  cases                      names; per case <name>.pred / <name>.label (uint8 maps), .K, .float_pred (the prediction is scored as
                             a float32 0 / 1 map), .transposed (the label is stored [W, H]), .areas (int64 [4, K]: intersect, union,
                             pred, label of IoUMetric.intersect_and_union)
  seqs                       names of case sequences of one K; per sequence <seq>.cases and, for beta in (1, 2) and nan_to_num in
                             (None, 0) under iou_metrics = ['mIoU', 'mDice', 'mFscore']:
                             <seq>.b<beta>.n<none|0>.<aAcc|IoU|Acc|Dice|Fscore|Precision|Recall>   total_area_to_metrics, unrounded
                             <seq>.b<beta>.n<none|0>.summary_keys / .summary_vals                 compute_metrics' rounded dict

The reference file is loaded by path with stand-ins for the third-party names it imports (mmengine's BaseMetric / logger / dist /
mkdir helper, prettytable, the mmseg registry) -- shells written here, no reference code.  Every per-class total stays far below
2^24, so the reference's float32 sums are exact.

    python tools/gen_golden_metric.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shells          # noqa: E402  (only for the location of the reference tree)


def load_reference():
    class BaseMetric:
        def __init__(self, collect_device="cpu", prefix=None):
            self.results, self.dataset_meta, self.prefix = [], None, prefix

    class _Logger:
        @staticmethod
        def get_current_instance():
            return _Logger()

        def info(self, *a, **k):
            pass

    class PrettyTable:
        def add_column(self, *a, **k):
            pass

        def get_string(self):
            return ""

    class _Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    mod("mmengine")
    mod("mmengine.dist", is_main_process=lambda: True)
    mod("mmengine.evaluator", BaseMetric=BaseMetric)
    mod("mmengine.logging", MMLogger=_Logger, print_log=lambda *a, **k: None)
    mod("mmengine.utils", mkdir_or_exist=lambda *a, **k: None)
    mod("prettytable", PrettyTable=PrettyTable)
    mod("mmseg")
    mod("mmseg.registry", METRICS=_Registry())
    path = os.path.join(ref_shells.SEG, "mmseg", "evaluation", "metrics", "iou_metric.py")
    spec = importlib.util.spec_from_file_location("_ref_iou_metric", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.IoUMetric


def blocky(rng, H, W, classes, bh, bw):
    """a map of bh x bw blocks, each one of `classes`"""
    grid = rng.choice(classes, size=((H + bh - 1) // bh, (W + bw - 1) // bw))
    return np.kron(grid, np.ones((bh, bw), dtype=np.int64))[:H, :W].astype(np.uint8)


def make_cases():
    rng = np.random.default_rng(20240607)
    cases = []

    def add(name, K, pred, label, float_pred=False, transposed=False):
        cases.append(dict(name=name, K=K, pred=np.ascontiguousarray(pred, dtype=np.uint8),
                          label=np.ascontiguousarray(label, dtype=np.uint8), float_pred=float_pred, transposed=transposed))

    # K = 150: blocky maps over a few classes (most classes absent from both maps), ignored rows, labels of 200 (neither a class nor
    # the ignore index), predictions >= K on scored and on ignored pixels
    some = np.array([0, 3, 7, 12, 41, 88, 149])
    label = blocky(rng, 96, 128, some, 16, 32)
    pred = blocky(rng, 96, 128, some, 24, 16)
    pred[:, :40] = label[:, :40]
    label[10:14, :] = 255
    label[60:, 100:] = 255
    label[30:38, 50:70] = 200
    pred[40:50, 20:30] = 180
    pred[11:13, 5:60] = 151
    pred[70:80, 110:120] = 255
    add("k150_blocky", 150, pred, label)
    add("k150_noise", 150, rng.integers(0, 160, size=(64, 96)), np.where(rng.random((64, 96)) < 0.1, 255, rng.integers(0, 150, size=(64, 96))))
    same = blocky(rng, 80, 112, np.arange(0, 150, 5), 8, 8)
    add("k150_equal", 150, same, same)
    add("k150_all_ignored", 150, blocky(rng, 48, 64, some, 8, 8), np.full((48, 64), 255))
    label = blocky(rng, 72, 120, some, 12, 24)
    label[:5] = 255
    pred = np.where(rng.random((72, 120)) < 0.7, label, blocky(rng, 72, 120, some, 9, 15))
    add("k150_transposed", 150, pred, label.T, transposed=True)
    # K = 19
    label = blocky(rng, 128, 160, np.arange(19), 32, 20)
    label[rng.random((128, 160)) < 0.05] = 255
    pred = np.where(rng.random((128, 160)) < 0.8, label, blocky(rng, 128, 160, np.arange(19), 16, 40))
    pred[pred == 255] = 4
    add("k19_blocky", 19, pred, label)
    add("k19_noise", 19, rng.integers(0, 19, size=(50, 70)), rng.integers(0, 21, size=(50, 70)))
    # K = 2, the float32 0 / 1 prediction of a one-class head against a 0 / 1 / 255 label
    label = blocky(rng, 64, 64, np.array([0, 1]), 16, 16)
    label[:, 60:] = 255
    add("k2_float", 2, np.where(rng.random((64, 64)) < 0.85, label == 1, label != 1), label, float_pred=True)
    return cases


SEQS = {"k150": ["k150_blocky", "k150_noise", "k150_equal", "k150_all_ignored", "k150_transposed"],
        "k150_only_ignored": ["k150_all_ignored"], "k150_equal_only": ["k150_equal"],
        "k150_absent": ["k150_blocky", "k150_transposed"],          # most classes in neither map: NaN IoU
        "k19": ["k19_blocky", "k19_noise"], "k2": ["k2_float"]}


def main():
    assert ref_shells.available(), "the reference tree is not mounted"
    IoUMetric = load_reference()
    out, per_case = {}, {}
    cases = make_cases()
    out["cases"] = np.array([c["name"] for c in cases])
    for c in cases:
        pred = torch.from_numpy(c["pred"]).to(torch.float32 if c["float_pred"] else torch.int64)
        label = torch.from_numpy(c["label"]).to(pred)          # process(): gt_sem_seg.data.squeeze().to(pred_label)
        areas = IoUMetric.intersect_and_union(pred, label, c["K"], 255)
        per_case[c["name"]] = areas
        n = c["name"]
        out[f"{n}.pred"], out[f"{n}.label"] = c["pred"], c["label"]
        out[f"{n}.K"], out[f"{n}.float_pred"], out[f"{n}.transposed"] = np.int64(c["K"]), np.bool_(c["float_pred"]), np.bool_(c["transposed"])
        out[f"{n}.areas"] = np.stack([a.numpy().astype(np.int64) for a in areas])
        assert max(float(a.max()) for a in areas) < 2 ** 24
    out["seqs"] = np.array(list(SEQS))
    metrics = ["mIoU", "mDice", "mFscore"]
    for s, names in SEQS.items():
        out[f"{s}.cases"] = np.array(names)
        K = int(out[f"{names[0]}.K"])
        for beta in (1, 2):
            for nan in (None, 0):
                tag = f"{s}.b{beta}.n{'none' if nan is None else nan}"
                m = IoUMetric(iou_metrics=metrics, nan_to_num=nan, beta=beta)
                m.dataset_meta = dict(classes=[str(i) for i in range(K)])
                results = [per_case[n] for n in names]
                totals = [sum(r[i] for r in results) for i in range(4)]
                for k, v in IoUMetric.total_area_to_metrics(*totals, metrics, nan, beta).items():
                    out[f"{tag}.{k}"] = np.asarray(v)
                summary = m.compute_metrics(list(results))
                out[f"{tag}.summary_keys"] = np.array(list(summary))
                out[f"{tag}.summary_vals"] = np.array([np.float32(v) for v in summary.values()], dtype=np.float32)
    path = os.path.join(ROOT, "tests", "golden", "metric_iou.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", sum(c["pred"].size for c in cases), "pixels")


if __name__ == "__main__":
    import warnings
    warnings.filterwarnings("ignore")          # the reference's nanmean of an all-NaN column
    main()
