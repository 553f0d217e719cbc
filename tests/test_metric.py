"""IoUMetric and its class-histogram op without a GPU: the C ABI's validation, `ops.seg_hist`'s CPU arithmetic and the host-side metric
against what the reference's own mmseg/evaluation/metrics/iou_metric.py computed (tests/golden/metric_iou.npz, recorded by
tools/gen_golden_metric.py -- data only; nothing here restates the reference's function)."""
import ctypes
import os
import re
import socket
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [(b, n) for b in (1, 2) for n in (None, 0)]
PER_CLASS = ("IoU", "Acc", "Dice", "Fscore", "Precision", "Recall")
ALL3 = ["mIoU", "mDice", "mFscore"]


@pytest.fixture(scope="module")
def g(golden):
    return golden("metric_iou.npz")


def case_maps(g, name, pred_dtype=None, label_dtype=torch.uint8):
    """-> (pred, label, K) of a recorded case as the tensors the op takes; the label keeps its stored ([W, H] if transposed) layout"""
    pred = torch.from_numpy(g[f"{name}.pred"])
    pred = pred.to(pred_dtype or (torch.float32 if bool(g[f"{name}.float_pred"]) else torch.int64))
    return pred, torch.from_numpy(g[f"{name}.label"]).to(label_dtype), int(g[f"{name}.K"])


def want_totals(g, names):
    """recorded areas (intersect, union, pred, label) of the cases -> the op's [3, K] rows (intersect, pred, label), summed"""
    a = sum(g[f"{n}.areas"] for n in names)
    return torch.from_numpy(np.stack([a[0], a[2], a[3]]))


def tag(seq, beta, nan):
    return f"{seq}.b{beta}.n{'none' if nan is None else nan}"


# ------------------------------------------------------------------------------------------------------------------ 1. ABI
def test_seg_hist_symbol_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "s2f.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "spike2former_amd", "libs2f_hip.so"))
    from spike2former_amd import _lib
    assert re.search(r"\bint\s+s2f_seg_hist\s*\(", src)
    assert hasattr(lib, "s2f_seg_hist") and "s2f_seg_hist" in _lib.SIGNATURES
    bound = int(re.search(r"#define S2F_SEG_HIST_MAX_CLASSES (\d+)", src).group(1))
    from spike2former_amd import ops
    assert bound >= 1024 and ops.SEG_HIST_MAX_CLASSES == bound


def test_seg_hist_argument_errors_without_a_gpu():
    from spike2former_amd._lib import lib
    from spike2former_amd import ops
    p = ctypes.c_void_p(64)           # never dereferenced: validation fails before any launch
    ok = dict(pd=0, ld=0, rs=4, ps=1, W=4, HW=16, K=3, ign=255, fl=0)

    def call(pred=p, label=p, totals=p, **kw):
        a = dict(ok, **kw)
        return lib.s2f_seg_hist(pred, a["pd"], label, a["ld"], a["rs"], a["ps"], a["W"], a["HW"], a["K"], a["ign"], a["fl"], totals, None)
    for kw in (dict(pred=None), dict(label=None), dict(totals=None)):
        assert call(**kw) == -1 and b"null" in lib.s2f_last_error()
    assert call(HW=0) == -1 and b"HW" in lib.s2f_last_error()
    assert call(HW=2 ** 31) == -1 and b"32-bit" in lib.s2f_last_error()
    assert call(HW=18) == -1                                                     # no whole number of rows
    assert call(K=0) == -1 and b"K 0" in lib.s2f_last_error()
    assert call(K=ops.SEG_HIST_MAX_CLASSES + 1) == -1 and b"LDS" in lib.s2f_last_error()
    assert call(pd=2) == -1 and b"pred dtype" in lib.s2f_last_error()
    assert call(ld=7) == -1 and b"label dtype" in lib.s2f_last_error()
    assert call(fl=2) == -1 and b"flags" in lib.s2f_last_error()
    assert call(rs=-1) == -1


# ------------------------------------------------------------------------------------------------------------------ 2. the op on CPU
def test_seg_hist_cpu_equals_every_recorded_case(g):
    from spike2former_amd import ops
    for name in g["cases"]:
        name = str(name)
        float_pred = bool(g[f"{name}.float_pred"])
        for pd in ((torch.float32,) if float_pred else (torch.int64,)):
            for ld in (torch.uint8, torch.int64):
                pred, label, K = case_maps(g, name, pd, ld)
                if bool(g[f"{name}.transposed"]):
                    assert label.shape == pred.shape[::-1] and pred.shape[0] != pred.shape[1]
                got = ops.seg_hist(pred, label, torch.zeros(3, K, dtype=torch.int64))
                assert torch.equal(got, want_totals(g, [name])), (name, pd, ld)
                got = ops.seg_hist(pred[None], label[None], torch.zeros(3, K, dtype=torch.int64))          # [1, H, W] maps
                assert torch.equal(got, want_totals(g, [name])), (name, pd, ld)
    # 0 / 1 predictions of the float case scored as float32 AND as int64 agree
    pred, label, K = case_maps(g, "k2_float", torch.int64)
    assert torch.equal(ops.seg_hist(pred, label, torch.zeros(3, K, dtype=torch.int64)), want_totals(g, ["k2_float"]))


def test_seg_hist_cpu_accumulates_and_reads_the_transposed_label_in_place(g):
    from spike2former_amd import ops
    for seq in g["seqs"]:
        names = [str(n) for n in g[f"{seq}.cases"]]
        K = int(g[f"{names[0]}.K"])
        totals = torch.zeros(3, K, dtype=torch.int64)
        for n in names:
            pred, label, _ = case_maps(g, n)
            assert ops.seg_hist(pred, label, totals) is totals
        assert torch.equal(totals, want_totals(g, names)), seq
    # the transposed case: the contiguous copy of the label gives the same as the strided view the op reads
    pred, label, K = case_maps(g, "k150_transposed")
    a = ops.seg_hist(pred, label, torch.zeros(3, K, dtype=torch.int64))
    b = ops.seg_hist(pred, label.t().contiguous(), torch.zeros(3, K, dtype=torch.int64))
    assert torch.equal(a, b)


def test_intersect_and_union_static(g):
    import spike2former_amd as s2f
    for name in ("k150_blocky", "k19_noise", "k2_float"):
        pred, label, K = case_maps(g, name)
        areas = s2f.IoUMetric.intersect_and_union(pred, label, K, 255)
        assert all(a.dtype == torch.int64 for a in areas)
        assert np.array_equal(torch.stack(areas).numpy(), g[f"{name}.areas"])


# ------------------------------------------------------------------------------------------------------------------ 3. reduce_zero_label
def test_reduce_zero_label_is_the_three_step_rule():
    from spike2former_amd import ops
    rng = np.random.default_rng(3)
    K = 150
    raw = rng.integers(0, 152, size=(40, 56)).astype(np.uint8)          # ADE20K's raw annotation: 0 = unlabelled, 1 .. 150
    raw[rng.random(raw.shape) < 0.05] = 255
    raw[:3] = 0
    pred = torch.from_numpy(rng.integers(0, K, size=raw.shape))
    shifted = raw.astype(np.int64)
    shifted = np.where(shifted == 0, 255, np.where(shifted == 255, 255, shifted - 1))
    want = ops.seg_hist(pred, torch.from_numpy(shifted), torch.zeros(3, K, dtype=torch.int64))
    for ld in (torch.uint8, torch.int64):
        got = ops.seg_hist(pred, torch.from_numpy(raw).to(ld), torch.zeros(3, K, dtype=torch.int64), reduce_zero_label=True)
        assert torch.equal(got, want)
    assert int(want[2].sum()) == int(((raw != 0) & (raw != 255) & (raw <= K)).sum())          # 151 -> 150: takes part, counts nowhere
    # the metric's switch for raw annotations takes the same route
    import spike2former_amd as s2f
    m = s2f.IoUMetric(label_reduce_zero=True)
    m.dataset_meta = dict(classes=[str(i) for i in range(K)])
    m.process({}, [dict(pred_sem_seg=dict(data=pred[None]), gt_sem_seg=dict(data=torch.from_numpy(raw)[None]))])
    assert torch.equal(m._totals, want)


# ------------------------------------------------------------------------------------------------------------------ 4. the metrics
def test_total_area_to_metrics_vs_the_recorded_reference(g):
    import spike2former_amd as s2f
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # the all-ignored and absent-class cases must not warn
        for seq in g["seqs"]:
            t = want_totals(g, [str(n) for n in g[f"{seq}.cases"]])
            for beta, nan in COMBOS:
                got = s2f.IoUMetric.total_area_to_metrics(t[0], t[1] + t[2] - t[0], t[1], t[2], ALL3, nan, beta)
                assert list(got) == ["aAcc", "IoU", "Acc", "Dice", "Fscore", "Precision", "Recall"]
                for k in ("aAcc",) + PER_CLASS:
                    want = g[f"{tag(seq, beta, nan)}.{k}"].astype(np.float64)
                    have = np.asarray(got[k], dtype=np.float64)
                    assert have.shape == want.shape and np.array_equal(np.isnan(have), np.isnan(want)), (seq, beta, nan, k)
                    ok = ~np.isnan(want)
                    assert np.allclose(have[ok], want[ok], rtol=1e-6, atol=0), (seq, beta, nan, k)
    assert np.isnan(g["k150_absent.b1.nnone.IoU"]).any() and np.isnan(g["k150_only_ignored.b1.nnone.aAcc"])          # the cases exist


def test_compute_metrics_summary_vs_the_recorded_reference(g):
    import spike2former_amd as s2f
    compared = printed = 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for seq in g["seqs"]:
            names = [str(n) for n in g[f"{seq}.cases"]]
            K = int(g[f"{names[0]}.K"])
            for beta, nan in COMBOS:
                m = s2f.IoUMetric(iou_metrics=ALL3, nan_to_num=nan, beta=beta)
                m.dataset_meta = dict(classes=[f"c{i}" for i in range(K)])
                got = m.compute_metrics(want_totals(g, names))
                keys, vals = [str(k) for k in g[f"{tag(seq, beta, nan)}.summary_keys"]], g[f"{tag(seq, beta, nan)}.summary_vals"]
                assert list(got) == keys
                for k, want in zip(keys, vals):
                    have = got[k]
                    assert isinstance(have, float)
                    if np.isnan(want):
                        assert np.isnan(have), (seq, beta, nan, k)
                        continue
                    assert abs(have - float(want)) <= 0.01 + 1e-9, (seq, beta, nan, k, have, want)
                    compared += 1
                    # away from a rounding boundary (judged on the reference's own unrounded arrays) the printed values are equal
                    rec = g[f"{tag(seq, beta, nan)}.{'aAcc' if k == 'aAcc' else k[1:]}"].astype(np.float64).reshape(-1)
                    x = rec[~np.isnan(rec)].mean() * 100 * 100
                    if abs(x - np.floor(x) - 0.5) > 1e-4 * 100:
                        assert f"{have:.2f}" == f"{float(want):.2f}", (seq, beta, nan, k, have, want)
                        printed += 1
    assert compared >= 80 and printed >= 70, (compared, printed)


# ------------------------------------------------------------------------------------------------------------------ 5. host logic
def _samples(g, names, as_dict):
    from spike2former_amd.data_preprocessor import PixelData, SegDataSample
    out = []
    for i, n in enumerate(names):
        pred, label, _ = case_maps(g, n)
        if as_dict:
            out.append(dict(pred_sem_seg=dict(data=pred[None]), gt_sem_seg=dict(data=label[None]), img_path=f"dir/img{i}.jpg",
                            reduce_zero_label=True))
        else:
            d = SegDataSample(gt_sem_seg=label[None], metainfo=dict(img_path=f"dir/img{i}.jpg", reduce_zero_label=True))
            d.pred_sem_seg = PixelData(pred[None])
            out.append(d)
    return out


def test_metric_builds_from_the_config_dict_and_scores_both_sample_kinds(g):
    import spike2former_amd as s2f
    names = [str(n) for n in g["k150.cases"]]
    res = []
    for as_dict in (True, False):
        m = s2f.METRICS.build(dict(type="IoUMetric", iou_metrics=["mIoU"]))
        assert isinstance(m, s2f.IoUMetric) and m.ignore_index == 255 and m.metrics == ["mIoU"]
        m.dataset_meta = dict(classes=[str(i) for i in range(150)])
        m.process({}, _samples(g, names, as_dict))
        assert torch.equal(m._totals, want_totals(g, names))
        res.append(m.evaluate())
        assert not bool(m._totals.any())                                       # evaluate() resets
        assert np.isnan(m.evaluate()["mIoU"])                                  # ... so a second one has nothing to score
    assert res[0] == res[1] and list(res[0]) == ["aAcc", "mIoU", "mAcc"]
    vals = dict(zip((str(k) for k in g["k150.b1.nnone.summary_keys"]), g["k150.b1.nnone.summary_vals"]))
    for k, v in res[0].items():
        assert abs(v - float(vals[k])) <= 0.01 + 1e-9


def test_metric_prefix_and_unknown_metric(g):
    import spike2former_amd as s2f
    m = s2f.IoUMetric(iou_metrics=["mDice"], prefix="val")
    m.dataset_meta = dict(classes=["a", "b"])
    m.process({}, _samples(g, ["k2_float"], True))
    assert list(m.evaluate()) == ["val/aAcc", "val/mDice", "val/mAcc"]
    bad = s2f.IoUMetric(iou_metrics=["mIoU", "mAP"])
    bad.dataset_meta = dict(classes=["a", "b"])
    bad.process({}, _samples(g, ["k2_float"], True))
    with pytest.raises(KeyError):
        bad.evaluate()
    with pytest.raises(KeyError):
        s2f.IoUMetric.total_area_to_metrics(*([np.ones(2, dtype=np.int64)] * 4), metrics="mAP")


def test_metric_registers_upstream_only_where_a_metrics_registry_exists(monkeypatch):
    import sys
    import types
    import spike2former_amd as s2f
    table = {}

    class Reg:
        def register_module(self, name=None, module=None, force=False):
            table[name] = module
    fake = types.ModuleType("mmseg.registry")
    fake.MODELS, fake.METRICS = Reg(), Reg()
    monkeypatch.setitem(sys.modules, "mmseg", types.ModuleType("mmseg"))
    monkeypatch.setitem(sys.modules, "mmseg.registry", fake)
    done = s2f.register_upstream()
    assert "mmseg.registry:IoUMetric" in done and table["IoUMetric"] is s2f.IoUMetric
    del fake.METRICS
    assert "mmseg.registry:IoUMetric" not in s2f.register_upstream()


def test_format_only_writes_the_pngs_with_the_plus_one(g, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import spike2former_amd as s2f
    out = tmp_path / "fmt"
    m = s2f.IoUMetric(output_dir=str(out), format_only=True)
    m.dataset_meta = dict(classes=[str(i) for i in range(19)])
    names = ["k19_blocky", "k19_noise"]
    m.process({}, _samples(g, names, True))
    m.process({}, [s for s in _samples(g, names, False)][1:])                   # objects too; img1 is written again
    assert m._totals is None and m.evaluate() == {}
    for i, n in enumerate(names):
        png = np.asarray(Image.open(out / f"img{i}.png"))
        assert png.dtype == np.uint8 and np.array_equal(png, g[f"{n}.pred"] + 1)


# ------------------------------------------------------------------------------------------------------------------ 6. two ranks over gloo
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


@pytest.mark.timeout(180)
def test_evaluate_world2_gloo_gives_both_ranks_the_whole_set_summary(g):
    import torch.multiprocessing as mp
    from _metric_dist_worker import worker
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(worker, args=(2, _free_port(), out), nprocs=2, join=True)
    keys = [str(k) for k in g["k150.b2.nnone.summary_keys"]]
    vals = g["k150.b2.nnone.summary_vals"]
    assert set(out.keys()) == {0, 1} and out[0] == out[1] and list(out[0]) == keys
    for k, v in zip(keys, vals):
        assert abs(out[0][k] - float(v)) <= 0.01 + 1e-9, (k, out[0][k], v)


def test_evaluate_single_rank_loop(g):
    import spike2former_amd as s2f
    from _metric_dist_worker import RecordedModel, batches_of
    m = s2f.IoUMetric(iou_metrics=ALL3, beta=2)
    m.dataset_meta = dict(classes=[str(i) for i in range(150)])
    model = RecordedModel().train()
    got = s2f.evaluate(model, batches_of(np.load(os.path.join(ROOT, "tests", "golden", "metric_iou.npz")), "k150"), m)
    assert not model.training
    for k, v in zip((str(k) for k in g["k150.b2.nnone.summary_keys"]), g["k150.b2.nnone.summary_vals"]):
        assert abs(got[k] - float(v)) <= 0.01 + 1e-9


# ------------------------------------------------------------------------------------------------------------------ 7. beyond float32
def test_totals_beyond_float32_stay_exact():
    """bins above 2^24 that differ by +1: float32 totals (the reference's sums) cannot tell them apart, the int64 totals can"""
    import spike2former_amd as s2f
    big = 2 ** 24
    inter = np.array([big + 1, big + 3, 5 * big + 1, 7], dtype=np.int64)
    label = np.array([big + 2, big + 3, 5 * big + 3, 9], dtype=np.int64)
    pred = np.array([big + 1, big + 5, 5 * big + 1, 11], dtype=np.int64)
    assert int(np.float32(inter[0])) != int(inter[0]) and int(np.float32(label[1])) != int(label[1])          # float32 cannot hold them
    m = s2f.IoUMetric(iou_metrics=ALL3)
    m.dataset_meta = dict(classes=list("abcd"))
    got = m.compute_metrics(torch.from_numpy(np.stack([inter, pred, label])))
    si, sl = int(inter.sum()), int(label.sum())
    assert got["aAcc"] == round(si * 100 / sl, 2)
    per = s2f.IoUMetric.total_area_to_metrics(inter, pred + label - inter, pred, label, ALL3)
    from fractions import Fraction
    for c in range(4):
        assert abs(per["Acc"][c] - float(Fraction(int(inter[c]), int(label[c])))) <= 2e-16
        assert abs(per["IoU"][c] - float(Fraction(int(inter[c]), int(pred[c] + label[c] - inter[c])))) <= 2e-16
    assert per["Acc"][0] < 1.0 and per["aAcc"] == si / sl
