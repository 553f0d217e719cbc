"""ConfusionMatrix and its class-pair op without a GPU: the C ABI's validation, `ops.seg_confusion`'s CPU arithmetic against a numpy
restatement of the participation rule, the cross-check against `ops.seg_hist` (whose three rows are the table's diagonal, column
sums and row sums) and the host-side evaluator."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_confusion(pred, label, K, ignore_index=255, reduce_zero_label=False):
    """numpy int64 [K, K], row = label, column = prediction: the pixels that take part (label != ignore_index after the
    reduce_zero_label mapping, label a class, prediction a class -- integral for a float map, NaN never) counted as the reference's
    tools/analysis_tools/confusion_matrix.py:46-65 counts every pixel: bincount(K * label + pred, minlength = K * K) as [K, K]."""
    pred = np.asarray(pred.cpu() if torch.is_tensor(pred) else pred)
    lab = np.asarray(label.cpu() if torch.is_tensor(label) else label).astype(np.int64)
    if lab.shape != pred.shape:
        lab = lab.T
    if reduce_zero_label:
        lab = np.where((lab == 0) | (lab == 255), 255, lab - 1)
    with np.errstate(invalid="ignore"):
        ok = (pred >= 0) & (pred < K)
        if pred.dtype.kind == "f":
            ok &= pred == np.trunc(pred)
    ok &= (lab != ignore_index) & (lab >= 0) & (lab < K)
    pc = np.where(ok, pred, 0).astype(np.int64)
    return np.bincount(K * lab[ok] + pc[ok], minlength=K * K).reshape(K, K).astype(np.int64)


def zeros(K, dev="cpu"):
    return torch.zeros(K, K, dtype=torch.int64, device=dev)


# ------------------------------------------------------------------------------------------------------------------ 1. ABI
def test_seg_confusion_symbol_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "s2f.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "spike2former_amd", "libs2f_hip.so"))
    from spike2former_amd import _lib, ops
    decl = re.search(r"\bint\s+s2f_seg_confusion\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert decl and hasattr(lib, "s2f_seg_confusion") and "s2f_seg_confusion" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["s2f_seg_confusion"][1]) == len(decl.group(1).split(",")) == 13
    assert int(re.search(r"#define S2F_ABI_VERSION (\d+)", src).group(1)) >= 40
    assert int(re.search(r"#define S2F_SEG_CONF_LDS_BYTES (\d+)", src).group(1)) == ops.SEG_CONF_LDS_BYTES
    assert int(re.search(r"#define S2F_SEG_CONF_GLOBAL (\d+)", src).group(1)) == 2


def test_seg_confusion_argument_errors_without_a_gpu():
    from spike2former_amd._lib import lib
    from spike2former_amd import ops
    p = ctypes.c_void_p(64)           # never dereferenced: validation fails before any launch
    ok = dict(pd=0, ld=0, rs=4, ps=1, W=4, HW=16, K=3, ign=255, fl=0)

    def call(pred=p, label=p, matrix=p, **kw):
        a = dict(ok, **kw)
        return lib.s2f_seg_confusion(pred, a["pd"], label, a["ld"], a["rs"], a["ps"], a["W"], a["HW"], a["K"], a["ign"], a["fl"], matrix,
                                     None)
    for kw in (dict(pred=None), dict(label=None), dict(matrix=None)):
        assert call(**kw) == -1 and b"s2f_seg_confusion: null" in lib.s2f_last_error()
    assert call(K=0) == -1 and b"K 0" in lib.s2f_last_error()
    assert call(K=ops.SEG_HIST_MAX_CLASSES + 1) == -1 and b"K 2049 outside 1 .. 2048" in lib.s2f_last_error()
    assert call(HW=18) == -1 and b"no whole number of rows" in lib.s2f_last_error()
    assert call(fl=4) == -1 and b"unknown flags 4" in lib.s2f_last_error()
    assert call(fl=8 | 1) == -1 and b"unknown flags" in lib.s2f_last_error()
    assert call(matrix=ctypes.c_void_p(68)) == -2 and b"not aligned" in lib.s2f_last_error()
    assert call(HW=0) == -1 and call(HW=2 ** 31) == -1 and call(pd=2) == -1 and call(ld=7) == -1 and call(rs=-1) == -1


# ------------------------------------------------------------------------------------------------------------------ 2. the op on CPU
def _maps(seed, H, W, K, float_pred=False):
    """random maps with every kind of pixel: ignored, labelled outside the classes, predicted -1 / K / (float) 2.5 / NaN"""
    rng = np.random.default_rng(seed)
    label = rng.integers(0, min(K + 2, 255), size=(H, W)).astype(np.uint8)
    label[rng.random((H, W)) < 0.1] = 255
    pred = rng.integers(-1, K + 1, size=(H, W))
    if float_pred:
        pred = pred.astype(np.float32)
        pred[rng.random((H, W)) < 0.05] = 2.5
        pred[rng.random((H, W)) < 0.05] = np.nan
    return torch.from_numpy(pred), torch.from_numpy(label)


@pytest.mark.parametrize("K", [1, 2, 7, 150])
@pytest.mark.parametrize("float_pred", [False, True])
def test_seg_confusion_cpu_equals_the_numpy_reference(K, float_pred):
    from spike2former_amd import ops
    pred, label = _maps(10 * K + float_pred, 23, 37, K, float_pred)
    want = ref_confusion(pred, label, K)
    assert want.sum() > 0 and want.sum() < pred.numel()
    for ld in (torch.uint8, torch.int64):
        got = ops.seg_confusion(pred, label.to(ld), zeros(K))
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want), (K, ld)
        assert np.array_equal(ops.seg_confusion(pred[None], label.to(ld)[None], zeros(K)).numpy(), want)
    # a label stored transposed is read in place
    lt = label.t().contiguous()
    assert lt.shape == (37, 23) and np.array_equal(ops.seg_confusion(pred, lt, zeros(K)).numpy(), want)
    # another ignore_index; reduce_zero_label on the raw annotation
    assert np.array_equal(ops.seg_confusion(pred, label, zeros(K), ignore_index=1).numpy(), ref_confusion(pred, label, K, 1))
    got = ops.seg_confusion(pred, label, zeros(K), reduce_zero_label=True)
    want_rzl = ref_confusion(pred, label, K, reduce_zero_label=True)
    assert np.array_equal(got.numpy(), want_rzl) and not np.array_equal(want_rzl, want)
    # two calls into one accumulator add; the route switch is accepted (and means nothing) on the CPU
    acc = zeros(K)
    assert ops.seg_confusion(pred, label, acc) is acc
    pred2, label2 = _maps(99 + K, 23, 37, K, float_pred)
    ops.seg_confusion(pred2, label2, acc, route="global")
    assert np.array_equal(acc.numpy(), want + ref_confusion(pred2, label2, K))


def test_seg_confusion_refuses_a_wrong_accumulator():
    from spike2former_amd import ops
    pred, label = _maps(1, 4, 4, 3)
    for bad in (torch.zeros(3, 3, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int64), torch.zeros(3, 6, dtype=torch.int64)[:, ::2],
                torch.zeros(9, dtype=torch.int64)):
        with pytest.raises(AssertionError):
            ops.seg_confusion(pred, label, bad)
    with pytest.raises(AssertionError):
        ops.seg_confusion(pred, label, zeros(3), route="lds")


@pytest.mark.parametrize("float_pred", [False, True])
def test_the_histogram_rows_are_the_tables_diagonal_and_marginals(float_pred):
    from spike2former_amd import ops
    K = 19
    pred, label = _maps(5 + float_pred, 31, 29, K, float_pred)
    m = ops.seg_confusion(pred, label, zeros(K))
    t = ops.seg_hist(pred, label, torch.zeros(3, K, dtype=torch.int64))
    assert torch.equal(m.diagonal(), t[0])
    assert not torch.equal(m.sum(0), t[1]) and not torch.equal(m.sum(1), t[2])          # invalid predictions / labels count in one only
    # every participating pixel with a valid prediction and a valid label: the marginals are the other two rows
    valid_pred = torch.from_numpy(np.random.default_rng(6).integers(0, K, size=pred.shape)).to(pred.dtype)
    label = torch.where((label >= K) & (label != 255), torch.zeros_like(label), label)
    m = ops.seg_confusion(valid_pred, label, zeros(K))
    t = ops.seg_hist(valid_pred, label, torch.zeros(3, K, dtype=torch.int64))
    assert torch.equal(m.diagonal(), t[0]) and torch.equal(m.sum(0), t[1]) and torch.equal(m.sum(1), t[2])
    assert int(m.sum()) == int((label != 255).sum())


# ------------------------------------------------------------------------------------------------------------------ 3. the evaluator
NAMES = ["sky", "wall", "tree"]


def hand_samples():
    """three images, K = 3, counted by hand.  Pairs (label -> prediction): image 0: 0->0 x3, 0->1 x2, ignored x1;
    image 1: 1->1 x2, 1->0 x2, 0->2 x2; image 2: 1->1 x1, 0->0 x1, ignored x2.  Class 2 is never a label: an empty row."""
    maps = [([[0, 0, 0], [1, 1, 2]], [[0, 0, 0], [0, 0, 255]]),
            ([[1, 1, 0], [0, 2, 2]], [[1, 1, 1], [1, 0, 0]]),
            ([[1, 0], [2, 2]], [[1, 0], [255, 255]])]
    return [dict(pred_sem_seg=dict(data=torch.tensor(p)[None]), gt_sem_seg=dict(data=torch.tensor(l, dtype=torch.uint8)[None]))
            for p, l in maps]


HAND = np.array([[4, 2, 2], [2, 3, 0], [0, 0, 0]], dtype=np.int64)


def cm_of(samples, **kw):
    import spike2former_amd as s2f
    m = s2f.METRICS.build(dict(type="ConfusionMatrix", **kw))
    assert isinstance(m, s2f.ConfusionMatrix)
    m.dataset_meta = dict(classes=NAMES)
    m.process({}, samples)
    return m


def test_confusion_matrix_on_three_images_counted_by_hand(tmp_path):
    import spike2former_amd as s2f
    m = cm_of(hand_samples())
    assert m.matrix is None and torch.equal(m._acc, torch.from_numpy(HAND))
    got = m.evaluate()
    assert m.matrix.dtype == np.int64 and np.array_equal(m.matrix, HAND)
    assert not bool(m._acc.any())                                                   # evaluate() zeroes the accumulator
    assert np.array_equal(m.totals(), np.array([[4, 3, 0], [6, 5, 2], [8, 5, 0]]))
    n = m.normalized()
    assert n.dtype == np.float64 and np.array_equal(n[0], [50.0, 25.0, 25.0]) and np.array_equal(n[1], [40.0, 60.0, 0.0])
    assert np.isnan(n[2]).all()                                                     # the empty row
    # three entries of 2 pixels tie: (0, 1), (0, 2), (1, 0) in index order, then the zeros in index order
    top = m.top_confusions()
    assert top[:3] == [("sky", "wall", 2, 25.0), ("sky", "tree", 2, 25.0), ("wall", "sky", 2, 40.0)]
    assert [t[:3] for t in top[3:]] == [("wall", "tree", 0), ("tree", "sky", 0), ("tree", "wall", 0)] and np.isnan(top[-1][3])
    assert m.top_confusions(2) == top[:2] and m.top_confusions(0) == []
    # the same samples through IoUMetric: the same summary
    iou = s2f.IoUMetric()
    iou.dataset_meta = dict(classes=NAMES)
    iou.process({}, hand_samples())
    assert np.array_equal(iou._totals.numpy(), m.totals())
    want = iou.evaluate()
    assert list(got) == ["aAcc", "mIoU", "mAcc"] and got == want and got["aAcc"] == 53.85
    # save: both formats round-trip
    m.save(str(tmp_path / "cm.npy"))
    back = np.load(tmp_path / "cm.npy")
    assert back.dtype == np.int64 and np.array_equal(back, HAND)
    m.save(str(tmp_path / "cm.csv"))
    lines = (tmp_path / "cm.csv").read_text().splitlines()
    assert lines[0].split(",") == NAMES and np.array_equal(np.array([[int(v) for v in ln.split(",")] for ln in lines[1:]]), HAND)
    with pytest.raises(ValueError):
        m.save(str(tmp_path / "cm.png"))
    # a second evaluate() has nothing to score, and replaces the matrix
    assert np.isnan(m.evaluate()["mIoU"]) and not m.matrix.any()


def test_confusion_matrix_prefix_reduce_zero_and_the_log(caplog):
    m = cm_of(hand_samples(), prefix="val")
    with caplog.at_level("INFO", logger="spike2former_amd"):
        assert list(m.evaluate()) == ["val/aAcc", "val/mIoU", "val/mAcc"]
    text = caplog.text
    assert "per class results" in text and "sky -> wall: 2, 25.00" in text and "wall -> tree" not in text          # no zero lines
    # raw annotations: 0 = unlabelled, class c stored as c + 1
    raw = [dict(pred_sem_seg=s["pred_sem_seg"],
                gt_sem_seg=dict(data=torch.where(s["gt_sem_seg"]["data"] == 255, torch.zeros((), dtype=torch.uint8),
                                                 s["gt_sem_seg"]["data"] + 1))) for s in hand_samples()]
    m = cm_of(raw, label_reduce_zero=True, collect_device="gpu")
    m.evaluate()
    assert np.array_equal(m.matrix, HAND)
    with pytest.raises(AssertionError):
        cm_of([]).totals()                                                          # nothing evaluated yet


class HandModel(torch.nn.Module):
    def test_step(self, batch):
        return batch["data_samples"]


def hand_batches():
    return [dict(inputs=[torch.zeros(3, 4, 4)], data_samples=[s]) for s in hand_samples()]


def test_evaluate_takes_a_list_of_metrics_and_one_metric_as_before():
    import spike2former_amd as s2f
    iou, cm = s2f.IoUMetric(), s2f.ConfusionMatrix(prefix="cm")
    iou.dataset_meta = cm.dataset_meta = dict(classes=NAMES)
    model = HandModel().train()
    got = s2f.evaluate(model, hand_batches(), [iou, cm])
    assert not model.training and list(got) == ["aAcc", "mIoU", "mAcc", "cm/aAcc", "cm/mIoU", "cm/mAcc"]
    assert [got[k] for k in ("aAcc", "mIoU", "mAcc")] == [got[f"cm/{k}"] for k in ("aAcc", "mIoU", "mAcc")]
    assert np.array_equal(cm.matrix, HAND)
    single = s2f.evaluate(model, hand_batches(), iou)                               # one metric: its own dictionary
    assert list(single) == ["aAcc", "mIoU", "mAcc"] and all(single[k] == got[k] for k in single)
    assert s2f.evaluate(model, hand_batches(), (cm,)) == {f"cm/{k}": v for k, v in single.items()}
    # a rank's share
    s2f.evaluate(model, hand_batches(), [cm], rank=1, world_size=2)
    assert np.array_equal(cm.matrix, ref_confusion(torch.tensor([[1, 1, 0], [0, 2, 2]]), torch.tensor([[1, 1, 1], [1, 0, 0]]), 3))


# ------------------------------------------------------------------------------------------------------------------ 4. two ranks over gloo
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


@pytest.mark.timeout(180)
def test_confusion_matrix_world2_gloo_gives_both_ranks_the_summed_matrix():
    import torch.multiprocessing as mp
    from _confusion_dist_worker import worker
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(worker, args=(2, _free_port(), out), nprocs=2, join=True)
    assert set(out.keys()) == {0, 1}
    for r in (0, 1):
        assert np.array_equal(np.array(out[r]["matrix"]), HAND) and out[r]["summary"] == out[0]["summary"]
    assert out[0]["own"] != out[1]["own"] and np.array_equal(np.array(out[0]["own"]) + np.array(out[1]["own"]), HAND)
