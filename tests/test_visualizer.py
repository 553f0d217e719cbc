"""CPU: ops.seg_draw's host arithmetic, the s2f_seg_draw argument rules, SegLocalVisualizer, SegVisualizationHook and evaluate()'s
hooks against tests/draw_ref.py, the numpy restatement of the reference's drawing.  Every comparison is byte equality."""
import ctypes
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draw_ref as D  # noqa: E402

PALETTE19 = [[(37 * k + 11) % 256, (91 * k + 5) % 256, (13 * k + 200) % 256] for k in range(19)]


def draw(image, palette, gt=None, pred=None, **kw):
    from spike2former_amd import ops
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    return ops.seg_draw(t(image), t(np.asarray(palette, np.uint8)), t(gt), t(pred), **kw).numpy()


def scene(h, w, K, seed, gt_dtype=np.uint8, pred_dtype=np.int64):
    """a random picture, a raw annotation holding 0, K - 1, K, K + 1 (when they fit the dtype), 254 and 255 among the classes, and a
    prediction holding K and 255 among them"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    gt = rng.integers(0, min(K + 2, 256), (h, w)).astype(gt_dtype)
    gt.reshape(-1)[rng.permutation(h * w)[:max(h * w // 8, 2)]] = rng.choice([254, 255], max(h * w // 8, 2))
    pred = rng.integers(0, K + 1, (h, w)).astype(pred_dtype)
    pred.reshape(-1)[rng.permutation(h * w)[:max(h * w // 16, 1)]] = 255
    return img, gt, pred


# ------------------------------------------------------------------------------------------------ 1. ops.seg_draw on CPU tensors
@pytest.mark.parametrize("gt_dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("pred_dtype", [np.int64, np.float32])
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("rzl", [False, True])
def test_cpu_draw_is_the_reference(gt_dtype, pred_dtype, bgr, rzl):
    img, gt, pred = scene(13, 21, 19, seed=1, gt_dtype=gt_dtype, pred_dtype=pred_dtype)
    for g, p in ((gt, pred), (gt, None), (None, pred)):
        got = draw(img, PALETTE19, g, p, bgr=bgr, reduce_zero_label=rzl)
        want = D.panel(img, PALETTE19, g, p, alpha=0.8, bgr=bgr, rzl=rzl)
        assert got.dtype == np.uint8 and got.shape == want.shape == (13, 21 * ((g is not None) + (p is not None)), 3)
        assert np.array_equal(got, want)


def test_cpu_draw_values_off_the_classes():
    K, pal = 19, PALETTE19
    img = np.random.default_rng(2).integers(0, 256, (2, 8, 3), dtype=np.uint8)
    gt = np.array([[0, K - 1, K, 254, 255, 1, 2, 3]] * 2, np.uint8)
    ints = np.array([[-1, K, 2 ** 31 + 3, 2 ** 40 + 3, np.iinfo(np.int64).min, 3, 0, K - 1]] * 2, np.int64)
    floats = np.array([[0.0, -0.0, 1.0, 0.5, np.nan, np.inf, 1e10, -1.0]] * 2, np.float32)
    for rzl in (False, True):
        for pred in (ints, floats):
            assert np.array_equal(draw(img, pal, gt, pred, reduce_zero_label=rzl), D.panel(img, pal, gt, pred, rzl=rzl))
    # what "paints nothing" means: the picture times 1 - alpha alone
    bare = (img * (1 - 0.8)).astype(np.uint8)
    got = draw(img, pal, pred=ints)
    assert np.array_equal(got[:, :5], bare[:, :5]) and not np.array_equal(got[:, 5:], bare[:, 5:])
    got = draw(img, pal, pred=floats)
    assert np.array_equal(got[:, 3:], bare[:, 3:])
    flat = np.ascontiguousarray(np.broadcast_to(np.array([10, 100, 200], np.uint8), (2, 8, 3)))
    got = draw(flat, pal, pred=floats)
    assert np.array_equal(got[:, 0], got[:, 1]) and not np.array_equal(got[:, 0], got[:, 3])          # -0.0 is class 0


def test_cpu_draw_accepts_a_leading_one_and_refuses_the_rest():
    from spike2former_amd import ops
    img, gt, pred = scene(5, 7, 19, seed=3)
    pal = torch.tensor(PALETTE19, dtype=torch.uint8)
    i, g, p = torch.from_numpy(img), torch.from_numpy(gt), torch.from_numpy(pred)
    want = D.panel(img, PALETTE19, gt, pred)
    assert np.array_equal(ops.seg_draw(i, pal, g[None], p[None]).numpy(), want)
    out = torch.zeros(5, 14, 3, dtype=torch.uint8)
    assert ops.seg_draw(i, pal, g, p, out=out) is out and np.array_equal(out.numpy(), want)
    # a non-contiguous map is made contiguous
    assert np.array_equal(ops.seg_draw(i, pal, pred=p.t().contiguous().t()).numpy(), D.panel(img, PALETTE19, pred=pred))
    with pytest.raises(ValueError):
        ops.seg_draw(i, pal)
    with pytest.raises(ValueError):
        ops.seg_draw(i, pal, pred=p, alpha=1.5)
    with pytest.raises(ValueError):
        ops.seg_draw(i, pal, pred=p[:, :5])
    with pytest.raises(TypeError):
        ops.seg_draw(i, pal, pred=p.to(torch.int32))
    with pytest.raises(RuntimeError):
        ops.seg_draw(i, pal.to("meta"), pred=p)          # mixed devices


# ------------------------------------------------------------------------------------------------ 2. the arithmetic itself
@pytest.mark.parametrize("alpha", D.ALPHAS)
def test_cpu_draw_every_value_pair(alpha):
    img, sem, pal = D.arithmetic_fixture()
    assert np.array_equal(draw(img, pal, pred=sem, alpha=alpha), D.panel(img, pal, pred=sem, alpha=alpha))


def test_the_fixture_sees_a_contracted_evaluation():
    """fma(v, 1 - alpha, fl64(c * alpha)) and fma(c, alpha, fl64(v * (1 - alpha))), each ONE rounding of the exact sum (emulated
    with fractions.Fraction: int / int division rounds correctly), on the fixture's inputs at alpha 0.8: both differ from the
    three-rounding reference at hundreds of the 65 536 (v, c) pairs, so a kernel that contracts cannot pass the fixture"""
    alpha = 0.8
    keep = 1 - alpha
    img, sem, pal = D.arithmetic_fixture()
    want = D.panel(img, pal, pred=sem, alpha=alpha)[..., 0].astype(np.int64)          # channel 0: c = column, v = row
    fa, fk = Fraction(alpha), Fraction(keep)
    differ = []
    for fused_first in (True, False):
        got = np.empty((256, 256), np.int64)
        for v in range(256):
            for c in range(256):
                exact = (Fraction(v) * fk + Fraction(float(c) * alpha)) if fused_first else (Fraction(float(v) * keep) + Fraction(c) * fa)
                got[v, c] = int(float(exact))
        differ.append(int((got != want).sum()))
    print("pairs at which a contracted evaluation differs:", differ)
    assert sorted(differ) == [644, 893], differ          # (what the issue of this feature measured, too)


# ------------------------------------------------------------------------------------------------ 3. the C ABI
def test_header_declares_seg_draw():
    src = open(os.path.join(ROOT, "include", "s2f.h")).read()
    assert re.search(r"\bint\s+s2f_seg_draw\s*\(", src) and "S2F_SEG_DRAW_BGR" in src
    assert int(re.search(r"#define S2F_ABI_VERSION (\d+)", src).group(1)) >= 43
    from spike2former_amd._lib import lib
    assert lib.s2f_version() >= 43


def test_seg_draw_argument_errors_before_any_launch():
    from spike2former_amd._lib import lib
    P = 1 << 20          # an aligned dummy address: never dereferenced on the host
    ok = dict(image=P, gt=P, gt_dtype=0, pred=P, pred_dtype=0, palette=P, K=19, alpha=0.8, flags=0, H=4, W=5, out=P)
    cases = [
        (dict(image=None), b"null pointer"), (dict(palette=None), b"null pointer"), (dict(out=None), b"null pointer"),
        (dict(gt=None, pred=None), b"neither"),
        (dict(H=0), b"bad picture size"), (dict(W=-1), b"bad picture size"),
        (dict(H=46341, W=46341), b"bad map size"),                        # 2^31 + 4 281 pixels
        (dict(H=1, W=2 ** 31 - 8), b"bad map size"),
        (dict(K=0), b"K 0 outside"), (dict(K=2049), b"K 2049 outside"),
        (dict(alpha=-0.01), b"alpha"), (dict(alpha=1.01), b"alpha"), (dict(alpha=float("nan")), b"alpha"),
        (dict(flags=2), b"unknown flags"), (dict(flags=8), b"unknown flags"),
        (dict(gt_dtype=2), b"unknown label dtype"), (dict(pred_dtype=2), b"unknown pred dtype"),
    ]
    for change, text in cases:
        a = dict(ok, **change)
        rc = lib.s2f_seg_draw(a["image"], a["gt"], a["gt_dtype"], a["pred"], a["pred_dtype"], a["palette"], a["K"], a["alpha"],
                              a["flags"], a["H"], a["W"], a["out"], None)
        assert rc == -1 and text in lib.s2f_last_error(), (change, rc, lib.s2f_last_error())
    # an int64 / fp32 map is aligned to its element (S2F_EALIGN); the byte streams are not
    rc = lib.s2f_seg_draw(P + 1, P + 1, 0, P + 4, 0, P + 3, 19, 0.8, 0, 4, 5, P + 1, None)
    assert rc == -2 and b"aligned" in lib.s2f_last_error()
    assert lib.s2f_seg_draw.argtypes[7] is ctypes.c_double          # alpha crosses the ABI as a double


# ------------------------------------------------------------------------------------------------ 4. SegLocalVisualizer
def sample(gt=None, pred=None, **meta):
    from spike2former_amd.data_preprocessor import PixelData, SegDataSample
    s = SegDataSample(gt_sem_seg=None if gt is None else torch.from_numpy(gt)[None], metainfo=meta)
    if pred is not None:
        s.pred_sem_seg = PixelData(torch.from_numpy(pred)[None])
    return s


def test_visualizer_meta_and_refusals():
    import spike2former_amd as s2f
    V = s2f.SegLocalVisualizer
    with pytest.raises(AssertionError):
        V(classes=["a", "b", "c"], palette=PALETTE19[:2])
    vis = V()
    assert vis.dataset_meta == dict(classes=None, palette=None) and vis.alpha == 0.8
    img, gt, pred = scene(5, 7, 19, seed=4)
    with pytest.raises(ValueError, match="palette"):          # nothing defaults to Cityscapes
        vis.add_datasample("x", img, sample(gt, pred))
    with pytest.raises(AssertionError):
        vis.dataset_meta = dict(classes=["a"], palette=PALETTE19)
    with pytest.raises(NotImplementedError, match="show"):
        V(palette=PALETTE19).add_datasample("x", img, sample(gt, pred), show=True)
    with pytest.raises(NotImplementedError, match="vis_backends.*TensorboardVisBackend"):
        V(vis_backends=[dict(type="LocalVisBackend"), dict(type="TensorboardVisBackend")])
    with pytest.raises(NotImplementedError, match="dataset_name.*palette="):
        V(dataset_name="ade")
    with pytest.raises(NotImplementedError, match="dataset_name"):
        V().set_dataset_meta(dataset_name="cityscapes")
    # the configs' own dictionary
    built = s2f.VISUALIZERS.build(dict(type="SegLocalVisualizer", vis_backends=[dict(type="LocalVisBackend")], name="visualizer"))
    assert isinstance(built, V) and built.name == "visualizer" and V.get_current_instance() is built
    built.dataset_meta = dict(classes=[str(i) for i in range(19)], palette=PALETTE19)
    got = built.add_datasample("x", img, sample(gt, pred))          # no save_dir: drawn, nothing written
    assert torch.is_tensor(got) and np.array_equal(got.numpy(), D.panel(img, PALETTE19, gt, pred))
    assert built.add_datasample("x", img, sample()) is None and built.add_datasample("x", img, None) is None


def test_visualizer_draws_and_writes(tmp_path):
    import spike2former_amd as s2f
    from PIL import Image
    img, gt, pred = scene(9, 11, 19, seed=5)
    vis = s2f.SegLocalVisualizer(save_dir=str(tmp_path / "run"), classes=[str(i) for i in range(19)], palette=PALETTE19, alpha=0.6)
    s = sample(gt, pred, reduce_zero_label=True)
    want = D.panel(img, PALETTE19, gt, pred, alpha=0.6, rzl=True)
    got = vis.add_datasample("val_a.jpg", img, s, step=7)
    assert np.array_equal(got.numpy(), want)
    path = tmp_path / "run" / "vis_image" / "val_a.jpg_7.png"          # mmengine's LocalVisBackend rule
    assert sorted(p.name for p in (tmp_path / "run" / "vis_image").iterdir()) == [path.name]
    assert np.array_equal(np.asarray(Image.open(path)), want)          # RGB in the file: the colours the palette names
    # out_file wins over save_dir
    other = tmp_path / "elsewhere" / "b.png"
    vis.add_datasample("val_b.jpg", img[..., ::-1], s, out_file=str(other), image_is_bgr=True)
    assert np.array_equal(np.asarray(Image.open(other)), want)
    assert sorted(p.name for p in (tmp_path / "run" / "vis_image").iterdir()) == [path.name]
    # one panel each, a dict sample, and _draw_sem_seg
    assert np.array_equal(vis.add_datasample("c", img, s, draw_gt=False, out_file=str(other)).numpy(),
                          D.panel(img, PALETTE19, pred=pred, alpha=0.6))
    d = dict(gt_sem_seg=dict(data=torch.from_numpy(gt)[None]), reduce_zero_label=False)
    assert np.array_equal(vis.add_datasample("d", img, d, out_file=str(other)).numpy(), D.panel(img, PALETTE19, gt=gt, alpha=0.6))
    meta = vis.dataset_meta
    assert np.array_equal(vis._draw_sem_seg(img, s.pred_sem_seg, meta["classes"], meta["palette"]).numpy(),
                          D.panel(img, PALETTE19, pred=pred, alpha=0.6))
    assert list(vis._palette_dev) == [torch.device("cpu")]          # uploaded once per device
    first = vis._palette_dev[torch.device("cpu")]
    vis.add_datasample("e", img, s, out_file=str(other))
    assert vis._palette_dev[torch.device("cpu")] is first
    vis.dataset_meta = dict(classes=meta["classes"], palette=PALETTE19[::-1])
    assert vis._palette_dev == {}


# ------------------------------------------------------------------------------------------------ 5. SegVisualizationHook
class Recorder:
    """a visualizer that records what the hook asks for"""

    def __init__(self):
        self.calls = []

    def add_datasample(self, name, image, **kw):
        self.calls.append((name, image, kw))


def outputs(*names):
    return [sample(img_path=n) for n in names]


def test_hook_draws_at_the_mmengine_indices():
    import spike2former_amd as s2f
    H = s2f.SegVisualizationHook
    assert s2f.HOOKS.get("SegVisualizationHook") is H
    pic = np.zeros((2, 2, 3), np.uint8)
    source = lambda batch, outs: [pic] * len(outs)  # noqa: E731
    with pytest.warns(UserWarning, match="draw is False"):
        off = H(visualizer=Recorder(), source=source)
    assert off.interval == 50 and off.step == 0
    for i in range(6):
        off.after_val_iter(i, None, outputs("a.png"))
    assert off.visualizer.calls == []
    for interval, want in ((1, [0, 1, 2, 3, 4, 5]), (2, [1, 3, 5]), (50, [])):
        h = H(draw=True, interval=interval, visualizer=Recorder(), source=source)
        for i in range(6):
            h._after_iter(i, None, outputs(f"/data/val/{i}.jpg"), mode="train")
        assert h.visualizer.calls == []
        for i in range(6):
            h.after_val_iter(i, None, outputs(f"/data/val/{i}.jpg"))
        assert [c[0] for c in h.visualizer.calls] == [f"val_{i}.jpg" for i in want]
    h = H(draw=True, interval=50, visualizer=Recorder(), source=source)
    h.step = 3
    h.after_test_iter(49, None, outputs("x/one.png", "x/two.png"))
    assert [(c[0], c[2]["step"], c[2]["image_is_bgr"]) for c in h.visualizer.calls] == [("test_one.png", 3, False), ("test_two.png", 3, False)]
    with pytest.raises(NotImplementedError, match="show"):
        H(draw=True, show=True)
    with pytest.raises(NotImplementedError, match="backend_args"):
        H(draw=True, backend_args=dict(backend="petrel"))


def test_hook_is_master_only(monkeypatch):
    import spike2former_amd as s2f
    h = s2f.SegVisualizationHook(draw=True, interval=1, visualizer=Recorder(), source=lambda b, o: [np.zeros((2, 2, 3), np.uint8)])
    monkeypatch.setattr(s2f.metrics, "_is_main_process", lambda: False)
    h.after_test_iter(0, None, outputs("a.png"))
    assert h.visualizer.calls == []
    monkeypatch.setattr(s2f.metrics, "_is_main_process", lambda: True)
    h.after_test_iter(0, None, outputs("a.png"))
    assert len(h.visualizer.calls) == 1


def test_hook_sources_in_order(tmp_path):
    """a `sources()` object or a callable before img_path; the img_path fallback decodes the file as RGB"""
    import spike2former_amd as s2f
    from PIL import Image
    img, gt, pred = scene(6, 9, 19, seed=6)
    other = 255 - img
    Image.fromarray(other).save(tmp_path / "f.png")
    s = sample(gt, pred, img_path=str(tmp_path / "f.png"))
    vis = s2f.SegLocalVisualizer(save_dir=str(tmp_path / "out"), palette=PALETTE19)
    s2f.SegVisualizationHook(draw=True, interval=1, visualizer=vis, source=lambda b, o: [img]).after_val_iter(0, None, [s])
    file = tmp_path / "out" / "vis_image" / "val_f.png_0.png"
    assert np.array_equal(np.asarray(Image.open(file)), D.panel(img, PALETTE19, gt, pred))

    class Staged:
        def sources(self):
            t = torch.from_numpy(np.ascontiguousarray(img[..., ::-1]))[None]
            t.is_bgr = True
            return t
    s2f.SegVisualizationHook(draw=True, interval=1, visualizer=vis, source=Staged()).after_test_iter(0, None, [s])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "vis_image" / "test_f.png_0.png")), D.panel(img, PALETTE19, gt, pred))
    file.unlink()
    s2f.SegVisualizationHook(draw=True, interval=1, visualizer=vis).after_val_iter(0, None, [s])
    assert np.array_equal(np.asarray(Image.open(file)), D.panel(other, PALETTE19, gt, pred))
    with pytest.raises(ValueError, match="source pictures"):
        s2f.SegVisualizationHook(draw=True, interval=1, visualizer=vis, source=lambda b, o: []).after_val_iter(0, None, [s])


# ------------------------------------------------------------------------------------------------ 6. evaluate(..., hooks=)
class StubModel(torch.nn.Module):
    def __init__(self, preds):
        super().__init__()
        self.preds = preds

    def test_step(self, batch):
        i = batch["index"]
        return [dict(pred_sem_seg=dict(data=torch.from_numpy(self.preds[i])[None]), gt_sem_seg=dict(data=torch.from_numpy(batch["gt"])[None]),
                     img_path=f"{i}.png")]


def test_evaluate_calls_the_hooks_with_rank_local_indices():
    import spike2former_amd as s2f
    K = 5
    rng = np.random.default_rng(7)
    preds = [rng.integers(0, K, (4, 6)).astype(np.int64) for _ in range(6)]
    batches = [dict(index=i, gt=rng.integers(0, K, (4, 6)).astype(np.uint8)) for i in range(6)]

    class Seen:
        def __init__(self):
            self.calls = []

        def after_test_iter(self, batch_idx, data_batch=None, outputs=None):
            self.calls.append((batch_idx, data_batch["index"], outputs[0]["img_path"]))

    def metric():
        m = s2f.IoUMetric()
        m.dataset_meta = dict(classes=[str(i) for i in range(K)])
        return m
    plain = s2f.evaluate(StubModel(preds), batches, metric())
    h = Seen()
    assert s2f.evaluate(StubModel(preds), batches, metric(), hooks=[h]) == plain
    assert h.calls == [(i, i, f"{i}.png") for i in range(6)]
    a, b = Seen(), Seen()
    s2f.evaluate(StubModel(preds), batches, metric(), rank=1, world_size=2, hooks=(a, b))
    assert a.calls == b.calls == [(0, 1, "1.png"), (1, 3, "3.png"), (2, 5, "5.png")]
