"""GPU: the bytes s2f_seg_draw writes against tests/draw_ref.py (the numpy restatement of the reference's drawing) on host copies,
and SegVisualizationHook inside evaluate() from decoded pictures to the PNG files.  Byte equality everywhere; STRICT, no fall-back."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draw_ref as D  # noqa: E402

pytestmark = pytest.mark.gpu

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], bgr_to_rgb=True)


def palette(K, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (K, 3), dtype=np.uint8)


def gpu_draw(img, pal, gt=None, pred=None, **kw):
    from spike2former_amd import ops
    assert ops.STRICT
    before = dict(ops.FALLBACKS)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out = ops.seg_draw(t(img), t(pal), t(gt), t(pred), **kw)
    assert out.is_cuda and dict(ops.FALLBACKS) == before
    return out.cpu().numpy()


def differing(got, want):
    return f"{int((got != want).sum())} of {want.size} bytes differ"


# ------------------------------------------------------------------------------------------------ 1. the arithmetic
@pytest.mark.parametrize("alpha", D.ALPHAS)
def test_every_value_pair(alpha):
    """every (v, c) pair in every channel: a kernel that fuses a product into the sum misses hundreds of them (test_visualizer.py)"""
    img, sem, pal = D.arithmetic_fixture()
    got, want = gpu_draw(img, pal, pred=sem, alpha=alpha), D.panel(img, pal, pred=sem, alpha=alpha)
    assert np.array_equal(got, want), differing(got, want)


# ------------------------------------------------------------------------------------------------ 2. ragged and unaligned
# the issue's sizes; then a row of more than one 256-pixel piece (with a ragged last one) and more pieces than workgroups (2048)
@pytest.mark.parametrize("h0,w0", [(1, 1), (1, 5), (3, 7), (5, 13), (2, 64), (17, 129), (2, 257), (3, 600), (2100, 3)])
def test_ragged_and_unaligned(h0, w0):
    """two pictures (and their uint8 annotations) back to back in ONE byte buffer, so the second starts at byte 3 h0 w0 (h0 w0); both
    panels into a slice at byte offset 1 (2, 3) of a buffer of 0xA5: the bytes in front of and behind the panel stay 0xA5"""
    from spike2former_amd import ops
    rng = np.random.default_rng(h0 * 1000 + w0)
    K, n = 19, h0 * w0
    pal = palette(K)
    imgs = rng.integers(0, 256, (2, h0, w0, 3), dtype=np.uint8)
    gts = rng.integers(0, K + 3, (2, h0, w0)).astype(np.uint8)
    preds = rng.integers(0, K + 1, (2, h0, w0)).astype(np.int64)
    data = torch.from_numpy(np.concatenate([imgs.reshape(-1), gts.reshape(-1)])).cuda()
    pal_d, preds_d = torch.from_numpy(pal).cuda(), torch.from_numpy(preds).cuda()
    for b in range(2):
        want = D.panel(imgs[b], pal, gts[b], preds[b], bgr=True, rzl=True)
        for off in (1, 2, 3):
            big = torch.full((off + 6 * n + 7,), 0xA5, dtype=torch.uint8, device="cuda")
            out = big[off:off + 6 * n].view(h0, 2 * w0, 3)
            image = data[3 * n * b:3 * n * (b + 1)].view(h0, w0, 3)
            gt = data[6 * n + n * b:6 * n + n * (b + 1)].view(h0, w0)
            assert ops.seg_draw(image, pal_d, gt, preds_d[b], bgr=True, reduce_zero_label=True, out=out) is out
            host = big.cpu().numpy()
            assert (host[:off] == 0xA5).all() and (host[off + 6 * n:] == 0xA5).all(), "bytes outside the panel were written"
            got = host[off:off + 6 * n].reshape(h0, 2 * w0, 3)
            assert np.array_equal(got, want), (b, off, differing(got, want))


# ------------------------------------------------------------------------------------------------ 3. values off the classes
def test_values_off_the_classes():
    K = 19
    pal = palette(K)
    img = np.random.default_rng(3).integers(0, 256, (3, 7, 3), dtype=np.uint8)
    gt = np.resize(np.array([0, K - 1, K, 254, 255], np.uint8), (3, 7))
    ints = np.resize(np.array([-1, K, 2 ** 31 + 3, 2 ** 40 + 3, np.iinfo(np.int64).min, 3], np.int64), (3, 7))
    floats = np.resize(np.array([0.0, -0.0, 1.0, 0.5, np.nan, np.inf, 1e10], np.float32), (3, 7))
    for rzl in (False, True):
        for pred in (ints, floats):
            got, want = gpu_draw(img, pal, gt, pred, reduce_zero_label=rzl), D.panel(img, pal, gt, pred, rzl=rzl)
            assert np.array_equal(got, want), (rzl, pred.dtype, differing(got, want))
    # 2^40 + 3 is not class 3, and a negative label paints nothing (the stated deviation): the picture times 1 - alpha alone
    bare = (img * (1 - 0.8)).astype(np.uint8)
    got = gpu_draw(img, pal, pred=ints)
    nothing = ints != 3
    assert np.array_equal(got[nothing], bare[nothing]) and not np.array_equal(got[~nothing], bare[~nothing])


# ------------------------------------------------------------------------------------------------ 4. class counts
@pytest.mark.parametrize("K", [1, 19, 150, 171, 256, 300, 2048])
def test_class_counts(K):
    """labels spanning [0, K) (and K itself, no class), as the int64 maps of an arg-max and as int64 ground truth"""
    h, w = 33, 70          # 2310 pixels: every class of 2048 occurs
    pal = palette(K, seed=K)
    img = np.random.default_rng(K).integers(0, 256, (h, w, 3), dtype=np.uint8)
    pred = (np.arange(h * w, dtype=np.int64) % (K + 1)).reshape(h, w)
    gt = pred[::-1].copy()
    got, want = gpu_draw(img, pal, gt, pred), D.panel(img, pal, gt, pred)
    assert np.array_equal(got, want), differing(got, want)


# ------------------------------------------------------------------------------------------------ 5. panel choice
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("which", ["gt", "pred", "both"])
@pytest.mark.parametrize("gt_dtype,pred_dtype", [(np.uint8, np.int64), (np.int64, np.float32)])
def test_panel_choice(which, bgr, gt_dtype, pred_dtype):
    K = 19
    rng = np.random.default_rng(5)
    pal, img = palette(K), rng.integers(0, 256, (11, 23, 3), dtype=np.uint8)
    gt = rng.integers(0, K + 2, (11, 23)).astype(gt_dtype) if which != "pred" else None
    pred = rng.integers(0, K + 1, (11, 23)).astype(pred_dtype) if which != "gt" else None
    got, want = gpu_draw(img, pal, gt, pred, bgr=bgr, alpha=0.6), D.panel(img, pal, gt, pred, alpha=0.6, bgr=bgr)
    assert got.shape == (11, 23 * (2 if which == "both" else 1), 3) and np.array_equal(got, want), differing(got, want)


# ------------------------------------------------------------------------------------------------ 6. end to end
class KeepPredictions:
    """a hook in front of the visualisation hook: the host copy of every sample's pred_sem_seg"""

    def __init__(self):
        self.preds = []

    def after_test_iter(self, batch_idx, data_batch=None, outputs=None):
        self.preds += [o.pred_sem_seg.data.cpu().numpy() for o in outputs]


@pytest.fixture(scope="module")
def tiny_model():
    import spike2former_amd as s2f
    from spike2former_amd.init_utils import seeded_init
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C1_64"))).cuda().eval()
    return s2f, model, s2f.WORKLOADS["C1_64"]["K"]


def same_metrics(a, b):
    return list(a) == list(b) and np.array_equal(np.array(list(a.values()), float), np.array(list(b.values()), float), equal_nan=True)


@pytest.mark.parametrize("tta", [False, True])
def test_from_decoded_pictures_to_the_files(tiny_model, tmp_path, tta):
    """four random pictures of an odd size with raw annotations through TestAugment, evaluate() with IoUMetric and the hook at
    interval 2 drawing from the staged pictures: exactly two PNG files, each draw_ref of (picture, raw annotation, that sample's
    pred_sem_seg), and the metric dictionary of the same run without the hook; once plain, once through SegTTAModel with a
    two-scale, two-flip tta_pipeline"""
    from spike2former_amd import ops
    from spike2former_amd.augment import TestAugment
    from PIL import Image
    s2f, model, K = tiny_model
    # sizes whose views are sizes the any-size tests run the model at: 37 x 53 -> 40 x 57; 33 x 49 x (2.0, 1.5) -> 66 x 98, 50 x 74
    h0, w0 = (33, 49) if tta else (37, 53)
    rng = np.random.default_rng(11)
    pictures = [(rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8), rng.integers(0, K + 1, (h0, w0)).astype(np.uint8), f"pics/img{i}.png")
                for i in range(4)]
    for _, seg, _ in pictures:
        seg[:2, :9] = 255
    pre = dict(type="SegDataPreProcessor", pad_val=0, seg_pad_val=255, **NORM)
    if tta:
        pipeline = [dict(type="LoadImageFromFile"),
                    dict(type="TestTimeAug", transforms=[[dict(type="Resize", scale_factor=r, keep_ratio=True) for r in (2.0, 1.5)],
                                                         [dict(type="RandomFlip", prob=0., direction="horizontal"),
                                                          dict(type="RandomFlip", prob=1., direction="horizontal")],
                                                         [dict(type="LoadAnnotations")], [dict(type="PackSegInputs")]])]
        runner = s2f.SegTTAModel(model)
    else:
        pipeline = [dict(type="LoadImageFromFile"), dict(type="Resize", scale=(96, 40), keep_ratio=True),
                    dict(type="LoadAnnotations", reduce_zero_label=True), dict(type="PackSegInputs")]
        runner = model
    aug = TestAugment.from_cfg(pipeline, pre, reduce_zero_label=True, max_source_pixels=64 * 64)
    with pytest.raises(RuntimeError):
        aug.sources()
    pal = palette(K, seed=2)

    def metric():
        m = s2f.IoUMetric(label_reduce_zero=aug.reduce_zero_label)
        m.dataset_meta = dict(classes=[str(i) for i in range(K)])
        return m
    batches = lambda: (aug([img], [seg], [path]) for img, seg, path in pictures)  # noqa: E731
    vis = s2f.SegLocalVisualizer(save_dir=str(tmp_path), classes=[str(i) for i in range(K)], palette=pal.tolist())
    keep = KeepPredictions()
    before = dict(ops.FALLBACKS)
    assert ops.STRICT
    with_hook = s2f.evaluate(runner, batches(), metric(),
                             hooks=[keep, s2f.SegVisualizationHook(draw=True, interval=2, visualizer=vis, source=aug)])
    src = aug.sources()
    assert src.is_cuda and src.is_bgr is True and tuple(src.shape) == (1, h0, w0, 3) and np.array_equal(src[0].cpu().numpy(), pictures[3][0])
    assert dict(ops.FALLBACKS) == before
    assert same_metrics(with_hook, s2f.evaluate(runner, batches(), metric())) and "mIoU" in with_hook
    assert sorted(os.listdir(tmp_path / "vis_image")) == ["test_img1.png_0.png", "test_img3.png_0.png"]
    assert len(keep.preds) == 4
    for i in (1, 3):
        img, seg, _ = pictures[i]
        want = D.panel(img, pal, seg, keep.preds[i], bgr=True, rzl=True)
        got = np.asarray(Image.open(tmp_path / "vis_image" / f"test_img{i}.png_0.png"))
        assert got.shape == (h0, 2 * w0, 3) and np.array_equal(got, want), (i, differing(got, want))
