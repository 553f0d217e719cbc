"""The device-side test pipeline (s2f_test_views in csrc/augment.hip through spike2former_amd.augment.TestAugment) against its numpy
restatement tests/view_ref.py.  The views must equal the fp32 restatement BIT FOR BIT: every operation of the chain is one IEEE fp32
operation on both sides.  The whole packed buffer is pre-filled with NaN between `stage` and `launch`: an element of a view the kernel
does not write fails the comparison, and so does an element between the blocks that it does write."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_ref as R  # noqa: E402
import view_ref as VR  # noqa: E402
from test_gpu_augment import RESIZES  # noqa: E402

pytestmark = pytest.mark.gpu

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
RATIOS = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
NORM = dict(mean=MEAN, std=STD, bgr_to_rgb=True)


def make(**kw):
    from spike2former_amd.augment import TestAugment
    return TestAugment(**{**dict(scale=None, max_source_pixels=64 * 128, **NORM), **kw})


def run(aug, images, segs=None, paths=None, views=None):
    """stage, NaN-fill, launch; the coverage rule and every block against the restatement -> (what the call returns, the sizes)"""
    table = aug.stage(images, segs, paths, views)
    aug._out.fill_(float("nan"))
    data = aug.launch()
    buf = aug._out.cpu().numpy()
    inside = np.zeros(buf.size, bool)
    for p in table:
        inside[int(p["out_off"]):int(p["out_off"]) + 3 * int(p["Hp"]) * int(p["Wp"])] = True
    assert not np.isnan(buf[inside]).any(), f"{int(np.isnan(buf[inside]).sum())} elements of the views were not written"
    assert np.isnan(buf[~inside]).all(), f"{int((~np.isnan(buf[~inside])).sum())} elements between the blocks were written"
    B = len(images)
    sizes = [(int(p["H"]), int(p["W"]), int(p["Hp"]), int(p["Wp"]), bool(p["flip"])) for p in table[::B]]
    want = VR.views(images, sizes, mean=aug.mean, std=aug.std, bgr_to_rgb=aug.bgr_to_rgb, pad_val=aug.pad_val)
    got = data["inputs"] if isinstance(data["inputs"], list) else [data["inputs"]]
    assert len(got) == len(want)
    for g, w, s in zip(got, want, sizes):
        assert tuple(g.shape) == w.shape and g.dtype == torch.float32
        differ = g.cpu().numpy() != w
        assert not differ.any(), f"view {s}: {int(differ.sum())} of {differ.size} elements differ from the fp32 restatement"
    return data, sizes


def preprocessor(img, **kw):
    """SegDataPreProcessor's test branch on the same picture (CPU) -> (inputs, the sample's metainfo)"""
    from spike2former_amd.data_preprocessor import SegDataPreProcessor, SegDataSample
    pre = SegDataPreProcessor(**NORM, **kw)
    res = pre(dict(inputs=[torch.from_numpy(img).permute(2, 0, 1).contiguous()], data_samples=[SegDataSample()]), training=False)
    return res["inputs"], res["data_samples"][0].metainfo


# ------------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("src", [(37, 53), (24, 40)])          # scalar stores (odd width) / 16-byte stores
def test_identity_is_the_data_preprocessor(src):
    img, _ = VR.scene(*src, seed=1)
    data, sizes = run(make(), [img])
    assert sizes == [(*src, *src, False)] and data["preprocessed"] is True
    want, _ = preprocessor(img)
    assert torch.equal(data["inputs"].cpu(), want)
    meta = data["data_samples"][0].metainfo
    assert meta["ori_shape"] == meta["img_shape"] == meta["pad_shape"] == src and "img_padding_size" not in meta
    assert meta["flip"] is False and meta["flip_direction"] is None and meta["scale_factor"] == (1.0, 1.0)


# ------------------------------------------------------------------------------------------------ 2. padding
@pytest.mark.parametrize("test_cfg, padded", [(dict(size_divisor=32), (64, 64)), (dict(size=(40, 56)), (40, 56))])
def test_padding_is_the_data_preprocessors(test_cfg, padded):
    img, _ = VR.scene(37, 53, seed=2)
    data, sizes = run(make(**test_cfg), [img])
    assert sizes == [(37, 53, *padded, False)]
    want, want_meta = preprocessor(img, test_cfg=test_cfg)
    assert torch.equal(data["inputs"].cpu(), want)
    meta = data["data_samples"][0].metainfo
    assert meta["img_padding_size"] == want_meta["img_padding_size"] and meta["pad_shape"] == want_meta["pad_shape"] == padded


# ------------------------------------------------------------------------------------------------ 3. resize
@pytest.mark.parametrize("src, size", [(r[0], r[1]) for r in RESIZES])
def test_resize_flip_and_padding(src, size):
    """shrinking, 2x, non-dyadic, mixed, odd widths: un-flipped and flipped, bare and padded to a multiple of 32, in one launch"""
    img, _ = VR.scene(*src, seed=3)
    H, W = size
    Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
    aug = make(scale_factors=(1.0, 1.0), flips=(False, True))          # room for four views
    data, _ = run(aug, [img], views=[(H, W, H, W, False), (H, W, H, W, True), (H, W, Hp, Wp, False), (H, W, Hp, Wp, True)])
    plain, flipped, plain_p, flipped_p = (v[0].cpu() for v in data["inputs"])
    assert torch.equal(flipped, plain.flip(-1))
    assert torch.equal(plain_p[:, :H, :W], plain) and torch.equal(flipped_p[:, :H, :W], flipped)
    for v in (plain_p, flipped_p):          # the padding stays on the right and at the bottom
        assert bool((v[:, H:, :] == 0).all()) and bool((v[:, :, W:] == 0).all())


# ------------------------------------------------------------------------------------------------ 4. twelve views, one launch
@pytest.mark.parametrize("src, widths", [((37, 53), (27, 40, 53, 66, 80, 93)), ((64, 48), (24, 36, 48, 60, 72, 84))])
def test_twelve_views_in_one_launch(src, widths):
    img, seg = VR.scene(*src, seed=4)
    aug = make(scale_factors=RATIOS, flips=(False, True))
    data, sizes = run(aug, [img], [seg], ["a/b.png"])
    assert len(sizes) == 12 and tuple(s[1] for s in sizes[::2]) == widths and [s[4] for s in sizes] == [False, True] * 6
    assert data["preprocessed"] == [True] * 12 and len(data["data_samples"]) == 12
    for s, samples in zip(sizes, data["data_samples"]):
        meta = samples[0].metainfo
        assert (meta["ori_shape"], meta["img_shape"], meta["pad_shape"]) == (src, s[:2], s[2:4])
        assert meta["flip"] is s[4] and meta["flip_direction"] == ("horizontal" if s[4] else None) and meta["img_path"] == "a/b.png"
        assert meta["scale_factor"] == (s[1] / src[1], s[0] / src[0])
        gt = samples[0].gt_sem_seg.data
        assert gt.is_cuda and gt.dtype == torch.uint8 and np.array_equal(gt.cpu().numpy(), seg[None])          # raw, un-flipped


# ------------------------------------------------------------------------------------------------ 5. a batch
def test_batch_of_two_is_one_tensor_per_view():
    pairs = [VR.scene(37, 53, seed=5 + i) for i in range(2)]          # 5 883-byte pictures: the second starts at an odd byte
    images, segs = [p[0] for p in pairs], [p[1] for p in pairs]
    aug = make(scale_factors=(1.0, 0.5), flips=(False, True), size_divisor=32, batch_size=2)
    data, sizes = run(aug, images, segs, ["0.png", "1.png"])
    assert [s[2:4] for s in sizes] == [(64, 64), (64, 64), (32, 32), (32, 32)]
    for v, s in zip(data["inputs"], sizes):
        assert tuple(v.shape) == (2, 3, *s[2:4]) and v.is_contiguous()
    assert not torch.equal(data["inputs"][0][0], data["inputs"][0][1])
    for samples in data["data_samples"]:
        assert [d.metainfo["img_path"] for d in samples] == ["0.png", "1.png"]
        assert all(d.metainfo["img_padding_size"] == (0, d.metainfo["pad_shape"][1] - d.metainfo["img_shape"][1], 0,
                                                      d.metainfo["pad_shape"][0] - d.metainfo["img_shape"][0]) for d in samples)
        for d, seg in zip(samples, segs):
            assert np.array_equal(d.gt_sem_seg.data.cpu().numpy(), seg[None])
    one, _ = run(aug, images[1:], segs[1:])                           # a smaller batch in the same buffers
    assert one["inputs"][0].data_ptr() == data["inputs"][0].data_ptr() and tuple(one["inputs"][0].shape) == (1, 3, 64, 64)


# ------------------------------------------------------------------------------------------------ 6. / 7. end to end
def label_row(seg, K):
    """numpy.bincount of the reduced annotation over the classes: what row 2 of IoUMetric's totals holds"""
    red = R.reduce_zero_label(seg).astype(np.int64).reshape(-1)
    return np.bincount(red[red < K], minlength=K)[:K]


def test_tta_from_decoded_picture_to_the_metric():
    """66 x 98, ratios (1.0, 0.75) x two flips -> views 66 x 98 and 50 x 74 (the sizes test_gpu_any_size.py runs)"""
    from test_gpu_any_size import tiny
    s2f, so, cfg, st, model = tiny()
    from spike2former_amd import ops
    model.eval()
    K = cfg.num_classes
    img, seg = VR.scene(66, 98, seed=6, n_classes=min(6, K))
    aug = make(scale_factors=(1.0, 0.75), flips=(False, True), reduce_zero_label=True)
    data, sizes = run(aug, [img], [seg], ["img0.png"])
    assert [s[:2] for s in sizes] == [(66, 98), (66, 98), (50, 74), (50, 74)]
    tta = s2f.MODELS.build(dict(type="SegTTAModel", module=model))
    before = dict(ops.FALLBACKS)
    assert ops.STRICT
    out = tta.test_step(data)
    assert dict(ops.FALLBACKS) == before
    assert len(out) == 1
    pred = out[0].pred_sem_seg.data
    assert tuple(pred.shape) == (1, 66, 98) and pred.dtype == torch.int64
    assert out[0].metainfo["img_path"] == "img0.png" and np.array_equal(out[0].gt_sem_seg.data.cpu().numpy(), seg[None])
    metric = s2f.metrics.IoUMetric(label_reduce_zero=aug.reduce_zero_label)
    metric.dataset_meta = dict(classes=[str(i) for i in range(K)])
    metric.process(None, out)
    totals = metric._totals.cpu().numpy()
    assert totals.dtype == np.int64 and np.array_equal(totals[2], label_row(seg, K)) and totals[2].sum() > 0
    assert totals[1].sum() == (R.reduce_zero_label(seg) != 255).sum()          # every scored pixel has a prediction among the classes


def test_test_form_through_evaluate():
    """Resize(scale=(96, 40)) on 37 x 53 -> 40 x 57, through model.test_step and evaluate() with a two-picture generator"""
    from test_gpu_any_size import tiny
    s2f, so, cfg, st, model = tiny()
    from spike2former_amd import ops
    from spike2former_amd.augment import TestAugment
    K = cfg.num_classes
    pipeline = [dict(type="LoadImageFromFile"), dict(type="Resize", scale=(96, 40), keep_ratio=True),
                dict(type="LoadAnnotations", reduce_zero_label=True), dict(type="PackSegInputs")]
    aug = TestAugment.from_cfg(pipeline, dict(type="SegDataPreProcessor", pad_val=0, seg_pad_val=255, **NORM), max_source_pixels=64 * 64)
    assert aug.view_sizes(37, 53) == [(40, 57, 40, 57, False)] and aug.tta is False and aug.reduce_zero_label is True
    pictures = [VR.scene(37, 53, seed=7 + i, n_classes=min(6, K)) + (f"{i}.png",) for i in range(2)]
    first, _ = run(aug, [pictures[0][0]], [pictures[0][1]], [pictures[0][2]])
    assert tuple(first["inputs"].shape) == (1, 3, 40, 57) and first["preprocessed"] is True
    metric = s2f.metrics.IoUMetric(label_reduce_zero=aug.reduce_zero_label)
    metric.dataset_meta = dict(classes=[str(i) for i in range(K)])
    seen, compute = {}, metric.compute_metrics

    def keep(totals):
        seen["totals"] = np.asarray(totals).copy()
        return compute(totals)
    metric.compute_metrics = keep
    before = dict(ops.FALLBACKS)
    result = s2f.metrics.evaluate(model, (aug([img], [seg], [path]) for img, seg, path in pictures), metric)
    assert dict(ops.FALLBACKS) == before
    assert "mIoU" in result and "aAcc" in result
    assert np.array_equal(seen["totals"][2], label_row(pictures[0][1], K) + label_row(pictures[1][1], K))
    assert seen["totals"][2].sum() > 0


# ------------------------------------------------------------------------------------------------ 8. graph capture
def test_graph_replays_follow_the_staged_picture():
    """the launch allocates nothing and synchronises nothing: captured once, a replay turns whatever `stage` copied last into the
    views (pictures of one size: the table does not change)"""
    pairs = [VR.scene(37, 53, seed=20 + i) for i in range(3)]
    aug = make(scale_factors=(0.75, 1.25), flips=(False, True), size_divisor=32)
    table = aug.stage([pairs[0][0]])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aug.launch()                                               # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                  # one kernel node
        data = aug.launch()
    sizes = [(int(p["H"]), int(p["W"]), int(p["Hp"]), int(p["Wp"]), bool(p["flip"])) for p in table]
    for img, _ in pairs[::-1]:
        assert aug.stage([img]).tobytes() == table.tobytes()
        aug._out.fill_(float("nan"))
        graph.replay()
        want = VR.views([img], sizes, mean=aug.mean, std=aug.std, bgr_to_rgb=aug.bgr_to_rgb, pad_val=aug.pad_val)
        for g, w in zip(data["inputs"], want):
            assert np.array_equal(g.cpu().numpy(), w)
    del graph


# ------------------------------------------------------------------------------------------------ 9. one sampler, two pipelines
@pytest.mark.parametrize("flip", (False, True))
@pytest.mark.parametrize("src, size, padded", [((37, 53), (29, 41), (40, 56)),          # 16-byte stores with padding
                                               ((37, 53), (29, 41), (29, 41)),          # scalar stores on both sides
                                               ((24, 40), (48, 80), (48, 80)),          # 2x, 16-byte stores
                                               ((64, 48), (23, 90), (32, 96))])         # shrinking rows, enlarging columns
def test_a_view_is_the_training_route_without_its_randomness(src, size, padded, flip):
    """TrainAugment with nothing random left -- no RandomResize draw (the entry names H x W), the crop at (0, 0) and as large as
    the padded view, no crop rule, no photometric distortion -- writes the tensor TestAugment writes for the view (H, W, Hp, Wp,
    flip): both kernels call one sampler and one normalisation.  No tolerance."""
    from spike2former_amd.augment import TrainAugment
    from test_gpu_augment import entry, prefilled
    img, seg = VR.scene(*src, seed=9)
    pre = dict(pad_val=-1.5, max_source_pixels=64 * 128, **NORM)
    train = TrainAugment(scale=None, cat_max_ratio=1.0, photometric=None, crop_size=padded, batch_size=1, seed=0, rank=0, **pre)
    got, _ = train([img], [seg], np.array([entry(train, *src, *size, origins=(0, 0), flip=int(flip))]), out=prefilled(train, 1))
    data, _ = run(make(**pre), [img], views=[(*size, *padded, flip)])
    assert tuple(got.shape) == (1, 3, *padded) and not bool(torch.isnan(got).any())
    assert torch.equal(got, data["inputs"][0])
