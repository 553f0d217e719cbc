"""GPU: FiringMaps on the tiny configuration C1_64 (64 x 64, T = 2, seeded, eval) -- the maps of every neuron against the firing
counters of FiringRecorder on the same pass (equality of integers), the package untouched once the hooks are gone (bit equality, a
new capture), and FiringMapHook inside evaluate() from decoded pictures to the PNG files (byte equality against tests/firingmap_ref.py
on the read-back planes).  STRICT, no fall-back."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import firingmap_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], bgr_to_rgb=True)


@pytest.fixture(scope="module")
def tiny_model():
    import spike2former_amd as s2f
    from spike2former_amd.init_utils import seeded_init
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C1_64"))).cuda().eval()
    return s2f, model, s2f.WORKLOADS["C1_64"]


def pictures(seed, B, H, W):
    """16 x a standard normal picture (tests/test_gpu_graphed_predict.py: at unit amplitude the seeded model's logits do not depend on
    the picture); every image of the batch differs"""
    return (16.0 * torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed))).cuda()


def hooked(model):
    return sum(len(m._forward_hooks) + len(m._forward_pre_hooks) for m in model.modules())


def logits_of(model, x):
    import spike2former_amd as s2f
    with torch.no_grad():
        s2f.reset_net(model)
        return model(x, mode="logits").clone()


def test_maps_against_the_firing_counters(tiny_model):
    from spike2former_amd import ops
    s2f, model, w = tiny_model
    T, B, H, W = w["T"], 2, w["H"], w["W"]
    x = pictures(3, B, H, W)
    model.test_cfg = dict(mode="whole")
    model.__dict__.pop("_graphed_predict", None)
    before = logits_of(model, x)
    assert not torch.equal(before[0], before[1])
    assert hooked(model) == 0
    with torch.no_grad():
        with s2f.FiringMaps(model) as maps:
            assert hooked(model) == len(maps.nodes) + 1
            s2f.reset_net(model)
            samples = model.test_step(dict(inputs=x))
            assert len(samples) == B
            read = maps.read()
            # the same pass again under FiringRecorder, the maps detached
            maps.detach()
            assert hooked(model) == 0
            with s2f.FiringRecorder(model) as rec:
                s2f.reset_net(model)
                model.test_step(dict(inputs=x))
                words = {n: ops.read_stats(m.stats).cpu().numpy() for n, m in rec.nodes.items()}
                elems = {n: int(m.stats_elems) for n, m in rec.nodes.items()}
            maps.attach()
        assert hooked(model) == 0
    # every neuron the pass ran has a map or a reason; the others (a module this configuration never calls) counted nothing either
    assert len(read.names) >= 10 and not set(read.names) & set(maps.skipped)
    assert all(elems.get(n, 0) == 0 for n in set(maps.nodes) - set(read.names) - set(maps.skipped))
    assert all(elems.get(n, 1) > 0 for n in list(read.names) + list(maps.skipped))
    strides = set()
    for n in read.names:
        planes = read.planes[n].astype(np.int64)
        Tn, C, D, passes = read.meta[n]
        h, wd = planes.shape[2:]
        assert Tn == T and planes.shape[:2] == (B, 4)
        assert int(planes[:, 0].sum()) == int(words[n][0]), n          # the sum-of-counts word
        assert int(planes[:, 1].sum()) == int(words[n][1]), n          # the non-zero word
        assert read.off_grid(n) == 0, n
        assert passes * (T * B * C * h * wd) == elems[n], n          # passes = the neuron's calls
        assert planes[:, 2].max() <= D and (planes[:, 0] <= T * C * D * passes).all()
        assert H % h == 0 and (H // h, W // wd) == (H // h,) * 2 and (H // h) & (H // h - 1) == 0, n
        if n.startswith("backbone."):
            strides.add(H // h)
        rate = read.rate(n)
        assert rate.shape == (B, h, wd) and 0.0 <= rate.min() and rate.max() <= 1.0
    # the backbone's stages: its four feature maps' strides are all there, and the two pictures fire differently somewhere
    with torch.no_grad():
        s2f.reset_net(model)
        feats = model.extract_feat(x)
    assert {H // f.shape[-2] for f in feats} <= strides, (strides, [tuple(f.shape) for f in feats])
    assert any(not np.array_equal(read.planes[n][0], read.planes[n][1]) for n in read.names)
    assert all(r.startswith(("token-major", "no power-of-two", "rank", "ambiguous", "not contiguous")) for r in maps.skipped.values())
    # after __exit__: bit-identical logits, and GraphedPredict captures again
    assert torch.equal(logits_of(model, x), before)
    model.test_cfg = dict(mode="whole", graph=dict(capture_after=1))
    try:
        with torch.no_grad():
            got = model(x, mode="logits")
            gp = model.graphed_predict()
            assert gp.census["captures"] == 1 and not gp.census["eager"], gp.census
            assert torch.equal(got, before)
            with s2f.FiringMaps(model, layers=r"^backbone\."):
                s2f.reset_net(model)
                model(x, mode="logits")
                assert gp.census["eager"] == {"forward_hooks": 1}
            assert torch.equal(model(x, mode="logits"), before) and gp.census["replays"] == 1
    finally:
        model.test_cfg = dict(mode="whole")
        model.__dict__.pop("_graphed_predict", None)


class Probe:
    """a hook in front of FiringMapHook: how many nn.Module hooks the model carried while this batch ran"""

    def __init__(self, model):
        self.model, self.counts = model, []

    def after_test_iter(self, batch_idx, data_batch=None, outputs=None):
        self.counts.append(hooked(self.model))


def same_metrics(a, b):
    return list(a) == list(b) and np.array_equal(np.array(list(a.values()), float), np.array(list(b.values()), float), equal_nan=True)


def test_hook_from_decoded_pictures_to_the_files(tiny_model, tmp_path):
    """four random 32 x 48 pictures through TestAugment (-> 64 x 96), evaluate() with FiringMapHook at interval 2: exactly two PNG
    files, each the grid of firingmap_ref tiles of the planes the hook read back; two lines of firing_maps.jsonl; batches 0 and 2 ran
    with no hook on any module, batches 1 and 3 with all of them"""
    from spike2former_amd import ops
    from spike2former_amd.augment import TestAugment
    from PIL import Image
    s2f, model, w = tiny_model
    K = w["K"]
    model.test_cfg = dict(mode="whole")
    model.__dict__.pop("_graphed_predict", None)
    h0, w0 = 32, 48
    rng = np.random.default_rng(11)
    pics = [(rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8), rng.integers(0, K + 1, (h0, w0)).astype(np.uint8), f"pics/img{i}.png")
            for i in range(4)]
    pre = dict(type="SegDataPreProcessor", pad_val=0, seg_pad_val=255, **NORM)
    pipeline = [dict(type="LoadImageFromFile"), dict(type="Resize", scale=(96, 64), keep_ratio=True),
                dict(type="LoadAnnotations", reduce_zero_label=True), dict(type="PackSegInputs")]
    aug = TestAugment.from_cfg(pipeline, pre, reduce_zero_label=True, max_source_pixels=64 * 64)

    def metric():
        m = s2f.IoUMetric(label_reduce_zero=aug.reduce_zero_label)
        m.dataset_meta = dict(classes=[str(i) for i in range(K)])
        return m
    batches = lambda: (aug([img], [seg], [path]) for img, seg, path in pics)  # noqa: E731
    vis = s2f.SegLocalVisualizer(save_dir=str(tmp_path))
    maps = s2f.FiringMaps(model, layers=r"^backbone\.")
    reads, inside = [], []
    read_once = maps.read
    maps.read = lambda: (reads.append(read_once()), reads[-1])[1]

    def source(data_batch, outputs):
        inside.append(hooked(model))
        return aug.sources()
    probe = Probe(model)
    assert ops.STRICT
    before = dict(ops.FALLBACKS)
    hook = s2f.FiringMapHook(maps, interval=2, visualizer=vis, source=source)
    assert hooked(model) == 0          # the first batch is not due
    with_hook = s2f.evaluate(model, batches(), metric(), hooks=[probe, hook])
    assert dict(ops.FALLBACKS) == before
    n_hooks = len(maps.nodes) + 1
    assert probe.counts == [0, n_hooks, 0, n_hooks] and inside == [n_hooks, n_hooks] and hooked(model) == 0
    assert same_metrics(with_hook, s2f.evaluate(model, batches(), metric())) and "mIoU" in with_hook
    assert sorted(os.listdir(tmp_path / "vis_image")) == ["test_img1.png_firing_0.png", "test_img3.png_firing_0.png"]
    lines = [json.loads(line) for line in open(tmp_path / "vis_data" / "firing_maps.jsonl")]
    assert [line["batch"] for line in lines] == [1, 3] and len(reads) == 2
    lut = vis.default_firing_lut()
    for k, i in enumerate((1, 3)):
        read = reads[k]
        assert lines[k]["samples"] == [f"test_img{i}.png_firing"] and list(lines[k]["maps"]) == read.names and len(read.names) >= 4
        assert all(read.meta[n][3] >= 1 and read.planes[n].shape[0] == 1 for n in read.names)
        n = len(read.names)
        cols = int(np.ceil(np.sqrt(n)))
        rows = (n + cols - 1) // cols
        want = np.zeros((rows * h0, cols * w0, 3), np.uint8)
        for t, name in enumerate(read.names):
            plane = read.planes[name][0, 0]
            r, c = divmod(t, cols)
            want[r * h0:(r + 1) * h0, c * w0:(c + 1) * w0] = R.firing_draw(pics[i][0], plane, max(1, int(plane.max())), lut, 128, bgr=True)
        got = np.asarray(Image.open(tmp_path / "vis_image" / f"test_img{i}.png_firing_0.png"))
        assert got.shape == want.shape and np.array_equal(got, want), (i, f"{int((got != want).sum())} of {want.size} bytes differ")
    assert any(int(reads[0].planes[n][0, 0].max()) > 0 for n in reads[0].names)          # something fired: the tiles are not bare
    assert not all(np.array_equal(reads[0].planes[n], reads[1].planes[n]) for n in reads[0].names)
