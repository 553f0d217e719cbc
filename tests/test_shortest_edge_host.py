"""CPU: the second resize rule of the training augmentation (spike2former_amd/augment.py) -- RandomChoiceResize over mmseg's
ResizeShortestEdge, the `train_pipeline` the ADE20K, Cityscapes and COCO-Stuff MaskFormer configs set for themselves: the two-step
rounding of the size, the uniform choice among the scales on the variate the ratio used to take, the configuration reader on the six
pipelines (tests/golden/train_pipelines.json: settings only, typed from the configs with `scales` evaluated), and that the
RandomResize mode draws what it drew.  Every comparison is exact."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_ref as R  # noqa: E402
from test_augment_host import ADE_PIPELINE, make, preprocessor  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "train_pipelines.json")) as f:
    PIPELINES = json.load(f)

# (h0, w0), scale, max_size, ResizeShortestEdge._get_output_shape's (new_w, new_h), the picture's (H, W) after the keep-ratio Resize
# to that scale.  Rows 1 and 2: the long edge ends ONE SHORT of max_size (2559, 59) -- the second rounding
TABLE = [
    ((256, 1000), 1280, 2560, (2560, 655), (655, 2559)),
    ((17, 28), 48, 60, (60, 36), (36, 59)),
    ((37, 53), 48, 60, (60, 42), (42, 60)),
    ((53, 37), 48, 60, (42, 60), (60, 42)),
    ((20, 27), 33, 1000, (45, 33), (33, 45)),
    ((64, 96), 12, 1000, (18, 12), (12, 18)),
    ((512, 683), 320, 2560, (427, 320), (320, 427)),
    ((512, 683), 1280, 2560, (1708, 1280), (1280, 1708)),
    ((683, 512), 704, 2560, (704, 939), (939, 704)),
    ((375, 500), 1216, 2560, (1621, 1216), (1216, 1621)),
    ((480, 640), 563, 600, (600, 450), (450, 600)),
    ((1024, 2048), 2048, 4096, (4096, 2048), (2048, 4096)),
    ((1024, 2048), 1126, 4096, (2252, 1126), (1126, 2252)),
]
ADE_SCALES = [320, 384, 448, 512, 576, 640, 704, 768, 832, 896, 960, 1024, 1088, 1152, 1216, 1280]
CITY_SCALES = [512, 614, 716, 819, 921, 1024, 1126, 1228, 1331, 1433, 1536, 1638, 1740, 1843, 1945, 2048]


class FixedVariates:
    """in place of TrainAugment.rng: `random(n)` hands out the chosen vectors, one per picture"""

    def __init__(self, *vectors):
        self.vectors = [np.asarray(v, np.float64) for v in vectors]

    def random(self, n):
        v = self.vectors.pop(0)
        assert v.shape == (n,)
        return v


def variates(u0, seed=0):
    from spike2former_amd.augment import VARIATES_PER_IMAGE
    u = np.random.default_rng(seed).random(VARIATES_PER_IMAGE)
    u[0] = u0
    return u


# ------------------------------------------------------------------------------------------------ 1. the size
@pytest.mark.parametrize("shape, scale, max_size, want_scale, want_size", TABLE)
def test_two_step_rounding_known_answers(shape, scale, max_size, want_scale, want_size):
    from spike2former_amd.augment import shortest_edge_scale, shortest_edge_size
    assert shortest_edge_scale(*shape, scale, max_size) == want_scale
    assert shortest_edge_size(*shape, scale, max_size) == want_size
    assert all(type(v) is int for v in shortest_edge_scale(*shape, scale, max_size) + shortest_edge_size(*shape, scale, max_size))


def test_the_cases_of_the_references_own_transform_test():
    from spike2former_amd.augment import shortest_edge_size
    assert shortest_edge_size(288, 512, (128, 256), 1333)[0] == 128          # a tuple scale takes its minimum
    assert shortest_edge_size(288, 512, 512, 512) == (288, 512)              # the cap holds the picture at its own size
    aug = make(device="cpu", scale=None, scales=[512], max_size=512, rank=0)
    assert tuple(int(aug.draw([(288, 512)])[0][k]) for k in ("H", "W")) == (288, 512)
    aug = make(device="cpu", scale=None, scales=[128, 256, 512], max_size=1333, seed=2, rank=0)
    heights = {int(p["H"]) for p in aug.draw([(288, 512)] * 40)}
    assert heights <= {128, 256, 512} and len(heights) > 1


# ------------------------------------------------------------------------------------------------ 2. the six configs
@pytest.mark.parametrize("name", sorted(PIPELINES))
def test_from_cfg_reads_the_maskformer_configs(name):
    from spike2former_amd.augment import TrainAugment
    e = PIPELINES[name]
    crop = tuple(e["crop_size"])
    city = crop == (512, 1024)
    assert crop in ((512, 512), (512, 1024)) and city == ("ityscapes" in name.lower())
    aug = TrainAugment.from_cfg(e["train_pipeline"], preprocessor(crop), batch_size=2, seed=1, rank=0)
    assert aug.crop_size == crop and aug.scale is None and aug.resize_type == "ResizeShortestEdge"
    assert list(aug.scales) == (CITY_SCALES if city else ADE_SCALES) and len(aug.scales) == 16
    assert aug.max_size == (4096 if city else 2560)
    assert aug.cat_max_ratio == 0.75 and aug.flip_prob == 0.5 and aug.ignore_index == 255
    assert aug.reduce_zero_label is e["reduce_zero_label"]
    assert aug.photometric == dict(brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18)
    assert aug.mean == [123.675, 116.28, 103.53] and aug.std == [58.395, 57.12, 57.375] and aug.bgr_to_rgb is True
    assert aug.pad_val == 0 and aug.seg_pad_val == 255
    shape = (1024, 2048) if city else (512, 683)
    p = aug.draw([shape])[0]
    assert (int(p["H"]), int(p["W"])) in {R_size(shape, s, aug.max_size) for s in aug.scales}


def R_size(shape, scale, max_size):
    from spike2former_amd.augment import shortest_edge_size
    return shortest_edge_size(*shape, scale, max_size)


def test_the_fixture_holds_the_six_configs():
    assert sorted(PIPELINES) == sorted([
        "SDTv2_maskformer_DCNpixelDecoder_ade20k.py", "SDTv3_b_Spike2former_ade20k_512x512.py",
        "SDTv2_maskformer_DCNPixelDecoder_CityScapes.py", "SDTv3_b_Spike2former_Cityscapes_512x1024.py",
        "SDTv2_maskformer_cocostuff10k_512x512.py", "SDTv2_maskformer_cocostuff164k_512x512.py"])
    assert {n: e["reduce_zero_label"] for n, e in PIPELINES.items() if e["reduce_zero_label"]}.keys() == {
        "SDTv2_maskformer_DCNpixelDecoder_ade20k.py", "SDTv3_b_Spike2former_ade20k_512x512.py",
        "SDTv2_maskformer_cocostuff10k_512x512.py"}


def test_a_stand_alone_resize_shortest_edge_is_one_scale():
    from spike2former_amd.augment import TrainAugment
    pipe = [dict(t) for t in ADE_PIPELINE]
    pipe[2] = dict(type="ResizeShortestEdge", scale=1280, max_size=2560)
    aug = TrainAugment.from_cfg(pipe, preprocessor((512, 512)), rank=0)
    assert aug.scales == (1280,) and aug.max_size == 2560 and aug.scale is None and aug.resize_type == "ResizeShortestEdge"
    p = aug.draw([(256, 1000)])[0]
    assert (int(p["H"]), int(p["W"])) == (655, 2559)


# ------------------------------------------------------------------------------------------------ 3. the choice
def test_the_first_variate_picks_the_scale_and_the_later_ones_stay():
    from spike2former_amd.augment import shortest_edge_size
    shape, crop = (375, 500), (512, 512)
    u0s = [(k + 0.5) / 16 for k in range(16)] + [0.0, float(np.nextafter(1, 0))]
    picks = list(range(16)) + [0, 15]
    aug = make(device="cpu", scale=None, scales=ADE_SCALES, max_size=2560, crop_size=crop, rank=0)
    for i, (u0, k) in enumerate(zip(u0s, picks)):
        u = variates(u0, seed=i)
        aug.rng = FixedVariates(u)
        p = aug.draw([shape])[0]
        H, W = shortest_edge_size(*shape, ADE_SCALES[k], 2560)
        assert (int(p["H"]), int(p["W"])) == (H, W), (u0, k)
        my, mx = max(H - crop[0], 0), max(W - crop[1], 0)
        assert (my, mx) == R.margins(H, W, crop)
        assert 0 <= p["crop_y"].min() and p["crop_y"].max() <= my and 0 <= p["crop_x"].min() and p["crop_x"].max() <= mx
        # a RandomResize object brought to the same (H, W) -- scale (W, H) at ratio 1, whatever u[0] is -- and given the same
        # vector draws the same origins, flip and photometric values: no later variate moved
        old = make(device="cpu", scale=(max(H, W), min(H, W)), ratio_range=None, crop_size=crop, rank=0)
        old.rng = FixedVariates(u)
        q = old.draw([shape])[0]
        assert (int(q["H"]), int(q["W"])) == (H, W)
        assert p.tobytes() == q.tobytes(), (u0, k)
    assert len({ADE_SCALES[k] for k in picks}) == 16


def test_the_generator_advances_as_in_the_other_mode():
    from spike2former_amd.augment import VARIATES_PER_IMAGE
    shapes = [(512, 683), (375, 500), (37, 53)]
    aug = make(device="cpu", scale=None, scales=ADE_SCALES, max_size=2560, seed=5, rank=0)
    aug.draw(shapes)
    ref = np.random.default_rng(np.random.SeedSequence([5, 0]))
    ref.random(len(shapes) * VARIATES_PER_IMAGE)
    assert np.array_equal(aug.rng.random(4), ref.random(4))


# ------------------------------------------------------------------------------------------------ 4. the old mode
@pytest.mark.parametrize("kw", [dict(), dict(scale=(2048, 1024), crop_size=(512, 1024)), dict(scale=(96, 48), crop_size=(32, 32)),
                                dict(ratio_range=None), dict(scale=None)])
def test_random_resize_mode_draws_what_it_drew(kw):
    """seed 0 / rank 0, three shapes: byte-identical to a table whose (H, W) and origins come from today's formula written out
    here -- the keep-ratio rescale to (int(s0 r), int(s1 r)) at r = u[0] (hi - lo) + lo -- on the same stream"""
    from spike2former_amd.augment import CANDIDATES, PARAM_DTYPE, VARIATES_PER_IMAGE
    shapes = [(512, 683), (37, 53), (1024, 2048)]
    aug = make(device="cpu", seed=0, rank=0, **kw)
    got = aug.draw(shapes)
    want = np.zeros(len(shapes), PARAM_DTYPE)
    rng = np.random.default_rng(np.random.SeedSequence([0, 0]))

    def pick(u, n):
        return min(int(u * n), n - 1)

    scale, crop = kw.get("scale", (2048, 512)), kw.get("crop_size", (512, 512))
    lo, hi = kw.get("ratio_range", (0.5, 2.0)) or (1.0, 1.0)
    for p, (h0, w0) in zip(want, shapes):
        u = rng.random(VARIATES_PER_IMAGE)
        if scale is None:
            H, W = h0, w0
        else:
            r = u[0] * (hi - lo) + lo
            s = (int(scale[0] * r), int(scale[1] * r))
            f = min(max(s) / max(h0, w0), min(s) / min(h0, w0))
            H, W = int(h0 * f + 0.5), int(w0 * f + 0.5)
            assert (H, W) == R.resized_size(h0, w0, scale, r)
        p["h0"], p["w0"], p["H"], p["W"] = h0, w0, H, W
        for c in range(CANDIDATES):
            p["crop_y"][c] = pick(u[1 + 2 * c], max(H - crop[0], 0) + 1)
            p["crop_x"][c] = pick(u[2 + 2 * c], max(W - crop[1], 0) + 1)
        v = u[1 + 2 * CANDIDATES:]
        p["flip"] = int(v[0] < 0.5)
        p["bright_on"], p["bright_beta"] = pick(v[1], 2), (2 * v[2] - 1) * 32
        p["mode"] = pick(v[3], 2)
        p["contrast_on"], p["contrast_alpha"] = pick(v[4], 2), 0.5 + v[5] * (1.5 - 0.5)
        p["sat_on"], p["sat_alpha"] = pick(v[6], 2), 0.5 + v[7] * (1.5 - 0.5)
        p["hue_on"], p["hue_delta"] = pick(v[8], 2), -18 + pick(v[9], 36)
    assert got.tobytes() == want.tobytes()
    assert aug.scales is None and aug.max_size is None


# ------------------------------------------------------------------------------------------------ 5. the refusals
def test_constructor_refusals():
    with pytest.raises(ValueError, match="scale=None"):
        make(device="cpu", scales=[320], max_size=2560)                          # the default scale=(2048, 512) is still there
    with pytest.raises(ValueError, match="resize_type 'RandomResize'"):
        make(device="cpu", scale=None, scales=[320], max_size=2560, resize_type="RandomResize")
    with pytest.raises(ValueError, match="max_size"):
        make(device="cpu", scale=None, scales=[320])
    with pytest.raises(ValueError, match="max_size"):
        make(device="cpu", scale=None, scales=[320], max_size=0)
    with pytest.raises(ValueError, match="max_size"):
        make(device="cpu", scale=None, scales=[320], max_size=2560.0)
    with pytest.raises(ValueError, match="non-empty"):
        make(device="cpu", scale=None, scales=[], max_size=2560)
    for bad in (0, -3, 1.5, (320,), (320, 0), "320", True):
        with pytest.raises(ValueError, match="scales holds"):
            make(device="cpu", scale=None, scales=[320, bad], max_size=2560)
    with pytest.raises(ValueError, match="2-tuples"):
        make(device="cpu", scale=None, scales=[(96, 40), 64], resize_type="Resize")
    with pytest.raises(ValueError, match="max_size"):
        make(device="cpu", scale=None, scales=[(96, 40)], resize_type="Resize", max_size=100)


def replaced(slot, *transforms):
    return ADE_PIPELINE[:slot] + list(transforms) + ADE_PIPELINE[slot + 1:]


def test_from_cfg_refusals():
    from spike2former_amd.augment import TrainAugment
    pre = preprocessor((512, 512))
    choice = dict(type="RandomChoiceResize", scales=ADE_SCALES, resize_type="ResizeShortestEdge", max_size=2560)
    edge = dict(type="ResizeShortestEdge", scale=640, max_size=2560)

    def refused(pipeline, match):
        with pytest.raises(NotImplementedError, match=match):
            TrainAugment.from_cfg(pipeline, pre)

    TrainAugment.from_cfg(replaced(2, choice), pre)
    TrainAugment.from_cfg(replaced(2, edge), pre)
    # two resize transforms in one list, whichever two
    refused(replaced(2, ADE_PIPELINE[2], choice), "RandomChoiceResize after RandomResize")
    refused(replaced(2, choice, ADE_PIPELINE[2]), "RandomResize after RandomChoiceResize")
    refused(replaced(2, choice, edge), "ResizeShortestEdge after RandomChoiceResize")
    refused(replaced(2, choice, choice), "RandomChoiceResize after RandomChoiceResize")
    # out of order
    refused(ADE_PIPELINE[:2] + [ADE_PIPELINE[3], choice] + ADE_PIPELINE[4:], "RandomChoiceResize after RandomCrop")
    refused(ADE_PIPELINE[:2] + [ADE_PIPELINE[3], edge] + ADE_PIPELINE[4:], "ResizeShortestEdge after RandomCrop")
    # options
    refused(replaced(2, dict(choice, interpolation="bicubic")), "RandomChoiceResize option.*interpolation")
    refused(replaced(2, dict(edge, interpolation="bicubic")), "ResizeShortestEdge option.*interpolation")
    refused(replaced(2, {k: v for k, v in choice.items() if k != "scales"}), "RandomChoiceResize needs scales")
    refused(replaced(2, dict(choice, scales=[])), "RandomChoiceResize needs scales")
    refused(replaced(2, {k: v for k, v in choice.items() if k != "max_size"}), "RandomChoiceResize.*ResizeShortestEdge.*max_size")
    refused(replaced(2, dict(choice, keep_ratio=True)), "RandomChoiceResize.*ResizeShortestEdge.*keep_ratio")
    refused(replaced(2, {k: v for k, v in edge.items() if k != "max_size"}), "ResizeShortestEdge needs scale and max_size")
    refused(replaced(2, {k: v for k, v in edge.items() if k != "scale"}), "ResizeShortestEdge needs scale and max_size")
    refused(replaced(2, dict(choice, resize_type="RandomResize")), "RandomChoiceResize resize_type='RandomResize'")
    pairs = dict(type="RandomChoiceResize", scales=[(2048, 512), (1024, 512)])
    TrainAugment.from_cfg(replaced(2, dict(pairs, keep_ratio=True)), pre)
    refused(replaced(2, pairs), "RandomChoiceResize.*keep_ratio")                          # Resize's own default is False
    refused(replaced(2, dict(pairs, keep_ratio=False)), "RandomChoiceResize.*keep_ratio")
    refused(replaced(2, dict(pairs, keep_ratio=True, max_size=2560)), "RandomChoiceResize.*max_size")


# ------------------------------------------------------------------------------------------------ 6. resize_type="Resize"
def test_choice_among_keep_ratio_resizes():
    from spike2former_amd.augment import TrainAugment, resized_size
    scales = [(96, 40), (64, 64)]
    aug = make(device="cpu", scale=None, scales=scales, resize_type="Resize", crop_size=(32, 32), rank=0)
    assert aug.max_size is None and aug.scales == ((96, 40), (64, 64))
    for shape in ((37, 53), (64, 48), (50, 50)):
        for u0, k in ((0.0, 0), (0.49, 0), (0.5, 1), (0.99, 1)):
            aug.rng = FixedVariates(variates(u0))
            p = aug.draw([shape])[0]
            assert (int(p["H"]), int(p["W"])) == resized_size(*shape, scales[k], 1.0) == R.resized_size(*shape, scales[k], 1.0)
    pipe = replaced(2, dict(type="RandomChoiceResize", scales=[list(s) for s in scales], keep_ratio=True))
    cfg = TrainAugment.from_cfg(pipe, preprocessor((512, 512)), rank=0)
    assert cfg.scales == aug.scales and cfg.resize_type == "Resize" and cfg.max_size is None and cfg.scale is None
