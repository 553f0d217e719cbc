"""CPU: the host half of the device-side training augmentation (spike2former_amd/augment.py) and the numpy restatement the GPU tests
compare the kernels with (tests/aug_ref.py): geometry, the 8-bit HSV known answers, the bilinear stage against ATen, the crop rule,
the configuration reader, and the argument errors of the two entry points."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_ref as R  # noqa: E402

ADE_PIPELINE = [
    dict(type="LoadImageFromFile"),
    dict(type="LoadAnnotations", reduce_zero_label=True),
    dict(type="RandomResize", scale=(2048, 512), ratio_range=(0.5, 2.0), keep_ratio=True),
    dict(type="RandomCrop", crop_size=(512, 512), cat_max_ratio=0.75),
    dict(type="RandomFlip", prob=0.5),
    dict(type="PhotoMetricDistortion"),
    dict(type="PackSegInputs"),
]
VOC_PIPELINE = [dict(t) for t in ADE_PIPELINE]
VOC_PIPELINE[1] = dict(type="LoadAnnotations")
CITY_PIPELINE = [dict(t) for t in VOC_PIPELINE]
CITY_PIPELINE[2] = dict(type="RandomResize", scale=(2048, 1024), ratio_range=(0.5, 2.0), keep_ratio=True)
CITY_PIPELINE[3] = dict(type="RandomCrop", crop_size=(512, 1024), cat_max_ratio=0.75)


def preprocessor(size):
    return dict(type="SegDataPreProcessor", mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], bgr_to_rgb=True, pad_val=0,
                seg_pad_val=255, size=size)


def make(**kw):
    from spike2former_amd.augment import TrainAugment
    return TrainAugment(**kw)


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("ratio, want", [(0.5, (256, 342)), (1.0, (512, 683)), (2.0, (1024, 1366))])
def test_resized_size_known_answers(ratio, want):
    from spike2former_amd.augment import resized_size
    assert resized_size(512, 683, (2048, 512), ratio) == want
    assert R.resized_size(512, 683, (2048, 512), ratio) == want


def test_draw_geometry_and_origins_stay_inside_the_margins():
    aug = make(seed=3, rank=0)
    shapes = [(512, 683), (683, 512), (37, 53), (300, 2000), (1024, 2048)] * 8
    params = aug.draw(shapes)
    assert params.dtype.itemsize == 160 and len(params) == len(shapes)
    ratios = []
    for p, (h0, w0) in zip(params, shapes):
        H, W = int(p["H"]), int(p["W"])
        assert (p["h0"], p["w0"]) == (h0, w0)
        # some ratio of the range gives this size, and the size keeps the aspect ratio to within the rounding
        lo, hi = R.resized_size(h0, w0, (2048, 512), 0.5), R.resized_size(h0, w0, (2048, 512), 2.0)
        assert lo[0] <= H <= hi[0] and lo[1] <= W <= hi[1]
        assert abs(H * w0 - W * h0) <= max(h0, w0)
        ratios.append(H / h0)
        my, mx = R.margins(H, W, (512, 512))
        assert p["crop_y"].min() >= 0 and p["crop_y"].max() <= my and p["crop_x"].min() >= 0 and p["crop_x"].max() <= mx
        assert p["flip"] in (0, 1) and p["mode"] in (0, 1) and -18 <= p["hue_delta"] <= 17
        assert -32 <= p["bright_beta"] <= 32 and 0.5 <= p["contrast_alpha"] <= 1.5 and 0.5 <= p["sat_alpha"] <= 1.5
    assert len(set(ratios)) > 10
    assert {int(p["flip"]) for p in params} == {0, 1} and {int(p["hue_on"]) for p in params} == {0, 1}
    big = params[[i for i, s in enumerate(shapes) if s == (1024, 2048)]]          # margins > 0: the origins do move
    assert len({int(v) for v in big["crop_x"].reshape(-1)}) > 20


def test_draw_is_reproducible_per_seed_and_rank():
    shapes = [(512, 683), (375, 500)]
    a, b = make(seed=7, rank=1).draw(shapes), make(seed=7, rank=1).draw(shapes)
    assert a.tobytes() == b.tobytes()
    assert make(seed=7, rank=0).draw(shapes).tobytes() != a.tobytes()
    assert make(seed=8, rank=1).draw(shapes).tobytes() != a.tobytes()


def test_draw_consumes_the_same_number_of_variates_whatever_is_used():
    """the second image's parameters do not depend on what the configuration used of the first image's variates"""
    from spike2former_amd.augment import VARIATES_PER_IMAGE
    shapes = [(512, 683), (375, 500)]
    full = make(seed=5, rank=0)
    bare = make(seed=5, rank=0, photometric=None, flip_prob=0.0, ratio_range=None)
    pf, pb = full.draw(shapes), bare.draw(shapes)
    assert pb["flip"].sum() == 0 and pb["sat_on"].sum() == 0 and pb[0]["H"] == R.resized_size(512, 683, (2048, 512), 1.0)[0]
    # both generators stand at the same place, VARIATES_PER_IMAGE per image behind the seed
    ref = np.random.default_rng(np.random.SeedSequence([5, 0]))
    ref.random(len(shapes) * VARIATES_PER_IMAGE)
    nxt = ref.random(4)
    assert np.array_equal(full.rng.random(4), nxt) and np.array_equal(bare.rng.random(4), nxt)
    # ... and the second image's flip variate was the same one: where both configurations use it, they agree
    assert int(make(seed=5, rank=0, photometric=None, ratio_range=None).draw(shapes)["flip"][1]) == int(pf["flip"][1])


# ------------------------------------------------------------------------------------------------ HSV
def test_hsv_known_answers():
    px = np.array([[0, 0, 255], [0, 255, 0], [255, 0, 0]], np.uint8)
    assert R.bgr2hsv(px).tolist() == [[0, 255, 255], [60, 255, 255], [120, 255, 255]]
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    hsv = R.bgr2hsv(grey)
    assert (hsv[:, 0] == 0).all() and (hsv[:, 1] == 0).all() and np.array_equal(hsv[:, 2], np.arange(256))
    assert np.array_equal(R.hsv2bgr(hsv), grey)
    # the primaries and secondaries survive the round trip; the hue just below 360 degrees wraps to 0
    prim = np.array([[0, 0, 255], [0, 255, 0], [255, 0, 0], [0, 255, 255], [255, 255, 0], [255, 0, 255]], np.uint8)
    assert np.array_equal(R.hsv2bgr(R.bgr2hsv(prim)), prim)
    assert R.bgr2hsv(np.array([[1, 0, 255]], np.uint8))[0, 0] == 0
    # float32 and float64 give the same BGR -> HSV on a sample of colours (the issue's observation for the plain conversion)
    rng = np.random.default_rng(0)
    col = rng.integers(0, 256, (20000, 3), dtype=np.uint8)
    h32, h64 = R.bgr2hsv(col), R.bgr2hsv(col, np.float64)
    assert h32[:, 0].max() <= 179
    print("bgr2hsv fp32 vs fp64: differing colours", int((h32 != h64).any(1).sum()), "of", len(col))


def test_convert_clips_and_truncates():
    v = np.array([0, 1, 100, 200, 255], np.uint8)
    assert R.convert(v, 1, -1.5).tolist() == [0, 0, 98, 198, 253]            # 98.5 -> 98: truncated, not rounded
    assert R.convert(v, 1.5, 0).tolist() == [0, 1, 150, 255, 255]
    assert R.convert(v, 1, 31.99).tolist() == [31, 32, 131, 231, 255]


# ------------------------------------------------------------------------------------------------ bilinear
def _aten(img, dst):
    x = torch.from_numpy(img).permute(2, 0, 1)[None].float().contiguous()          # planes: ATen's separable route
    return F.interpolate(x, size=dst, mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()


@pytest.mark.parametrize("src, dst", [((37, 53), (74, 106)), ((64, 48), (32, 24)), ((50, 50), (50, 50)), ((16, 20), (64, 80)),
                                      ((64, 48), (32, 96)), ((512, 683), (256, 683))])
def test_bilinear_stage_is_atens_rounded(src, dst):
    """Scales 1/2, 1, 2, 4: every weight is a multiple of 1/8 and every product and sum of the interpolation is exact in fp32, so
    ATen's CPU kernel (compiled with fused multiply-adds) and the restatement (one rounding per operation, as the HIP kernel)
    cannot differ: equal as floats, and equal after the rounding to uint8."""
    rng = np.random.default_rng(src[0] * 1000 + dst[0])
    img = rng.integers(0, 256, (*src, 3), dtype=np.uint8)
    want = _aten(img, dst)
    assert np.array_equal(R.bilinear_float(img, *dst), want)
    got = R.bilinear_u8(img, *dst)
    assert got.dtype == np.uint8 and np.array_equal(got.astype(np.float32), np.rint(want))


@pytest.mark.parametrize("src, dst", [((37, 53), (19, 27)), ((64, 48), (23, 61)), ((50, 50), (63, 64)), ((37, 53), (64, 40))])
def test_bilinear_stage_is_atens_rounded_at_any_scale(src, dst):
    """General scales.  ATen's CPU build contracts a * b + c into fused multiply-adds (where, is the compiler's choice), so its
    floats differ from the uncontracted restatement in the last bits and the two can round a value that lies within that
    round-off of k + 1/2 to different grey levels.  Bound of the round-off of EITHER evaluation against the exact value, for
    coordinates below 64: the source coordinate carries <= 2.5 ulp(64) = 2.5 * 2^-18 (the scale's relative error 2^-24 times 64,
    three roundings of half an ulp), which moves the value by <= 255 * that = 2.4e-3 per axis; the six roundings of the
    interpolation itself add <= 6 * 2^-17.  Sum < 2^-7.  So: wherever the float64 restatement lies farther than 2^-7 from a tie,
    the rounded values must agree EXACTLY; nearer pixels (1.6 % of uniform noise) are counted, not compared."""
    assert max(*src, *dst) <= 64
    rng = np.random.default_rng(src[0] * 1000 + dst[0])
    img = rng.integers(0, 256, (*src, 3), dtype=np.uint8)
    want = np.rint(_aten(img, dst))
    got = R.bilinear_u8(img, *dst).astype(np.float32)
    exact = R.bilinear_float(img, *dst, dtype=np.float64)
    clear = np.abs(exact - np.floor(exact) - 0.5) > 2.0 ** -7
    print(f"{src} -> {dst}: {int((~clear).sum())} of {clear.size} values within 2^-7 of a tie; "
          f"{int((got != want).sum())} rounded differently by ATen's CPU kernel")
    assert clear.mean() > 0.95
    assert np.array_equal(got[clear], want[clear])
    assert np.abs(got - want).max() <= 1


# ------------------------------------------------------------------------------------------------ the crop rule
def window(counts, n=1024):
    """a 32 x 32 window holding counts = {label: pixels}"""
    flat = np.concatenate([np.full(c, l, np.uint8) for l, c in counts.items()])
    assert flat.size == n
    return flat.reshape(32, 32)


CROP_CASES = {
    "three_quarters_is_refused": ({3: 768, 9: 256}, False, False),          # 0.75 is not < 0.75
    "just_under_is_accepted": ({3: 767, 9: 257}, False, True),
    "one_class_plus_ignored": ({3: 500, 255: 524}, False, False),
    "all_ignored": ({255: 1024}, False, False),
    "ignored_do_not_enter_the_sum": ({3: 300, 9: 124, 255: 600}, False, True),      # 300 / 424 = 0.71; with the ignored: 0.29 either way
    "ignored_do_not_enter_the_sum_2": ({3: 400, 9: 100, 255: 524}, False, False),   # 400 / 500 = 0.8 refused; 400 / 1024 would pass
    "raw_zero_is_ignored_when_reduced": ({0: 524, 4: 400, 10: 100}, True, False),   # 400 / 500 after 0 -> 255
    "raw_zero_counts_otherwise": ({0: 524, 4: 400, 10: 100}, False, True),          # 524 / 1024
}


@pytest.mark.parametrize("name", list(CROP_CASES))
def test_crop_rule(name):
    counts, rzl, want = CROP_CASES[name]
    w = window(counts)
    if rzl:
        w = R.reduce_zero_label(w)
    assert R.crop_passes(w, 255, 0.75) is want


def crop_scene():
    """a 64 x 96 annotation whose 32 x 32 windows at known origins pass or fail; -> (seg, passing origin, failing origins)"""
    seg = np.full((64, 96), 5, np.uint8)
    seg[:32, 64:80] = 7                     # window (0, 64): 512 of 7, 512 of 5 -> passes
    return seg, (0, 64), [(0, 0), (32, 0), (32, 32), (16, 16)]


def test_candidate_choice():
    seg, good, bad = crop_scene()
    origins = [bad[i % 4] for i in range(11)]
    assert R.choose_candidate(seg, origins, (32, 32)) [0] == 10                        # all eleven fail: the eleventh
    origins[6] = good
    origins[8] = good
    assert R.choose_candidate(seg, origins, (32, 32))[0] == 6                          # the first passing one
    origins = [bad[0]] * 10 + [good]
    assert R.choose_candidate(seg, origins, (32, 32))[0] == 10
    assert R.choose_candidate(seg, [good] * 11, (32, 32), cat_max_ratio=1.0)[0] == 0   # no test at all: the first origin


# ------------------------------------------------------------------------------------------------ configuration
@pytest.mark.parametrize("pipeline, crop, scale, rzl", [(ADE_PIPELINE, (512, 512), (2048, 512), True),
                                                        (VOC_PIPELINE, (512, 512), (2048, 512), False),
                                                        (CITY_PIPELINE, (512, 1024), (2048, 1024), False)])
def test_from_cfg_reads_the_shipped_setups(pipeline, crop, scale, rzl):
    from spike2former_amd.augment import TrainAugment
    aug = TrainAugment.from_cfg(pipeline, preprocessor(crop), batch_size=2, seed=1, rank=0)
    assert aug.crop_size == crop and aug.scale == scale and aug.ratio_range == (0.5, 2.0)
    assert aug.cat_max_ratio == 0.75 and aug.flip_prob == 0.5 and aug.reduce_zero_label is rzl and aug.ignore_index == 255
    assert aug.photometric == dict(brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18)
    assert aug.mean == [123.675, 116.28, 103.53] and aug.std == [58.395, 57.12, 57.375] and aug.bgr_to_rgb is True
    assert aug.pad_val == 0 and aug.seg_pad_val == 255
    p = aug.draw([(1024, 2048)])[0]
    assert R.margins(int(p["H"]), int(p["W"]), crop) == (max(int(p["H"]) - crop[0], 0), max(int(p["W"]) - crop[1], 0))


def test_from_cfg_refuses_what_the_kernels_do_not_do():
    from spike2former_amd.augment import TrainAugment
    pre = preprocessor((512, 512))
    with pytest.raises(NotImplementedError, match="RandomRotate"):
        TrainAugment.from_cfg(ADE_PIPELINE[:5] + [dict(type="RandomRotate", prob=0.5, degree=10)] + ADE_PIPELINE[5:], pre)
    bad = [dict(t) for t in ADE_PIPELINE]
    bad[2] = dict(bad[2], keep_ratio=False)
    with pytest.raises(NotImplementedError, match="keep_ratio"):
        TrainAugment.from_cfg(bad, pre)
    bad = [dict(t) for t in ADE_PIPELINE]
    bad[4] = dict(bad[4], direction="vertical")
    with pytest.raises(NotImplementedError, match="RandomFlip"):
        TrainAugment.from_cfg(bad, pre)
    bad = [dict(t) for t in ADE_PIPELINE]
    bad[3] = dict(bad[3], some_option=1)
    with pytest.raises(NotImplementedError, match="some_option"):
        TrainAugment.from_cfg(bad, pre)
    with pytest.raises(NotImplementedError, match="after"):
        TrainAugment.from_cfg(ADE_PIPELINE[:3] + [ADE_PIPELINE[4], ADE_PIPELINE[3]] + ADE_PIPELINE[5:], pre)
    with pytest.raises(NotImplementedError, match="size"):
        TrainAugment.from_cfg(ADE_PIPELINE, preprocessor((640, 640)))
    with pytest.raises(NotImplementedError, match="size_divisor"):
        TrainAugment.from_cfg(ADE_PIPELINE, dict(preprocessor(None), size_divisor=32))


def test_there_is_no_host_route():
    from spike2former_amd import ops
    aug = make(device="cpu", crop_size=(32, 32), rank=0)
    img, seg = np.zeros((37, 53, 3), np.uint8), np.zeros((37, 53), np.uint8)
    with pytest.raises(RuntimeError, match="GPU only"):
        aug([img], [seg])
    data, table = torch.zeros(64, dtype=torch.uint8), torch.zeros(160, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.aug_crop_stats(data, table, torch.zeros(1, 11, dtype=torch.int32), (32, 32))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.aug_apply(data, table, None, torch.zeros(1, 3, 32, 32), torch.zeros(1, 32, 32, dtype=torch.uint8))


def test_stage_validates_the_table():
    aug = make(device="cpu", crop_size=(32, 32), rank=0, max_source_pixels=4096)
    img, seg = np.zeros((37, 53, 3), np.uint8), np.zeros((37, 53), np.uint8)
    p = aug.draw([(37, 53)])
    bad = p.copy()
    bad["crop_x"][0, 3] = int(bad["W"][0])          # outside [0, margin]
    with pytest.raises(ValueError, match="margin"):
        aug.stage([img], [seg], bad)
    with pytest.raises(ValueError, match="max_source_pixels"):
        aug.stage([np.zeros((100, 100, 3), np.uint8)], [np.zeros((100, 100), np.uint8)])
    with pytest.raises(ValueError, match="batch size"):
        aug.stage([img] * 3, [seg] * 3)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_argument_errors_are_reported_without_a_gpu():
    from spike2former_amd._lib import lib
    P = 1 << 20          # an aligned dummy address: never dereferenced on the host
    assert lib.s2f_aug_param_bytes() == 160
    ok_stats = (P, 1024, P, 1, 32, 32, 255, 0, 0.75, P, None)
    assert lib.s2f_aug_crop_stats(*((None,) + ok_stats[1:])) == -1 and b"null" in lib.s2f_last_error()
    assert lib.s2f_aug_crop_stats(*(ok_stats[:2] + (None,) + ok_stats[3:])) == -1 and b"null" in lib.s2f_last_error()
    assert lib.s2f_aug_crop_stats(*(ok_stats[:9] + (None, None))) == -1 and b"null" in lib.s2f_last_error()
    assert lib.s2f_aug_crop_stats(*(ok_stats[:3] + (0,) + ok_stats[4:])) == -1 and b"batch" in lib.s2f_last_error()
    assert lib.s2f_aug_crop_stats(*(ok_stats[:4] + (0, 32) + ok_stats[6:])) == -1 and b"crop" in lib.s2f_last_error()
    assert lib.s2f_aug_crop_stats(*(ok_stats[:4] + (32, -1) + ok_stats[6:])) == -1 and b"crop" in lib.s2f_last_error()
    assert lib.s2f_aug_crop_stats(*(ok_stats[:4] + (5000, 32) + ok_stats[6:])) == -1 and b"crop" in lib.s2f_last_error()
    ok_apply = (P, 1024, P, None, 1, 32, 32, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1, 0.0, 255, 0, P, P, None)
    assert lib.s2f_aug_apply(*((None,) + ok_apply[1:])) == -1 and b"null" in lib.s2f_last_error()
    assert lib.s2f_aug_apply(*(ok_apply[:17] + (None, P, None))) == -1 and b"null" in lib.s2f_last_error()
    assert lib.s2f_aug_apply(*(ok_apply[:17] + (P, None, None))) == -1 and b"null" in lib.s2f_last_error()
    assert lib.s2f_aug_apply(*(ok_apply[:4] + (-2,) + ok_apply[5:])) == -1 and b"batch" in lib.s2f_last_error()
    assert lib.s2f_aug_apply(*(ok_apply[:5] + (32, 0) + ok_apply[7:])) == -1 and b"crop" in lib.s2f_last_error()
    assert lib.s2f_aug_apply(*(ok_apply[:10] + (1.0, 0.0, 1.0) + ok_apply[13:])) == -1 and b"std" in lib.s2f_last_error()
    assert lib.s2f_aug_apply(*(ok_apply[:15] + (256,) + ok_apply[16:])) == -1 and b"seg_pad_val" in lib.s2f_last_error()
    assert lib.s2f_aug_apply(*(ok_apply[:1] + (0,) + ok_apply[2:])) == -1 and b"byte count" in lib.s2f_last_error()
