"""The device-side training augmentation (csrc/augment.hip through spike2former_amd.augment.TrainAugment) against its numpy
restatement tests/aug_ref.py.  The label map, the crop flags and the chosen crop are integers and must equal the restatement; the
image must equal the fp32 restatement BIT FOR BIT: every operation of the chain is one IEEE fp32 operation on both sides.  Every
output is pre-filled (NaN / 7) before the launches, so an element the kernel does not write fails the comparison."""
import gc
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_ref as R  # noqa: E402
from step_rig import region_map  # noqa: E402
from test_augment_host import CROP_CASES, crop_scene, window  # noqa: E402

pytestmark = pytest.mark.gpu

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
SOURCES = ((37, 53), (64, 48), (50, 50))
CROPS = ((32, 32), (24, 40), (30, 30))          # 30 x 30: the scalar-store variant
OFF = dict(flip=0, bright_on=0, mode=0, contrast_on=0, sat_on=0, hue_on=0, hue_delta=0, bright_beta=0.0, contrast_alpha=1.0,
           sat_alpha=1.0)


def scene(h0, w0, seed, n_classes=6):
    """a picture with noise, flat extremes, greys and saturated colours (the corners of the HSV conversions) and an annotation of
    rectangles with an ignored strip and some raw zeros"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8)
    img[:4, :6] = 0
    img[:4, 6:12] = 255
    img[4:8, :12] = np.arange(12, dtype=np.uint8)[None, :, None] * 23          # greys
    img[8:12, :6] = (0, 0, 255)
    img[8:12, 6:12] = (250, 3, 251)                                            # hue just below 360 degrees
    img[12:16, :6] = (255, 255, 0)
    img[12:16, 6:12] = (3, 250, 2)
    seg = np.empty((h0, w0), np.uint8)
    classes = rng.permutation(20)[:n_classes] + 1
    for i, (y, x) in enumerate((y, x) for y in range(0, h0, 9) for x in range(0, w0, 11)):
        seg[y:y + 9, x:x + 11] = classes[i % n_classes]
    seg[2:4, 3:17] = 255
    seg[20:23, 5:9] = 0
    return img, seg


def entry(aug, h0, w0, H=None, W=None, origins=None, **kw):
    """one parameter record: resized to H x W (default: not at all), all candidates at `origins` (one (y, x) or eleven)"""
    from spike2former_amd.augment import PARAM_DTYPE
    p = np.zeros(1, PARAM_DTYPE)[0]
    p["h0"], p["w0"], p["H"], p["W"] = h0, w0, H or h0, W or w0
    origins = origins or (0, 0)
    origins = [origins] * R.CANDIDATES if isinstance(origins[0], int) else origins
    p["crop_y"], p["crop_x"] = [o[0] for o in origins], [o[1] for o in origins]
    for k, v in {**OFF, **kw}.items():
        p[k] = v
    return p


def make(crop, batch=1, **kw):
    from spike2former_amd.augment import TrainAugment
    a = dict(crop_size=crop, cat_max_ratio=1.0, mean=MEAN, std=STD, bgr_to_rgb=True, batch_size=batch, max_source_pixels=64 * 96,
             seed=0, rank=0)
    a.update(kw)
    return TrainAugment(**a)


def ref_kwargs(aug):
    return dict(mean=aug.mean, std=aug.std, bgr_to_rgb=aug.bgr_to_rgb, pad_val=aug.pad_val, seg_pad_val=aug.seg_pad_val,
                reduce_zero=aug.reduce_zero_label, ignore_index=aug.ignore_index, cat_max_ratio=aug.cat_max_ratio)


def prefilled(aug, B):
    dev = torch.device("cuda")
    return (torch.full((B, 3, *aug.crop_size), float("nan"), device=dev),
            torch.full((B, *aug.crop_size), 7, dtype=torch.uint8, device=dev))


def run_and_compare(aug, images, segs, params):
    """-> (inputs, seg) as numpy after they were found equal to the restatement"""
    from spike2former_amd.augment import PARAM_DTYPE
    params = np.array(params, dtype=PARAM_DTYPE)
    out = prefilled(aug, len(images))
    got_in, got_seg = aug(images, segs, params, out=out)
    assert got_in.data_ptr() == out[0].data_ptr() and got_seg.data_ptr() == out[1].data_ptr()
    got_in, got_seg = got_in.cpu().numpy(), got_seg.cpu().numpy()
    want_in, want_seg, _ = R.batch(images, segs, params, aug.crop_size, **ref_kwargs(aug))
    assert np.array_equal(got_seg, want_seg)
    assert not np.isnan(got_in).any(), "an element of the image was not written"
    differ = got_in != want_in
    assert not differ.any(), (f"{int(differ.sum())} of {differ.size} image elements differ from the fp32 restatement, "
                              f"max |d| {np.abs(got_in - want_in).max():.3e}")
    return got_in, got_seg


# ------------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("src, crop", [((37, 53), (40, 56)), ((20, 27), (32, 32)), ((20, 27), (30, 30)), ((24, 40), (24, 40))])
def test_identity_route_is_the_data_preprocessor(src, crop):
    from spike2former_amd.data_preprocessor import PixelData, SegDataPreProcessor, SegDataSample
    img, seg = scene(*src, seed=1)
    aug = make(crop)
    got_in, got_seg = run_and_compare(aug, [img], [seg], [entry(aug, *src)])
    pre = SegDataPreProcessor(mean=MEAN, std=STD, bgr_to_rgb=True, size=crop, pad_val=0, seg_pad_val=255)
    sample = SegDataSample(gt_sem_seg=PixelData(torch.from_numpy(seg)[None].clone()))
    res = pre(dict(inputs=[torch.from_numpy(img).permute(2, 0, 1).contiguous()], data_samples=[sample]), training=True)
    assert np.array_equal(got_in, res["inputs"].numpy())          # bit for bit: the component preproc_f2.npz pins
    assert np.array_equal(got_seg, res["data_samples"][0].gt_sem_seg.data.numpy())


# ------------------------------------------------------------------------------------------------ 2. resize
RESIZES = [
    ((64, 48), (40, 30), (32, 32), (8, 0)),        # shrinking; narrower than the crop: padding on the right
    ((37, 53), (74, 106), (24, 40), (50, 66)),     # enlarging 2x, origin at the margin
    ((37, 53), (61, 87), (32, 32), (13, 21)),      # enlarging, no dyadic scale
    ((50, 50), (20, 25), (32, 32), (0, 0)),        # smaller than the crop in both dimensions
    ((50, 50), (45, 61), (30, 30), (7, 30)),       # scalar stores
    ((64, 48), (23, 90), (24, 40), (0, 17)),       # shrinking rows, enlarging columns; shorter than the crop
]


@pytest.mark.parametrize("src, size, crop, origin", RESIZES)
def test_resize(src, size, crop, origin):
    img, seg = scene(*src, seed=2)
    aug = make(crop)
    run_and_compare(aug, [img], [seg], [entry(aug, *src, *size, origins=origin)])
    # the same window of ATen's own bilinear resize on the device, rounded: the raw grey levels (no swap, no normalisation).  ATen's
    # kernel is built with fused multiply-adds, this one and the restatement with one rounding per operation: the two may round a
    # value within their round-off of k + 1/2 differently.  Coordinates below 128: <= 2.5 ulp(128) * 255 = 4.9e-3 per axis from the
    # source coordinate + 6 * 2^-17 from the interpolation < 2^-6 (test_augment_host.py derives the bound); farther from a tie than
    # that the grey levels must be EQUAL
    assert max(*src, *size) <= 128
    raw = make(crop, mean=None, std=None, bgr_to_rgb=False)
    got, _ = raw([img], [seg], np.array([entry(raw, *src, *size, origins=origin)]), out=prefilled(raw, 1))
    x = torch.from_numpy(img).permute(2, 0, 1)[None].float().contiguous().cuda()
    hv, wv = min(crop[0], size[0]), min(crop[1], size[1])
    win = (slice(None), slice(origin[0], origin[0] + hv), slice(origin[1], origin[1] + wv))
    want = torch.round(F.interpolate(x, size=size, mode="bilinear", align_corners=False))[0][win].cpu().numpy()
    exact = R.bilinear_float(img, *size, dtype=np.float64).transpose(2, 0, 1)[win]
    clear = np.abs(exact - np.floor(exact) - 0.5) > 2.0 ** -6
    got = got[0, :, :hv, :wv].cpu().numpy()
    print(f"{src} -> {size}: {int((~clear).sum())} of {clear.size} values within 2^-6 of a tie, {int((got != want).sum())} rounded "
          f"differently by ATen's kernel")
    # (not vacuous: most values are compared -- at an exact scale of 2 every second column has the weight 1/2 and every odd a + b
    # is a tie, computed exactly by both sides: up to an eighth of the values there)
    assert clear.mean() > 0.75 and np.array_equal(got[clear], want[clear]) and np.abs(got - want).max() <= 1


# ------------------------------------------------------------------------------------------------ 3. crop and flip
@pytest.mark.parametrize("crop", CROPS)
@pytest.mark.parametrize("flip", (0, 1))
def test_crop_and_flip(crop, flip):
    src, size = (64, 48), (80, 60)
    img, seg = scene(*src, seed=3)
    aug = make(crop, batch=3)
    my, mx = R.margins(*size, crop)
    assert my > 0 and mx > 0
    params = [entry(aug, *src, *size, origins=o, flip=flip) for o in ((0, 0), (my, mx), (my // 3 + 1, mx // 2 + 1))]
    got_in, _ = run_and_compare(aug, [img] * 3, [seg] * 3, params)
    assert not np.array_equal(got_in[0], got_in[1]) and not np.array_equal(got_in[0], got_in[2])


def test_flip_of_a_picture_narrower_than_the_crop_stays_left_aligned():
    src, crop = (50, 50), (32, 32)
    img, seg = scene(*src, seed=4)
    aug = make(crop)
    got_in, got_seg = run_and_compare(aug, [img], [seg], [entry(aug, *src, 40, 20, origins=(5, 0), flip=1)])
    assert (got_seg[0, :, 20:] == 255).all() and (got_in[0, :, :, 20:] == 0).all() and (got_seg[0, :, :20] != 255).any()


# ------------------------------------------------------------------------------------------------ 4. photometric
PHOTO = {
    "brightness_up_clips_at_255": dict(bright_on=1, bright_beta=31.7),
    "brightness_down_clips_at_0": dict(bright_on=1, bright_beta=-31.2),
    "contrast_up_clips": dict(contrast_on=1, contrast_alpha=1.49, mode=0),
    "contrast_down_mode_1": dict(contrast_on=1, contrast_alpha=0.53, mode=1),
    "saturation_up_clips": dict(sat_on=1, sat_alpha=1.47),
    "saturation_down": dict(sat_on=1, sat_alpha=0.51),
    "hue_up_wraps": dict(hue_on=1, hue_delta=17),
    "hue_down_wraps": dict(hue_on=1, hue_delta=-18),
    "all_mode_0": dict(bright_on=1, bright_beta=-20.3, contrast_on=1, contrast_alpha=1.3, sat_on=1, sat_alpha=1.3, hue_on=1,
                       hue_delta=11, mode=0),
    "all_mode_1": dict(bright_on=1, bright_beta=25.6, contrast_on=1, contrast_alpha=0.7, sat_on=1, sat_alpha=0.8, hue_on=1,
                       hue_delta=-7, mode=1, flip=1),
}


@pytest.mark.parametrize("name", list(PHOTO))
def test_photometric(name):
    src, size, crop = (37, 53), (45, 64), (32, 32)
    img, seg = scene(*src, seed=5)
    aug = make(crop, batch=2)
    params = [entry(aug, *src, origins=(0, 0), **PHOTO[name]), entry(aug, *src, *size, origins=(6, 20), **PHOTO[name])]
    got_in, _ = run_and_compare(aug, [img] * 2, [seg] * 2, params)
    plain, _ = run_and_compare(aug, [img], [seg], [entry(aug, *src, origins=(0, 0))])
    assert not np.array_equal(got_in[0], plain[0]), "the distortion changed nothing"


def test_photometric_modes_differ():
    src, crop = (37, 53), (32, 32)
    img, seg = scene(*src, seed=5)
    aug = make(crop, batch=2)
    both = {k: v for k, v in PHOTO["all_mode_0"].items() if k != "mode"}
    got_in, _ = run_and_compare(aug, [img] * 2, [seg] * 2, [entry(aug, *src, mode=0, **both), entry(aug, *src, mode=1, **both)])
    assert not np.array_equal(got_in[0], got_in[1])


# ------------------------------------------------------------------------------------------------ 5. batches
@pytest.mark.parametrize("crop", CROPS)
def test_batch_of_three_sizes_with_drawn_parameters(crop):
    """B = 3, three source sizes packed back to back (5 883-, 9 216- and 7 500-byte pictures: unaligned offsets), parameters from
    TrainAugment.draw with every transform on, the crop rule included (two launches), reduce_zero_label on"""
    pairs = [scene(h, w, seed=10 + i) for i, (h, w) in enumerate(SOURCES)]
    images, segs = [p[0] for p in pairs], [p[1] for p in pairs]
    aug = make(crop, batch=3, scale=(96, 48), ratio_range=(0.5, 2.0), cat_max_ratio=0.75, flip_prob=0.5, photometric=True,
               reduce_zero_label=True, seed=crop[0])
    for _ in range(3):
        params = aug.draw([s.shape for s in segs])
        out = prefilled(aug, 3)
        staged = aug.stage(images, segs, params)
        assert [int(v) % 4 for v in staged["img_off"]] != [0, 0, 0] or [int(v) % 4 for v in staged["seg_off"]] != [0, 0, 0]
        aug.launch(out)
        want_in, want_seg, _ = R.batch(images, segs, staged, crop, **ref_kwargs(aug))
        assert np.array_equal(out[1].cpu().numpy(), want_seg)
        assert np.array_equal(out[0].cpu().numpy(), want_in)


def test_own_buffers_and_smaller_batches():
    pairs = [scene(h, w, seed=20 + i) for i, (h, w) in enumerate(SOURCES)]
    images, segs = [p[0] for p in pairs], [p[1] for p in pairs]
    aug = make((32, 32), batch=3)
    params = [entry(aug, *s.shape, origins=(1, 2)) for s in segs]
    a_in, a_seg = aug(images, segs, np.array(params))
    assert tuple(a_in.shape) == (3, 3, 32, 32) and tuple(a_seg.shape) == (3, 32, 32)
    want_in, want_seg, _ = R.batch(images, segs, params, (32, 32), **ref_kwargs(aug))
    assert np.array_equal(a_in.cpu().numpy(), want_in) and np.array_equal(a_seg.cpu().numpy(), want_seg)
    b_in, b_seg = aug(images[1:], segs[1:], np.array(params[1:]))          # persistent buffers: the same storage, a shorter view
    assert b_in.data_ptr() == a_in.data_ptr() and tuple(b_in.shape) == (2, 3, 32, 32)
    assert np.array_equal(b_in.cpu().numpy(), want_in[1:]) and np.array_equal(b_seg.cpu().numpy(), want_seg[1:])


def test_odd_offsets_through_the_op_layer():
    """the op layer on a hand-packed buffer: one stray byte in front, so the picture starts at byte 1 and the annotation at an odd
    byte as well"""
    from spike2former_amd import ops
    from spike2former_amd.augment import PARAM_DTYPE
    img, seg = scene(37, 53, seed=25)
    aug = make((32, 32), cat_max_ratio=0.75)
    p = entry(aug, 37, 53, 45, 64, origins=[(i, 2 * i) for i in range(11)], flip=1, **PHOTO["all_mode_0"])
    p["img_off"], p["seg_off"] = 1, 1 + img.size
    raw = np.concatenate([np.array([99], np.uint8), img.reshape(-1), seg.reshape(-1)])
    data = torch.from_numpy(raw).cuda()
    table = torch.from_numpy(np.array([p], dtype=PARAM_DTYPE).view(np.uint8).copy()).cuda()
    flags = torch.full((1, R.CANDIDATES), 7, dtype=torch.int32, device="cuda")
    out = prefilled(aug, 1)
    ops.aug_crop_stats(data, table, flags, (32, 32), 255, False, 0.75)
    ops.aug_apply(data, table, flags, *out, MEAN, STD, True, 0.0, 255, False)
    want = R.pipeline(img, seg, p, (32, 32), **ref_kwargs(aug))
    assert flags.cpu().tolist() == [[int(f) for f in want["flags"]]]
    assert np.array_equal(out[1][0].cpu().numpy(), want["seg"]) and np.array_equal(out[0][0].cpu().numpy(), want["inputs"])


# ------------------------------------------------------------------------------------------------ 6. the crop rule
def test_crop_stats_on_the_constructed_windows():
    """the 32 x 32 windows of the CPU test, one picture each: the flag of every candidate equals crop_bbox's rule"""
    from spike2former_amd import ops
    for rzl in (False, True):
        names = [n for n, c in CROP_CASES.items() if c[1] is rzl]
        wins = [window(CROP_CASES[n][0]) for n in names]
        aug = make((32, 32), batch=len(wins), cat_max_ratio=0.75, reduce_zero_label=rzl)
        aug.stage([np.zeros((32, 32, 3), np.uint8)] * len(wins), wins, np.array([entry(aug, 32, 32) for _ in wins]))
        B = len(wins)
        flags = torch.full((B, R.CANDIDATES), 7, dtype=torch.int32, device="cuda")
        ops.aug_crop_stats(aug._dev[aug._table_cap:], aug._dev[:B * 160], flags, (32, 32), 255, rzl, 0.75)
        want = [[int(CROP_CASES[n][2])] * R.CANDIDATES for n in names]
        assert flags.cpu().tolist() == want, names
        for w, n in zip(wins, names):
            assert R.crop_passes(R.reduce_zero_label(w) if rzl else w, 255, 0.75) is CROP_CASES[n][2]


@pytest.mark.parametrize("crop", ((32, 32), (30, 30)))
def test_chosen_candidate_is_the_restatements(crop):
    """a nearest-RESIZED annotation (64 x 96 -> 96 x 144, then 51 x 77) and windows that pass or fail by construction or by chance:
    every flag and the chosen candidate (through the crop that comes out) equal the restatement"""
    from spike2former_amd import ops
    seg, good, bad = crop_scene()
    img = scene(64, 96, seed=30)[0]
    rng = np.random.default_rng(31)
    tables = []
    aug = make(crop, batch=4, cat_max_ratio=0.75)
    fail = [(3 * y // 2, 3 * x // 2) for y, x in bad]                       # uniform regions of the 96 x 144 map
    tables.append(entry(aug, 64, 96, 96, 144, origins=[fail[i % 4] for i in range(11)]))                       # all fail -> 10
    o = [fail[i % 4] for i in range(11)]
    o[6] = o[8] = (0, 104)                                             # 16 columns of class 7, the rest class 5
    tables.append(entry(aug, 64, 96, 96, 144, origins=o))                                                      # -> 6
    my, mx = R.margins(96, 144, crop)
    tables.append(entry(aug, 64, 96, 96, 144, origins=[(int(rng.integers(0, my + 1)), int(rng.integers(0, mx + 1)))
                                                       for _ in range(11)]))
    my, mx = R.margins(51, 77, crop)
    tables.append(entry(aug, 64, 96, 51, 77, origins=[(int(rng.integers(0, my + 1)), int(rng.integers(0, mx + 1)))
                                                      for _ in range(11)], flip=1))
    images, segs = [img] * 4, [seg] * 4
    _, _ = run_and_compare(aug, images, segs, tables)
    want = [R.pipeline(i, s, p, crop, **ref_kwargs(aug)) for i, s, p in zip(images, segs, tables)]
    assert [w["choice"] for w in want][:2] == [10, 6]
    assert aug._flags.cpu().tolist() == [[int(f) for f in w["flags"]] for w in want]
    assert len({tuple(w["flags"]) for w in want}) > 1


# ------------------------------------------------------------------------------------------------ 7. graph capture
def test_graph_replays_follow_the_static_buffers():
    pairs = [scene(h, w, seed=40 + i) for i, (h, w) in enumerate(SOURCES)]
    images, segs = [p[0] for p in pairs], [p[1] for p in pairs]
    crop = (32, 32)
    aug = make(crop, batch=3, scale=(96, 48), cat_max_ratio=0.75, photometric=True, seed=9)
    out = prefilled(aug, 3)
    first = aug.stage(images, segs, aug.draw([s.shape for s in segs]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aug.launch(out)                                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                  # the two launches: one chain
        aug.launch(out)
    for k, (imgs_k, segs_k, table) in enumerate(((images, segs, first), (images[::-1], segs[::-1], None), (images, segs, None))):
        table = aug.stage(imgs_k, segs_k, table if table is not None else aug.draw([s.shape for s in segs_k]))
        out[0].fill_(float("nan"))
        out[1].fill_(7)
        graph.replay()
        want_in, want_seg, _ = R.batch(imgs_k, segs_k, table, crop, **ref_kwargs(aug))
        assert np.array_equal(out[1].cpu().numpy(), want_seg), k
        assert np.array_equal(out[0].cpu().numpy(), want_in), k
    del graph


# ------------------------------------------------------------------------------------------------ 8. the training step
def test_training_step_fed_in_place():
    """GraphedHungarianStep(assign="device") on the tiny configuration, fed through out=(static_in, static_seg): finite losses,
    bit-equal to the same step fed with the restatement's tensors"""
    import spike2former_amd as s2f
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.graph import GraphedHungarianStep
    from spike2former_amd.init_utils import seeded_init
    w = s2f.WORKLOADS["C1_64"]
    crop = (w["H"], w["W"])
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C1_64"))).cuda().train()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    s2f.set_keep_membrane(model, False)
    red = FlatGradAllReduce(model.parameters(), 1)
    rng = np.random.default_rng(50)
    shapes = ((70, 90), (64, 48))
    images = [rng.integers(0, 256, (h, ww, 3), dtype=np.uint8) for h, ww in shapes]
    segs = [region_map(h, ww, rng.permutation(w["K"])[:5 + i]) for i, (h, ww) in enumerate(shapes)]
    aug = make(crop, batch=2, scale=(2 * crop[1], crop[0]), ratio_range=(0.5, 2.0), cat_max_ratio=0.75, photometric=True, seed=11,
               max_source_pixels=70 * 90)
    example_in = torch.randn(2, 3, *crop, generator=torch.Generator().manual_seed(5)).cuda()
    example_seg = torch.from_numpy(np.stack([region_map(*crop, [1, 2, 3]), region_map(*crop, [4, 5])])).cuda()
    step = GraphedHungarianStep(model, example_in, example_seg, red, warmup=1, assign="device")
    table = aug.draw(shapes)
    want_in, want_seg, _ = R.batch(images, segs, table, crop, **ref_kwargs(aug))
    model.load_state_dict(sd)
    step.static_in.fill_(float("nan"))
    step.static_seg.fill_(7)
    aug(images, segs, table, out=(step.static_in, step.static_seg))
    got = step()
    step.check()
    got = {k: float(v) for k, v in got.items()}
    assert np.array_equal(step.static_in.cpu().numpy(), want_in) and np.array_equal(step.static_seg.cpu().numpy(), want_seg)
    model.load_state_dict(sd)
    ref = step(torch.from_numpy(want_in).cuda(), torch.from_numpy(want_seg).cuda())
    step.check()
    ref = {k: float(v) for k, v in ref.items()}
    assert all(np.isfinite(v) for v in got.values()) and len(got) > 0
    assert got == ref
    del step
    for p in model.parameters():
        p.grad = None
    gc.collect()
