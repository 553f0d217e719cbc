"""CPU: the host half of the device-side test pipeline (spike2former_amd.augment.TestAugment, ops.test_views): the sizes of the
views against constants computed with mmcv 2.x's rule, the padding, the configuration reader on the shipped test_pipeline /
tta_pipeline, the table, the op's validation of a table before any launch, and EncoderDecoder.preprocess' pass-through."""
import itertools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import view_ref as VR  # noqa: E402

RATIOS = [0.5, 0.75, 1.0, 1.25, 1.5, 1.75]
TEST_PIPELINE = [
    dict(type="LoadImageFromFile"),
    dict(type="Resize", scale=(2048, 512), keep_ratio=True),
    dict(type="LoadAnnotations", reduce_zero_label=True),
    dict(type="PackSegInputs"),
]
TTA_PIPELINE = [
    dict(type="LoadImageFromFile"),
    dict(type="TestTimeAug", transforms=[
        [dict(type="Resize", scale_factor=r, keep_ratio=True) for r in RATIOS],
        [dict(type="RandomFlip", prob=0., direction="horizontal"), dict(type="RandomFlip", prob=1., direction="horizontal")],
        [dict(type="LoadAnnotations")],
        [dict(type="PackSegInputs")]]),
]
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
ADE_PRE = dict(type="SegDataPreProcessor", mean=MEAN, std=STD, bgr_to_rgb=True, pad_val=0, seg_pad_val=255, size=(512, 512))
CITY_PRE = dict(type="SegDataPreProcessor", mean=MEAN, std=STD, bgr_to_rgb=True, pad_val=0, seg_pad_val=255, size=(512, 1024),
                test_cfg=dict(size_divisor=32))

# (source) -> the six (H, W) of Resize(scale_factor=r, keep_ratio=True), r = 0.5 .. 1.75, computed with mmcv 2.x's rule
FACTOR_SIZES = {
    (37, 53): [(19, 27), (28, 40), (37, 53), (46, 66), (56, 80), (65, 93)],
    (512, 683): [(256, 342), (384, 512), (512, 683), (640, 854), (768, 1025), (896, 1195)],          # 1025: rounded twice
    (375, 500): [(188, 250), (281, 375), (375, 500), (469, 625), (563, 750), (656, 875)],
}
SCALE_SIZES = {(375, 500): (512, 683), (37, 53): (512, 733), (1024, 2048): (512, 1024)}          # Resize(scale=(2048, 512))


def make(**kw):
    from spike2former_amd.augment import TestAugment
    return TestAugment(**{**dict(device="cpu"), **kw})


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("src", list(FACTOR_SIZES))
def test_scale_factor_sizes_known_answers(src):
    aug = make(scale=None, scale_factors=RATIOS, flips=(False, True))
    got = aug.view_sizes(*src)
    assert len(got) == 12
    assert [v[:2] for v in got[::2]] == FACTOR_SIZES[src] and [v[:2] for v in got[1::2]] == FACTOR_SIZES[src]
    assert [v[4] for v in got] == [False, True] * 6                      # ratio slowest, flip fastest
    assert all(v[2:4] == v[:2] for v in got)                             # no test_cfg: no padding


@pytest.mark.parametrize("src", list(SCALE_SIZES))
def test_scale_sizes_known_answers(src):
    assert make(scale=(2048, 512)).view_sizes(*src) == [(*SCALE_SIZES[src], *SCALE_SIZES[src], False)]


def test_no_resize_is_the_source_size():
    assert make(scale=None).view_sizes(37, 53) == [(37, 53, 37, 53, False)]


def test_padding_follows_stack_batch():
    from spike2former_amd.data_preprocessor import stack_batch
    assert make(scale=None, size=(40, 56)).view_sizes(37, 53) == [(37, 53, 40, 56, False)]
    assert make(scale=None, size=(40, 56)).view_sizes(64, 48) == [(64, 48, 64, 56, False)]          # max(size - dim, 0)
    assert make(scale=None, size_divisor=32).view_sizes(37, 53) == [(37, 53, 64, 64, False)]
    assert make(scale=None, size_divisor=32).view_sizes(64, 96) == [(64, 96, 64, 96, False)]
    assert make(scale=None).view_sizes(37, 53) == [(37, 53, 37, 53, False)]
    for kw in (dict(size=(40, 56)), dict(size_divisor=32), dict(size_divisor=1)):
        for src in ((37, 53), (64, 48), (64, 96)):
            _, info = stack_batch([torch.zeros(3, *src)], None, kw.get("size"), kw.get("size_divisor"))
            assert make(scale=None, **kw).view_sizes(*src)[0][2:4] == info[0]["pad_shape"], (kw, src)
    with pytest.raises(ValueError, match="only one"):
        make(size=(40, 56), size_divisor=32)


# ------------------------------------------------------------------------------------------------ configuration
def test_from_cfg_reads_the_shipped_test_pipeline():
    from spike2former_amd.augment import TestAugment
    aug = TestAugment.from_cfg(TEST_PIPELINE, ADE_PRE, device="cpu")
    assert aug.scale == (2048, 512) and aug.scale_factors is None and aug.flips == (False,) and aug.tta is False
    assert aug.reduce_zero_label is True and aug.n_views == 1
    assert aug.mean == MEAN and aug.std == STD and aug.bgr_to_rgb is True and aug.pad_val == 0
    assert aug.size is None and aug.size_divisor is None          # `size` outside test_cfg is the training branch's
    assert aug.view_sizes(375, 500) == [(512, 683, 512, 683, False)]
    city = TestAugment.from_cfg([TEST_PIPELINE[0], dict(type="Resize", scale=(2048, 1024), keep_ratio=True),
                                 dict(type="LoadAnnotations"), TEST_PIPELINE[3]], CITY_PRE, device="cpu")
    assert city.scale == (2048, 1024) and city.size_divisor == 32 and city.reduce_zero_label is False
    assert city.view_sizes(1024, 2048) == [(1024, 2048, 1024, 2048, False)]
    assert city.view_sizes(375, 500) == [(1024, 1365, 1024, 1376, False)]


def test_from_cfg_reads_the_shipped_tta_pipeline():
    from spike2former_amd.augment import TestAugment
    aug = TestAugment.from_cfg(TTA_PIPELINE, ADE_PRE, reduce_zero_label=True, device="cpu")
    assert aug.scale is None and aug.scale_factors == tuple(RATIOS) and aug.flips == (False, True) and aug.tta is True
    assert aug.n_views == 12 and aug.reduce_zero_label is True          # LoadAnnotations without the option: the keyword
    assert TestAugment.from_cfg(TTA_PIPELINE, ADE_PRE, device="cpu").reduce_zero_label is False
    want = [(*FACTOR_SIZES[(37, 53)][i], f) for i, f in itertools.product(range(6), (False, True))]
    assert [(v[0], v[1], v[4]) for v in aug.view_sizes(37, 53)] == want
    city = TestAugment.from_cfg(TTA_PIPELINE, CITY_PRE, device="cpu")
    assert city.size_divisor == 32
    assert [v[2:4] for v in city.view_sizes(37, 53)[::2]] == [(32, 32), (32, 64), (64, 64), (64, 96), (64, 96), (96, 96)]


def _tta(resize=None, flip=None, groups=None):
    t = [list(g) for g in TTA_PIPELINE[1]["transforms"]]
    if resize is not None:
        t[0] = resize
    if flip is not None:
        t[1] = flip
    if groups is not None:
        t = [t[i] for i in groups]
    return [TTA_PIPELINE[0], dict(type="TestTimeAug", transforms=t)]


def test_from_cfg_refuses_what_the_kernel_does_not_do():
    from spike2former_amd.augment import TestAugment
    f = TestAugment.from_cfg
    with pytest.raises(NotImplementedError, match="keep_ratio"):
        f([TEST_PIPELINE[0], dict(type="Resize", scale=(2048, 512), keep_ratio=False)] + TEST_PIPELINE[2:], ADE_PRE)
    with pytest.raises(NotImplementedError, match="keep_ratio"):
        f(_tta(resize=[dict(type="Resize", scale_factor=0.5, keep_ratio=False)]), ADE_PRE)
    with pytest.raises(NotImplementedError, match="vertical"):
        f(_tta(flip=[dict(type="RandomFlip", prob=0.), dict(type="RandomFlip", prob=1., direction="vertical")]), ADE_PRE)
    with pytest.raises(NotImplementedError, match="prob=0.5"):
        f(_tta(flip=[dict(type="RandomFlip", prob=0.5, direction="horizontal")]), ADE_PRE)
    with pytest.raises(NotImplementedError, match="RandomRotate"):
        f(TEST_PIPELINE[:2] + [dict(type="RandomRotate", prob=1.0, degree=10)] + TEST_PIPELINE[2:], ADE_PRE)
    with pytest.raises(NotImplementedError, match="ResizeToMultiple"):
        f(_tta(resize=[dict(type="ResizeToMultiple", size_divisor=32)]), ADE_PRE)
    with pytest.raises(NotImplementedError, match="Resize after RandomFlip"):
        f(_tta(groups=(1, 0, 2, 3)), ADE_PRE)
    with pytest.raises(NotImplementedError, match="Resize after LoadAnnotations"):
        f([TEST_PIPELINE[0], TEST_PIPELINE[2], TEST_PIPELINE[1], TEST_PIPELINE[3]], ADE_PRE)
    with pytest.raises(NotImplementedError, match="interpolation"):
        f([TEST_PIPELINE[0], dict(TEST_PIPELINE[1], interpolation="bicubic")] + TEST_PIPELINE[2:], ADE_PRE)
    with pytest.raises(NotImplementedError, match="batch_augments"):
        f(TEST_PIPELINE, dict(ADE_PRE, batch_augments=[dict(type="X")]))
    with pytest.raises(NotImplementedError, match="mode"):
        f(TEST_PIPELINE, dict(ADE_PRE, test_cfg=dict(size_divisor=32, mode="x")))


def test_there_is_no_host_route():
    from spike2former_amd import ops
    aug = make(scale=None)
    with pytest.raises(RuntimeError, match="GPU only"):
        aug([np.zeros((37, 53, 3), np.uint8)])
    t, n = aug.table(37, 53)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.test_views(torch.zeros(3 * 37 * 53, dtype=torch.uint8), t, torch.zeros(n))
    with pytest.raises(ValueError, match="ONE size"):
        make(scale=None, batch_size=2).stage([np.zeros((37, 53, 3), np.uint8), np.zeros((24, 40, 3), np.uint8)])
    with pytest.raises(ValueError, match="max_source_pixels"):
        make(scale=None, max_source_pixels=100).stage([np.zeros((37, 53, 3), np.uint8)])


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("B", (1, 2))
def test_table_blocks_are_aligned_disjoint_and_in_view_order(B):
    from spike2former_amd import ops
    from spike2former_amd.augment import VIEW_PARAM_DTYPE
    assert VIEW_PARAM_DTYPE.itemsize == ops.VIEW_PARAM_BYTES == 48
    aug = make(scale=None, scale_factors=RATIOS, flips=(False, True), batch_size=B)
    t, n = aug.table(37, 53, B)
    sizes = aug.view_sizes(37, 53)
    assert t.dtype == VIEW_PARAM_DTYPE and len(t) == 12 * B
    end = 0
    for k, p in enumerate(t):
        v, b = divmod(k, B)
        assert (p["H"], p["W"], p["Hp"], p["Wp"], bool(p["flip"])) == sizes[v]
        assert (p["h0"], p["w0"], p["img_off"]) == (37, 53, 3 * 37 * 53 * b)
        assert p["out_off"] % 4 == 0 and end <= p["out_off"] < end + 4          # packed: the next multiple of 4
        end = int(p["out_off"]) + 3 * int(p["Hp"]) * int(p["Wp"])
    assert end <= n < end + 4
    assert any((3 * int(p["Hp"]) * int(p["Wp"])) % 4 for p in t)                # the odd sizes do leave gaps
    ops.check_view_table(t, 3 * 37 * 53 * B, n)


def test_op_refuses_a_bad_table_before_any_launch():
    """CPU tensors: a valid table gets as far as the device check (RuntimeError), a bad entry is refused before that (ValueError)"""
    from spike2former_amd import ops
    aug = make(scale=None, scale_factors=(1.0, 0.5), flips=(False,))
    good, n = aug.table(37, 53)
    data, out = torch.zeros(3 * 37 * 53, dtype=torch.uint8), torch.zeros(n)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.test_views(data, good, out)

    def bad(match, **fields):
        t = good.copy()
        for k, v in fields.items():
            t[1][k] = v
        with pytest.raises(ValueError, match=match):
            ops.test_views(data, t, out)
    bad("leaves data", img_off=1)                                      # source past data
    bad("leaves data", img_off=-1)
    bad("leaves data", h0=38)
    bad("leaves out", out_off=int(good[1]["out_off"]) + 4)             # block past out
    bad("multiple of 4", out_off=int(good[1]["out_off"]) + 1)
    bad("overlap", out_off=int(good[0]["out_off"]))                    # on top of entry 0
    bad("overlap", out_off=int(good[1]["out_off"]) - 4)
    bad("padded", Hp=int(good[1]["H"]) - 1)                            # Hp < H
    bad("padded", Wp=int(good[1]["W"]) - 1)
    bad("padded", H=0)
    bad("padded", Wp=4097, W=4097)
    bad("source size", w0=0)
    with pytest.raises(ValueError, match="VIEW_PARAM_DTYPE"):
        ops.test_views(data, np.zeros(1, np.int32), out)
    with pytest.raises(ValueError, match="go together"):
        ops.test_views(data, good, out, mean=MEAN)


def test_argument_errors_are_reported_without_a_gpu():
    from spike2former_amd._lib import lib
    P = 1 << 20          # an aligned dummy address: never dereferenced on the host
    assert lib.s2f_view_param_bytes() == 48
    ok = (P, 1024, P, 1, 32, 32, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1, 0.0, P, 3 * 32 * 32, None)
    assert lib.s2f_test_views(*((None,) + ok[1:])) == -1 and b"null" in lib.s2f_last_error()
    assert lib.s2f_test_views(*(ok[:14] + (None,) + ok[15:])) == -1 and b"null" in lib.s2f_last_error()
    assert lib.s2f_test_views(*(ok[:3] + (0,) + ok[4:])) == -1 and b"entries" in lib.s2f_last_error()
    assert lib.s2f_test_views(*(ok[:3] + (65536,) + ok[4:])) == -1 and b"entries" in lib.s2f_last_error()
    assert lib.s2f_test_views(*(ok[:4] + (0, 32) + ok[6:])) == -1 and b"padded size" in lib.s2f_last_error()
    assert lib.s2f_test_views(*(ok[:4] + (32, 4097) + ok[6:])) == -1 and b"padded size" in lib.s2f_last_error()
    assert lib.s2f_test_views(*(ok[:9] + (1.0, 0.0, 1.0) + ok[12:])) == -1 and b"std" in lib.s2f_last_error()
    assert lib.s2f_test_views(*(ok[:15] + (0,) + ok[16:])) == -1 and b"element count" in lib.s2f_last_error()
    assert lib.s2f_test_views(*(ok[:2] + (P + 4,) + ok[3:])) == -2 and b"aligned" in lib.s2f_last_error()


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_at_the_source_size_is_the_data_preprocessor():
    from spike2former_amd.data_preprocessor import SegDataPreProcessor
    img, _ = VR.scene(37, 53, seed=1)
    pre = SegDataPreProcessor(mean=MEAN, std=STD, bgr_to_rgb=True, test_cfg=dict(size_divisor=32))
    want = pre(dict(inputs=[torch.from_numpy(img).permute(2, 0, 1).contiguous()]), training=False)["inputs"][0].numpy()
    got = VR.view(img, 37, 53, 64, 64, False, mean=MEAN, std=STD, bgr_to_rgb=True)
    assert np.array_equal(got, want)
    flipped = VR.view(img, 37, 53, 64, 64, True, mean=MEAN, std=STD, bgr_to_rgb=True)
    assert np.array_equal(flipped[:, :37, :53], want[:, :37, :53][:, :, ::-1]) and (flipped[:, :, 53:] == 0).all()


# ------------------------------------------------------------------------------------------------ the consumer
def test_preprocess_passes_a_preprocessed_batch_through():
    from spike2former_amd.data_preprocessor import SegDataPreProcessor, SegDataSample
    from spike2former_amd.segmentor import EncoderDecoder
    pre = SegDataPreProcessor(mean=MEAN, std=STD, bgr_to_rgb=True, test_cfg=dict(size_divisor=32))
    model = types.SimpleNamespace(data_preprocessor=pre)
    x, samples = torch.randn(1, 3, 64, 64), [SegDataSample(metainfo=dict(ori_shape=(37, 53)))]
    out = EncoderDecoder.preprocess(model, dict(inputs=x, data_samples=samples, preprocessed=True), False)
    assert out["inputs"] is x and out["data_samples"] is samples and set(out) == {"inputs", "data_samples"}
    img, _ = VR.scene(37, 53, seed=2)

    def raw():
        return dict(inputs=[torch.from_numpy(img).permute(2, 0, 1).contiguous()], data_samples=[SegDataSample()])
    for data in (raw(), dict(raw(), preprocessed=False)):
        got, want = EncoderDecoder.preprocess(model, data, False), pre(raw(), False)
        assert torch.equal(got["inputs"], want["inputs"]) and tuple(got["inputs"].shape) == (1, 3, 64, 64)
        assert got["data_samples"][0].metainfo == want["data_samples"][0].metainfo
    # the training branch never looks at the mark
    with pytest.raises(AssertionError):
        EncoderDecoder.preprocess(model, dict(inputs=[torch.zeros(3, 8, 8)], data_samples=None, preprocessed=True), True)
