"""GPU: s2f_slide_accumulate / s2f_slide_windows against tests/slide_ref.py (the numpy restatement of the reference's
slide_inference loop) and against torch slicing, and EncoderDecoder.slide_inference's device route against the reference's vectors
(tests/golden/predict_a13.npz), against its own torch route and, on the real tiny model, against a hand composition.  The merge
adds a pixel's windows in the reference's order and divides once (IEEE), so every comparison of the merge is bit equality."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slide_ref as R  # noqa: E402
from slide_ref import METAS, segmentor  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = dict(mode="slide", crop_size=(16, 24), stride=(11, 17))


def _groups(nw):
    return sorted({1, 2, 3, nw})


@pytest.mark.parametrize("case", list(R.GRIDS.values()), ids=list(R.GRIDS))
def test_slide_accumulate_is_the_reference_loop_bit_for_bit(case):
    """B in {1, 2} x K in {1, 5, 19} x groups of 1, 2, 3 and all windows at once; a -0.0 where one window alone covers the pixel (the
    reference's zero-filled map turns it into +0.0) and one mid-map; preds pre-filled with NaN: a stale value that was read, or a
    pixel that was not written, shows"""
    from spike2former_amd import ops
    H, W, crop, stride, (ny, nx, eh, ew) = case
    nw = ny * nx
    rng = np.random.default_rng(H * 1000 + W)
    for B in (1, 2):
        for K in (1, 5, 19):
            logits = rng.standard_normal((nw, B, K, eh, ew)).astype(np.float32) * 3
            logits[0, :, :, 0, 0] = -0.0
            logits[nw // 2, B - 1, K // 2, eh // 2, ew // 2] = -0.0
            want = R.bits(R.merge(logits, H, W, crop, stride))
            dev = torch.from_numpy(logits).cuda()
            for g in _groups(nw):
                preds = torch.full((B, K, H, W), float("nan"), device="cuda")
                for w0 in range(0, nw, g):
                    ops.slide_accumulate(preds, dev[w0:w0 + g], crop, stride, w0)
                got = R.bits(preds)
                assert np.array_equal(got, want), (B, K, g, int((got != want).sum()))


def test_slide_accumulate_touches_only_the_groups_pixels():
    """one group of the fixture grid: the pixels its windows do not cover keep their NaN, the others hold the running sum"""
    from spike2former_amd import ops
    H, W, crop, stride, (ny, nx, eh, ew) = R.GRIDS["fixture_3x3"]
    logits = torch.randn(2, 1, 2, eh, ew, generator=torch.Generator().manual_seed(3)).cuda()
    preds = torch.full((1, 2, H, W), float("nan"), device="cuda")
    ops.slide_accumulate(preds, logits, crop, stride, 0)
    wins = R.windows(H, W, crop, stride)[:2]
    covered = np.zeros((H, W), bool)
    for y1, y2, x1, x2 in wins:
        covered[y1:y2, x1:x2] = True
    assert np.array_equal(~np.isnan(preds.cpu().numpy()[0, 0]), covered)


@pytest.mark.parametrize("case", list(R.GRIDS.values()), ids=list(R.GRIDS))
def test_slide_windows_equals_torch_slicing(case):
    from spike2former_amd import ops
    H, W, crop, stride, (ny, nx, eh, ew) = case
    nw = ny * nx
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H + W)).cuda()
    wins = R.windows(H, W, crop, stride)
    for w0, n in {(0, nw), (nw // 3, max(1, nw // 2)), (nw - 1, 1)}:
        got = ops.slide_windows(x, crop, stride, w0, n)
        want = torch.stack([x[:, :, y1:y2, x1:x2] for y1, y2, x1, x2 in wins[w0:w0 + n]])
        assert got.shape == (n, 2, 3, eh, ew) and torch.equal(got, want), (w0, n)


@pytest.mark.parametrize("cfg,route", [(FIXTURE, None), (dict(FIXTURE, window_batch=4), None), (FIXTURE, "torch"),
                                       (dict(FIXTURE, window_batch=4), "torch")],
                         ids=["device", "device_batch4", "torch", "torch_batch4"])
def test_segmentor_on_the_fixture_vs_reference_vectors(golden, cfg, route):
    g = golden("predict_a13.npz")
    img, want = torch.from_numpy(g["i_img"]).cuda(), torch.from_numpy(g["slide_logits"])
    got = segmentor(cfg, 5, R.fake_net).slide_inference(img, [dict(x) for x in METAS], route=route).cpu()
    # the existing GPU bound (tests/test_a13_callers.py _check): the stand-in network's sin / einsum on the device
    assert (got - want).abs().max().item() <= 1e-5 * max(want.abs().max().item(), 1.0)


@pytest.mark.parametrize("g", [None, 1, 2, 4, 9, 16])
def test_device_route_is_the_torch_route_bit_for_bit(golden, g):
    img = torch.from_numpy(golden("predict_a13.npz")["i_img"]).cuda()
    cfg = FIXTURE if g is None else dict(FIXTURE, window_batch=g)
    want = segmentor(FIXTURE, 5, R.lin_net).slide_inference(img, [dict(x) for x in METAS], route="torch")
    calls = []
    got = segmentor(cfg, 5, R.lin_net, calls).inference(img, [dict(x) for x in METAS])
    assert got.is_cuda and np.array_equal(R.bits(got), R.bits(want))
    assert len(calls) == (9 if g is None else -(-9 // g))


@pytest.fixture(scope="module")
def tiny():
    import spike2former_amd as s2f
    from spike2former_amd.init_utils import seeded_init
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C1_64"))).cuda().eval()
    img = torch.randn(2, 3, 96, 112, generator=torch.Generator().manual_seed(7)).cuda()
    return model, img


def _metas():
    return [dict(img_shape=(96, 112), ori_shape=(96, 112), pad_shape=(96, 112), padding_size=[0, 0, 0, 0]) for _ in range(2)]


def test_tiny_model_window_batch_is_the_hand_composition(tiny):
    """window_batch = 4 on the 2 x 3 grid: groups of 4 and 2 windows, batches of 8 and 4.  The hand composition cuts the same groups
    with torch slicing, resets, runs model.encode_decode per group and merges with slide_ref: the same batches through the same
    kernels, so the test is about the composition (bit equality), not about the model's batch-invariance"""
    import spike2former_amd as s2f
    model, img = tiny
    crop, stride = (64, 64), (43, 43)
    model.test_cfg = dict(mode="slide", crop_size=crop, stride=stride, window_batch=4)
    wins = R.windows(96, 112, crop, stride)
    assert len(wins) == 6
    with torch.no_grad():
        s2f.reset_net(model)
        got = model.inference(img, _metas())
        parts = []
        for w0 in (0, 4):
            batch = torch.cat([img[:, :, y1:y2, x1:x2] for y1, y2, x1, x2 in wins[w0:w0 + 4]])
            s2f.reset_net(model)
            metas = _metas()
            metas[0]["img_shape"] = (64, 64)
            lg = model.encode_decode(batch, metas)
            parts.append(lg.view(-1, 2, *lg.shape[1:]).cpu().numpy())
    want = R.merge(np.concatenate(parts), 96, 112, crop, stride)
    assert got.is_cuda and got.dtype == torch.float32 and np.isfinite(want).all()
    assert np.array_equal(R.bits(got), R.bits(want))


def test_tiny_model_without_window_batch_is_the_torch_loop_membranes_carried(tiny):
    import spike2former_amd as s2f
    model, img = tiny
    model.test_cfg = dict(mode="slide", crop_size=(64, 64), stride=(43, 43))
    with torch.no_grad():
        s2f.reset_net(model)
        want = model.slide_inference(img, _metas(), route="torch")
        s2f.reset_net(model)
        got = model.inference(img, _metas())
    assert np.array_equal(R.bits(got), R.bits(want))


def test_tiny_model_predict_in_slide_mode(tiny):
    import spike2former_amd as s2f
    model, img = tiny
    model.test_cfg = dict(mode="slide", crop_size=(64, 64), stride=(43, 43), window_batch=4)
    with torch.no_grad():
        s2f.reset_net(model)
        res = model(img, mode="predict")
    K = s2f.WORKLOADS["C1_64"]["K"]
    assert len(res) == 2
    for r in res:
        assert r.seg_logits.data.shape == (K, 96, 112) and r.pred_sem_seg.data.shape == (1, 96, 112)
        assert torch.isfinite(r.seg_logits.data).all()
