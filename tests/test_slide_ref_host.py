"""CPU: the numpy restatement of sliding-window inference (tests/slide_ref.py) against the vectors the reference's own
slide_inference wrote (tests/golden/predict_a13.npz), ops.slide_grid, the coverage check, the argument rules of the two entry points
and EncoderDecoder.slide_inference's torch route with test_cfg['window_batch']."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slide_ref as R  # noqa: E402

METAS, segmentor = R.METAS, R.segmentor


def test_slide_ref_reproduces_the_reference_vectors(golden):
    g = golden("predict_a13.npz")
    want = g["slide_logits"]
    got = R.slide_ref(torch.from_numpy(g["i_img"]), R.fake_net, 5, (16, 24), (11, 17))
    assert got.shape == want.shape and got.dtype == np.float32
    # bit-exact on the host the vectors were generated on; on another SIMD level fake_net's sin / einsum round differently
    # (the bound of tests/test_a13_callers.py on the CPU)
    assert np.array_equal(got, want) or np.abs(got - want).max() <= 2e-6 * max(np.abs(want).max(), 1.0)


@pytest.mark.parametrize("case", list(R.GRIDS.values()) + [R.CITYSCAPES], ids=list(R.GRIDS) + ["cityscapes"])
def test_slide_grid(case):
    from spike2former_amd import ops
    H, W, crop, stride, want = case
    assert ops.slide_grid(H, W, crop, stride) == want
    assert len(R.windows(H, W, crop, stride)) == want[0] * want[1]


def test_slide_grid_refuses_non_positive_sizes():
    from spike2former_amd import ops
    with pytest.raises(ValueError):
        ops.slide_grid(16, 24, (16, 24), (0, 17))


def test_uncovered_grid_raises_before_any_window_runs():
    calls = []
    m = segmentor(dict(mode="slide", crop_size=(16, 24), stride=(20, 17)), 5, R.lin_net, calls)
    img = torch.zeros(1, 3, 40, 53)
    with pytest.raises(AssertionError):
        m.inference(img, [dict(METAS[0])])
    assert calls == []
    with pytest.raises(AssertionError):          # the numpy restatement asserts where the reference does: after its loop
        R.merge(np.zeros((9, 1, 1, 16, 24), np.float32), 40, 53, (16, 24), (20, 17))
    # stride > crop alone is no gap: 30 rows, the second (last) window is shifted back to row 14
    out = segmentor(dict(mode="slide", crop_size=(16, 24), stride=(20, 17)), 5, R.lin_net).inference(torch.zeros(1, 3, 30, 53),
                                                                                                   [dict(METAS[0])])
    assert out.shape == (1, 5, 30, 53)


@pytest.mark.parametrize("case", list(R.GRIDS.values()), ids=list(R.GRIDS))
def test_torch_route_without_window_batch_is_the_reference_loop(case):
    H, W, crop, stride, _ = case
    img = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H * W))
    got = segmentor(dict(mode="slide", crop_size=crop, stride=stride), 5, R.lin_net).inference(img, [dict(x) for x in METAS])
    assert np.array_equal(R.bits(got), R.bits(R.slide_ref(img, R.lin_net, 5, crop, stride)))


@pytest.mark.parametrize("g", [1, 2, 4, 9, 16])
def test_window_batch_on_the_torch_route(golden, g):
    """window_batch = g: ceil(9 / g) calls of encode_decode with window-major batches of g B (the last one smaller), the result bit
    for bit that of the route without window_batch"""
    img = torch.from_numpy(golden("predict_a13.npz")["i_img"])
    B = img.shape[0]
    cfg = dict(mode="slide", crop_size=(16, 24), stride=(11, 17))
    want = segmentor(cfg, 5, R.lin_net).inference(img, [dict(x) for x in METAS])
    calls = []
    got = segmentor(dict(cfg, window_batch=g), 5, R.lin_net, calls).inference(img, [dict(x) for x in METAS])
    assert np.array_equal(R.bits(got), R.bits(want))
    sizes = [min(g, 9 - w0) * B for w0 in range(0, 9, g)]
    assert len(calls) == -(-9 // g)
    assert calls == [((s, 3, 16, 24), (16, 24)) for s in sizes]


def test_window_batch_must_be_a_positive_integer():
    for bad in (0, -1, 1.5):
        m = segmentor(dict(mode="slide", crop_size=(16, 24), stride=(11, 17), window_batch=bad), 5, R.lin_net)
        with pytest.raises(ValueError):
            m.inference(torch.zeros(1, 3, 37, 53), [dict(METAS[0])])


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """nulls, sizes, a group outside the grid and alignment: S2F_EINVAL / S2F_EALIGN before any launch, so no GPU is needed"""
    from spike2former_amd._lib import lib
    P = 1 << 20          # an aligned dummy address: never dereferenced on the host
    ok = dict(B=2, C=5, H=37, W=53, ch=16, cw=24, sh=11, sw=17, w0=0, n=9)
    for fn in (lib.s2f_slide_windows, lib.s2f_slide_accumulate):
        def call(a=P, b=P, **kw):
            v = dict(ok, **kw)
            return fn(a, b, v["B"], v["C"], v["H"], v["W"], v["ch"], v["cw"], v["sh"], v["sw"], v["w0"], v["n"], None)
        assert call(a=None) == -1 and b"null" in lib.s2f_last_error()
        assert call(b=None) == -1
        for bad in (dict(B=0), dict(C=0), dict(H=0), dict(W=-3), dict(ch=0), dict(cw=0), dict(sh=0), dict(sw=-1), dict(w0=-1), dict(n=0),
                    dict(w0=8, n=2), dict(w0=9, n=1), dict(B=256, C=256), dict(H=65536)):
            assert call(**bad) == -1, bad
        assert call(a=P + 2) == -2 and call(b=P + 1) == -2          # S2F_EALIGN
