"""GPU: the integers s2f_firing_map writes and the bytes s2f_firing_draw writes against tests/firingmap_ref.py (the numpy int64
restatement).  Equality everywhere -- both sides are integer arithmetic; outputs are slices / windows of sentinel-filled buffers whose
other bytes must stay untouched.  STRICT, no fall-back."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import firingmap_cases as K  # noqa: E402
import firingmap_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def run_map(x, host, B, D, off, assign_first=True, again=None):
    """x [TB, C, P] at element offset `off` of a larger device buffer, stats a slice of a sentinel buffer -> asserts the planes (and,
    with again=(tensor, host), the accumulated and the overwritten planes) and the sentinels"""
    from spike2former_amd import ops
    assert ops.STRICT
    before = dict(ops.FALLBACKS)
    P = x.shape[2]
    big, stats = K.sentinel_stats(B, P, "cuda")
    if not assign_first:
        stats.zero_()
    ops.firing_map(K.at_offset(x, off, "cuda"), B, D, stats, assign=assign_first)
    want = R.firing_map(host, B, D)
    got = big.cpu().numpy()
    assert (got[:3] == -123456789).all() and (got[3 + 4 * B * P:] == -123456789).all(), "words outside stats were written"
    body = got[3:3 + 4 * B * P].reshape(B, 4, P)
    assert np.array_equal(body, want), f"{int((body != want).sum())} of {want.size} words differ"
    if again is not None:
        y, host2 = again
        yd = K.at_offset(y, (off + 1) % 4, "cuda")
        ops.firing_map(yd, B, D, stats)
        assert np.array_equal(stats.cpu().numpy(), R.firing_map(host2, B, D, stats=want)), "second call did not accumulate"
        ops.firing_map(yd, B, D, stats, assign=True)
        assert np.array_equal(stats.cpu().numpy(), R.firing_map(host2, B, D)), "ASSIGN did not overwrite"
    assert dict(ops.FALLBACKS) == before


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("P", K.MAP_P)
def test_shapes_offsets_and_dtypes(P, bf16):
    """every C, (TB, B) and element offset 0 .. 3 at this P; D cycles through 4, 8, 3"""
    n = 0
    for C in K.MAP_C:
        for TB, B in K.MAP_TB_B:
            for off in range(4):
                D = K.MAP_D[n % len(K.MAP_D)]
                x, host = K.spike_map(TB, C, P, D, seed=1000 * P + n, bf16=bf16)
                run_map(x, host, B, D, off, assign_first=bool(n % 2))
                n += 1


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("TB,B,C,P", K.MAP_ENDS)
def test_both_ends_of_the_split_rule(TB, B, C, P, bf16):
    """many pixels of few planes (tiles of 256 lanes, one slice) and few pixels of 640 channels (16 lanes x 16 slices, the partials
    combined in LDS), wide and scalar; two calls accumulate, ASSIGN overwrites, plane 2 is a running maximum"""
    x, host = K.spike_map(TB, C, P, 8, seed=P + C, bf16=bf16)
    run_map(x, host, B, 8, 0, again=K.spike_map(TB, C, P, 8, seed=P + C + 1, bf16=bf16))


def test_two_runs_give_the_same_bits():
    from spike2former_amd import ops
    x, _ = K.spike_map(4, 640, 256, 8, seed=5)
    xd = x.cuda()
    a = ops.firing_map(xd, 2, 8, torch.empty(2, 4, 256, dtype=torch.int32, device="cuda"), assign=True)
    b = ops.firing_map(xd, 2, 8, torch.empty(2, 4, 256, dtype=torch.int32, device="cuda"), assign=True)
    assert torch.equal(a, b)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("D", K.MAP_D)
def test_every_value_in_its_plane(D, bf16):
    """every level 0 .. D and -0.0, 0.3, -1/D, 65536/D, a subnormal, NaN, +-inf, 65535/D, one pixel each: the planes by hand for fp32
    (tests/test_firing_maps_host.py checks the restatement against the same table), the restatement for both dtypes"""
    from spike2former_amd import ops
    sp = K.specials(D)
    levels = np.arange(D + 1, dtype=np.float32) / np.float32(D)
    x = torch.from_numpy(np.concatenate([sp, levels]).astype(np.float32)[None, None])
    if bf16:
        x = x.to(torch.bfloat16)
        host = x.view(torch.int16).numpy().view(np.uint16)
    else:
        host = x.numpy()
    for off in range(4):
        stats = torch.empty(1, 4, x.shape[2], dtype=torch.int32, device="cuda")
        ops.firing_map(K.at_offset(x, off, "cuda"), 1, D, stats, assign=True)
        got = stats.cpu().numpy()
        assert np.array_equal(got, R.firing_map(host, 1, D)), off
        if not bf16:
            n_sp = len(sp)
            assert got[0, 1, 0] == 0 and (got[0, 1, 1:n_sp] == 1).all() and got[0, 3, 0] == 0 and (got[0, 3, 1:n_sp - 1] == 1).all()
            assert got[0, 0, n_sp - 1] == got[0, 2, n_sp - 1] == 65535 and got[0, 3, n_sp - 1] == 0
            assert np.array_equal(got[0, 0, n_sp:], np.arange(D + 1)) and np.array_equal(got[0, 2, n_sp:], np.arange(D + 1))
            assert (got[0, 3, n_sp:] == 0).all() and (got[0, 0, :n_sp - 1] == 0).all()


# ------------------------------------------------------------------------------------------------ s2f_firing_draw
@pytest.mark.parametrize("hw,HW", K.DRAW_SIZES)
def test_draw_bytes_and_sentinels(hw, HW):
    """every a8, four `full` (1, the plane's maximum, twice and a third of it: the last saturates at row 255), RGB and BGR; the window
    at byte offsets 1, 2, 3 with rows 3 W + 5 bytes apart: the sentinels left, right, above and below stay"""
    from spike2former_amd import ops
    from spike2former_amd.visualization import SegLocalVisualizer
    assert ops.STRICT
    before = dict(ops.FALLBACKS)
    (h, w), (H, W) = hw, HW
    rng = np.random.default_rng(h * 31 + W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    plane = K.draw_plane(h, w, seed=H + w)          # (has a negative entry where there is room: counts as 0)
    top = int(plane.max())
    lut = SegLocalVisualizer.default_firing_lut()
    # the picture itself at an odd byte offset, too
    img_d = K.at_offset(torch.from_numpy(img), 1, "cuda")
    plane_d, lut_d = torch.from_numpy(plane).cuda(), K.at_offset(torch.from_numpy(lut), 3, "cuda")
    n = 0
    for a8 in K.DRAW_A8:
        for full in (1, top, 2 * top, max(1, top // 3)):
            for bgr in (False, True):
                off = 1 + n % 3
                n += 1
                big, out, _ = K.draw_window(H, W, off, "cuda")
                assert ops.firing_draw(img_d, plane_d, full, lut_d, a8 / 256, bgr=bgr, out=out) is out
                want = K.expect_window(H, W, off, R.firing_draw(img, plane, full, lut, a8, bgr))
                got = big.cpu().numpy()
                assert np.array_equal(got, want), (a8, full, bgr, off, f"{int((got != want).sum())} of {want.size} bytes differ")
    if top // 3 >= 1:
        assert R.firing_index(plane, max(1, top // 3), H, W).max() == 255
    assert dict(ops.FALLBACKS) == before


def test_draw_allocates_a_contiguous_out():
    from spike2former_amd import ops
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (9, 300, 3), dtype=np.uint8)
    plane = K.draw_plane(4, 7, seed=1)
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    got = ops.firing_draw(torch.from_numpy(img).cuda(), torch.from_numpy(plane).cuda(), 600, torch.from_numpy(lut).cuda(), 0.5)
    assert got.is_cuda and got.is_contiguous() and np.array_equal(got.cpu().numpy(), R.firing_draw(img, plane, 600, lut, 128))


def test_draw_large_values_do_not_overflow():
    """plane values and `full` near 2^31 - 1 (the restatement itself is checked against unbounded integers on the host)"""
    from spike2former_amd import ops
    top = 2 ** 31 - 1
    plane = np.array([[top, top - 1, 0], [top // 2, -top, top]], np.int32)
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (5, 9, 3), dtype=np.uint8)
    lut = np.stack([np.arange(256, dtype=np.uint8)] * 3, 1)
    for full in (top, top - 5, top // 2):
        got = ops.firing_draw(torch.from_numpy(img).cuda(), torch.from_numpy(plane).cuda(), full, torch.from_numpy(lut).cuda(), 1.0)
        assert np.array_equal(got.cpu().numpy(), R.firing_draw(img, plane, full, lut, 256)), full
        got = ops.firing_draw(torch.from_numpy(img).cuda(), torch.from_numpy(plane).cuda(), full, torch.from_numpy(lut).cuda(), 0.3)
        assert np.array_equal(got.cpu().numpy(), R.firing_draw(img, plane, full, lut, 77)), full
