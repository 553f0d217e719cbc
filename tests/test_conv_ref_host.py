"""tests/conv_ref.py against what it restates, on the host: the closed forms against autograd of F.conv2d in fp64 (the bordered
depthwise form against F.conv2d on the explicitly padded tensor), and abs_sums against the same operations on absolute values."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref  # noqa: E402


def _r(g, *s):
    return torch.randn(*s, generator=g, dtype=torch.float64)


def _close(a, b):
    return a.shape == b.shape and torch.allclose(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("k,stride,pad,H,W", [(3, 1, 1, 6, 7), (3, 2, 1, 9, 8), (3, 2, 1, 6, 7), (7, 2, 3, 11, 12), (7, 1, 3, 8, 9),
                                              (5, 1, 2, 6, 5)])
def test_dense_closed_forms_equal_autograd_of_conv2d(k, stride, pad, H, W, with_bias):
    N, C, M = 2, 3, 4
    g = torch.Generator().manual_seed(10 * k + stride)
    x, w, bias = _r(g, N, C, H, W), _r(g, M, C, k, k), (_r(g, M) if with_bias else None)
    leaves = [t.clone().requires_grad_(True) for t in (x, w)] + ([bias.clone().requires_grad_(True)] if with_bias else [])
    y = F.conv2d(leaves[0], leaves[1], leaves[2] if with_bias else None, stride, pad)
    gy = _r(g, *y.shape)
    y.backward(gy)
    got = conv_ref.conv_dense(x, w, bias, stride, pad, gy)
    assert _close(got["y"], y.detach()) and _close(got["dx"], leaves[0].grad) and _close(got["dw"], leaves[1].grad)
    if with_bias:
        assert _close(got["db"], leaves[2].grad)
    else:
        assert got["db"] is None
    fwd = conv_ref.conv_dense(x, w, bias, stride, pad, None)
    assert torch.equal(fwd["y"], got["y"]) and fwd["dx"] is None and fwd["dw"] is None and fwd["db"] is None
    # the fp32 evaluation is the same association in the narrower type
    assert all(v is None or v.dtype == torch.float32 for v in conv_ref.conv_dense(x, w, bias, stride, pad, gy, torch.float32).values())


@pytest.mark.parametrize("with_border", [True, False])
@pytest.mark.parametrize("K,pad", [(K, p) for K in (3, 5, 7) for p in (0, (K - 1) // 2, K - 1)])
def test_depthwise_closed_forms_equal_autograd_of_conv2d_on_the_padded_tensor(K, pad, with_border):
    N, C, H, W = 2, 3, 9, 8
    g = torch.Generator().manual_seed(10 * K + pad)
    x, w, border = _r(g, N, C, H, W), _r(g, C, 1, K, K), (_r(g, C) if with_border else None)
    xl, wl = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    if with_border:
        # BNAndPadLayer: the ring holds the channel's constant, the interior is x itself
        xp = border.view(1, C, 1, 1).expand(N, C, H + 2 * pad, W + 2 * pad).clone()
        xp[:, :, pad:pad + H, pad:pad + W] = xl
        y = F.conv2d(xp, wl, None, 1, 0, 1, C)
    else:
        y = F.conv2d(xl, wl, None, 1, pad, 1, C)
    gy = _r(g, *y.shape)
    y.backward(gy)
    got = conv_ref.dwconv(x, w, pad, border, gy)
    assert tuple(got["y"].shape) == (N, C, H + 2 * pad - K + 1, W + 2 * pad - K + 1)
    assert _close(got["y"], y.detach()) and _close(got["dx"], xl.grad) and _close(got["dw"], wl.grad)
    fwd = conv_ref.dwconv(x, w, pad, border, None)
    assert torch.equal(fwd["y"], got["y"]) and fwd["dx"] is None and fwd["dw"] is None
    assert all(v.dtype == torch.float32 for v in conv_ref.dwconv(x, w, pad, border, gy, torch.float32).values())
    if with_border and pad:
        # the ring matters: without the border the outputs next to the edge differ
        assert not _close(conv_ref.dwconv(x, w, pad, None, gy)["y"], got["y"])


def test_abs_sums_equal_the_same_operations_on_absolute_values():
    g = torch.Generator().manual_seed(5)
    x, w, bias, gy = _r(g, 2, 3, 6, 7), _r(g, 4, 3, 3, 3), _r(g, 4), _r(g, 2, 4, 3, 4)
    a = conv_ref.abs_sums(conv_ref.conv_dense, x.float(), w.float(), bias.float(), 2, 1, gy.float())
    xa, wa, ba, ga = (t.float().double().abs() for t in (x, w, bias, gy))
    xl, wl, bl = (t.clone().requires_grad_(True) for t in (xa, wa, ba))
    y = F.conv2d(xl, wl, bl, 2, 1)
    y.backward(ga)
    assert set(a) == {"y", "dx", "dw", "db"}
    assert _close(a["y"], y.detach()) and _close(a["dx"], xl.grad) and _close(a["dw"], wl.grad) and _close(a["db"], bl.grad)
    assert all(v.dtype == torch.float64 and (v >= 0).all() for v in a.values())
    # every entry bounds the signed one
    s = conv_ref.conv_dense(x.float(), w.float(), bias.float(), 2, 1, gy.float())
    assert all((s[k].abs() <= a[k] * (1 + 1e-12) + 1e-12).all() for k in a)
    assert conv_ref.abs_sums(conv_ref.conv_dense, x, w, None, 2, 1, gy)["db"] is None

    x, w, border, gy = _r(g, 2, 3, 6, 7), _r(g, 3, 1, 5, 5), _r(g, 3), _r(g, 2, 3, 10, 11)
    a = conv_ref.abs_sums(conv_ref.dwconv, x, w, 4, border, gy)
    xa, wa, ra, ga = (t.abs() for t in (x, w, border, gy))
    xl, wl = xa.clone().requires_grad_(True), wa.clone().requires_grad_(True)
    xp = ra.view(1, 3, 1, 1).expand(2, 3, 14, 15).clone()
    xp[:, :, 4:10, 4:11] = xl
    y = F.conv2d(xp, wl, None, 1, 0, 1, 3)
    y.backward(ga)
    assert set(a) == {"y", "dx", "dw"}
    assert _close(a["y"], y.detach()) and _close(a["dx"], xl.grad) and _close(a["dw"], wl.grad)
