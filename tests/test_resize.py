"""csrc/resize.hip: the general bilinear resize (forward against F.interpolate in fp32 and fp64, its gather adjoint), the post-processing
arg-max / threshold and the test-time-augmentation accumulator -- and SegTTAModel.merge_preds on the host against a literal
restatement of mmseg segmentors/seg_tta.py:14-48."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("s2f_resize_fwd", "s2f_resize_bwd_add", "s2f_seg_argmax", "s2f_tta_accumulate", "s2f_tta_finish")


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_resize_symbols_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "s2f.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "spike2former_amd", "libs2f_hip.so"))
    from spike2former_amd import _lib
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


def test_resize_argument_errors_without_a_gpu():
    from spike2former_amd._lib import lib
    p = ctypes.c_void_p(16)           # never dereferenced: validation fails before any launch
    assert lib.s2f_resize_fwd(None, p, 1, 16, 4, 0, 0, 4, 4, 8, 8, 0, None) == -1
    assert b"null" in lib.s2f_last_error()
    assert lib.s2f_resize_fwd(p, p, 1, 16, 4, 0, 0, 4, 4, 0, 8, 0, None) == -1            # H == 0
    assert lib.s2f_resize_fwd(p, p, 1, 16, 4, 0, 1, 4, 4, 8, 8, 0, None) == -1            # window wider than the row
    assert b"window" in lib.s2f_last_error()
    assert lib.s2f_resize_fwd(p, p, 1, 16, 4, 0, 0, 4, 4, 8, 8, 16, None) == -1           # unknown flag
    assert lib.s2f_resize_bwd_add(p, None, None, 1, 4, 4, 8, 8, 0, None) == -1
    assert lib.s2f_resize_bwd_add(p, None, p, 1, 4, 4, 8, 8, 4, None) == -1               # flips have no adjoint here
    assert lib.s2f_seg_argmax(p, None, None, 3, 16, 0, 0.3, None) == -1
    assert lib.s2f_seg_argmax(p, None, p, 3, 16, 0, 0.3, None) == -1                      # float labels: one class only
    assert lib.s2f_tta_accumulate(p, p, 3, 16, 4, 0, 0, 5, 4, 8, 8, 0, 1, None) == -1     # window taller than the plane
    assert lib.s2f_tta_finish(p, p, None, 3, 16, 0, 0.3, None) == -1                      # no views


class _Sample:
    def __init__(self, logits, gt=None, img_path=None):
        from spike2former_amd.data_preprocessor import PixelData
        self.seg_logits = PixelData(logits)
        self.metainfo = dict(img_path=img_path)
        if gt is not None:
            self.gt_sem_seg = PixelData(gt)

    def set_metainfo(self, m):
        self.metainfo.update(m)


def _reference_merge(data_samples, out_channels, threshold):
    """seg_tta.py:27-40, line for line (the merged label map before PixelData's 2-D -> [1, H, W])"""
    seg_logits = data_samples[0].seg_logits.data
    logits = torch.zeros(seg_logits.shape).to(seg_logits)
    for data_sample in data_samples:
        seg_logit = data_sample.seg_logits.data
        if out_channels > 1:
            logits += seg_logit.softmax(dim=0)
        else:
            logits += seg_logit.sigmoid()
    logits /= len(data_samples)
    if out_channels == 1:
        seg_pred = (logits > threshold).to(logits).squeeze(1)
    else:
        seg_pred = logits.argmax(dim=0)
    return seg_pred


def _tta(K, threshold=0.3):
    import types

    from spike2former_amd.tta import SegTTAModel
    module = types.SimpleNamespace(out_channels=K, decode_head=types.SimpleNamespace(threshold=threshold))
    m = object.__new__(SegTTAModel)
    torch.nn.Module.__init__(m)
    m.__dict__["module"] = module
    return m


@pytest.mark.parametrize("K", [5, 1])
def test_merge_preds_cpu_is_seg_tta(K):
    g = torch.Generator().manual_seed(K)
    imgs = []
    for b in range(2):
        views = [_Sample(torch.randn(K, 6, 7, generator=g) * 3, gt=torch.full((1, 6, 7), b) if b == 0 else None,
                         img_path=f"img{b}_view{v}.png") for v in range(3)]
        imgs.append(views)
    want = [_reference_merge(v, K, 0.3) for v in imgs]
    last_logits = [v[-1].seg_logits.data for v in imgs]
    out = _tta(K).merge_preds(imgs)
    assert len(out) == 2
    for b, d in enumerate(out):
        assert d is imgs[b][-1]                                  # the merged sample is the LAST view's ...
        assert d.seg_logits.data is last_logits[b]               # ... with its seg_logits (the reference's quirk)
        assert d.metainfo["img_path"] == f"img{b}_view0.png"     # img_path and gt_sem_seg: the first view's
        assert hasattr(d, "gt_sem_seg") == (b == 0)
        got = d.pred_sem_seg.data
        assert got.shape == (1, 6, 7) and got.dtype == want[b].dtype
        assert torch.equal(got.reshape(want[b].shape), want[b])


# ------------------------------------------------------------------------------------------------------------------ GPU
def _ref(x, size, align, flip=None, crop=None, sigmoid=False, dtype=torch.float64):
    x = x.to(dtype)
    if crop is not None:
        t, b, l, r = crop
        x = x[..., t:x.shape[-2] - b, l:x.shape[-1] - r]
    if flip == "horizontal":
        x = x.flip(-1)
    elif flip == "vertical":
        x = x.flip(-2)
    y = F.interpolate(x[None] if x.dim() == 3 else x, size=size, mode="bilinear", align_corners=align)
    y = y[0] if x.dim() == 3 else y
    return y.sigmoid() if sigmoid else y


def _close(got, want64, want32):
    """against the fp64 resize: no farther than ATen's own fp32 resize is, + 2e-6 of the maximum.  At a ratio that is not a power
    of two the fp32 source index is itself rounded (up to ~2.7e-5 of the maximum here, in ATen as in this kernel), so a plain 2e-6
    bound against fp64 holds for no fp32 implementation; and ATen's ROCm build contracts src = scale * (o + 0.5) - 0.5 into an FMA
    where this kernel keeps the two roundings of upsample.hip::taps, so the two fp32 results round at different pixels."""
    m = max(want64.abs().max().item(), 1.0)
    d64 = (got.double() - want64).abs().max().item()
    ref = (want32.double() - want64).abs().max().item()
    return d64 <= ref + 2e-6 * m, (d64, ref, m)


SIZES = [((1, 1), (1, 1)), ((1, 1), (3, 5)), ((5, 7), (9, 13)), ((128, 171), (256, 342)), ((86, 86), (171, 171)),
         ((64, 86), (128, 171)), ((32, 43), (64, 86)), ((40, 60), (20, 30)), ((40, 60), (30, 45)), ((33, 49), (17, 25)),
         ((16, 24), (32, 48)), ((3, 4), (1, 1))]


@pytest.mark.gpu
@pytest.mark.parametrize("src,dst", SIZES)
@pytest.mark.parametrize("align", [False, True])
def test_resize_forward_matches_interpolate(src, dst, align):
    from spike2former_amd import ops
    x = torch.randn(6, 2, *src, generator=torch.Generator().manual_seed(src[0] * 7 + dst[1])).cuda()
    want, want32 = _ref(x, dst, align), _ref(x, dst, align, dtype=torch.float32)
    got = ops.resize_bilinear(x, dst, align_corners=align)
    assert got.shape == want.shape
    ok, why = _close(got, want, want32)
    assert ok, why
    if not align:
        ok, why = _close(ops.upsample_bilinear(x, dst), want, want32)
        assert ok, why
    with torch.no_grad():
        s = ops.resize_bilinear(x, dst, align_corners=align, sigmoid=True)
    ok, why = _close(s, want.sigmoid(), want32.sigmoid())
    assert ok, why


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [None, "horizontal", "vertical"])
@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("sigmoid", [False, True])
def test_resize_window_crop_and_flip(flip, align, sigmoid):
    from spike2former_amd import ops
    x = torch.randn(7, 37, 53, generator=torch.Generator().manual_seed(11)).cuda()
    crop = (1, 3, 2, 5)                       # top, bottom, left, right
    for size in ((30, 41), (64, 96), (17, 23)):
        want, want32 = _ref(x, size, align, flip, crop, sigmoid), _ref(x, size, align, flip, crop, sigmoid, torch.float32)
        got = ops.resize_window(x, size, crop=crop, flip=flip, align_corners=align, sigmoid=sigmoid)
        ok, why = _close(got, want, want32)
        assert ok, (size, why)


@pytest.mark.gpu
def test_exact_2x_even_width_dispatch_is_the_2x_kernel():
    from spike2former_amd import ops
    from spike2former_amd._lib import lib
    x = torch.randn(3, 8, 20, 34, generator=torch.Generator().manual_seed(3)).cuda()
    ref = torch.empty(3, 8, 40, 68, device="cuda")
    ops.check(lib.s2f_upsample2x_fwd(x.data_ptr(), ref.data_ptr(), 24, 20, 34, ops._stream()), "s2f_upsample2x_fwd")
    assert torch.equal(ops.upsample_bilinear(x, (40, 68)), ref)
    # the general kernel at scale 0.5 is the same arithmetic: bit for bit
    assert torch.equal(ops.resize_bilinear(x, (40, 68)), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("src,dst", [((5, 7), (9, 13)), ((33, 49), (66, 98)), ((64, 86), (128, 171)), ((40, 60), (30, 45)),
                                     ((1, 1), (4, 6)), ((9, 13), (17, 25))])
@pytest.mark.parametrize("align", [False, True])
def test_resize_adjoint(src, dst, align):
    from spike2former_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, *src, generator=g).cuda()
    gy = torch.randn(2, 3, *dst, generator=g).cuda()
    add = torch.randn(2, 3, *src, generator=g).cuda()
    xd = x.double().requires_grad_()
    F.interpolate(xd, size=dst, mode="bilinear", align_corners=align).backward(gy.double())
    want = xd.grad
    x32 = x.clone().requires_grad_()
    F.interpolate(x32, size=dst, mode="bilinear", align_corners=align).backward(gy)
    runs = []
    for _ in range(2):
        xr = x.clone().requires_grad_()
        ops.resize_bilinear(xr, dst, align_corners=align).backward(gy)
        runs.append(xr.grad.clone())
    ok, why = _close(runs[0], want, x32.grad)
    assert ok, why
    assert torch.equal(runs[0], runs[1])                                   # no atomics: bit-repeatable
    # the pass-through port: a second reader's gradient summed inside the adjoint kernel
    xr = x.clone().requires_grad_()
    y, through = ops.resize_bilinear(xr, dst, align_corners=align, skip=True)
    torch.autograd.backward([y, through], [gy, add])
    assert torch.equal(xr.grad, runs[0] + add)


def _ref_softmax_mean(views, K):
    acc = torch.zeros_like(views[0], dtype=torch.float64)
    for v in views:
        acc += v.double().softmax(0) if K > 1 else v.double().sigmoid()
    return acc / len(views)


def _labels_ok(got, prob):
    """labels equal to prob's arg-max except where the top-two margin is at most 1e-6"""
    want = prob.argmax(0)
    top2 = prob.topk(2, dim=0).values
    ok = (got.reshape(want.shape).cpu() == want.cpu()) | ((top2[0] - top2[1]) <= 1e-6).cpu()
    return bool(ok.all())


@pytest.mark.gpu
def test_seg_argmax_ties_nan_and_threshold():
    from spike2former_amd import ops
    x = torch.randn(9, 21, 30, generator=torch.Generator().manual_seed(9)).cuda()
    x[4, 0, :5] = 100.0
    x[7, 0, :5] = 100.0                            # a tie: the lowest index wins
    x[3, 1, 0] = float("nan")
    x[6, 1, 0] = float("nan")                      # NaN counts as the maximum, the first one wins
    x[:, 2, 0] = 1.0                               # all equal: index 0
    got = ops.seg_argmax(x)
    assert got.dtype == torch.int64 and got.shape == (1, 21, 30)
    assert torch.equal(got[0], x.argmax(0))
    assert got[0, 0, 0].item() == 4 and got[0, 1, 0].item() == 3 and got[0, 2, 0].item() == 0
    one = torch.randn(1, 21, 30, generator=torch.Generator().manual_seed(2)).cuda()
    f = ops.seg_argmax(one.sigmoid(), 0.3, float_out=True)
    assert f.dtype == torch.float32 and torch.equal(f, (one.sigmoid() > 0.3).float())


@pytest.mark.gpu
@pytest.mark.parametrize("K", [150, 4, 1])
def test_tta_accumulate_and_finish(K):
    from spike2former_amd import ops
    g = torch.Generator().manual_seed(K)
    ori = (30, 41)
    specs = [((37, 53), (1, 3, 2, 5), None), ((37, 53), (1, 3, 2, 5), "horizontal"), ((19, 27), (0, 2, 0, 1), None),
             ((19, 27), (0, 2, 0, 1), "vertical")]
    xs = [torch.randn(K, *shape, generator=g).cuda() * 4 for shape, _, _ in specs]
    # the views resized in fp32 by ops.resize_window (the resize is judged above), then the softmax / sigmoid and mean in fp64
    from spike2former_amd import ops as o
    views = [o.resize_window(x, ori, crop=crop, flip=flip, sigmoid=K == 1) for x, (_, crop, flip) in zip(xs, specs)]
    want = _ref_softmax_mean(views, K)
    acc = torch.empty(K, *ori, device="cuda")
    for n, (x, (_, crop, flip)) in enumerate(zip(xs, specs)):
        ops.tta_accumulate(acc, x, n == 0, crop=crop, flip=flip, pre_sigmoid=K == 1)
    lab = ops.tta_finish(acc, len(xs), 0.3)
    assert (acc.double() - want).abs().max().item() <= 1e-6
    assert lab.shape == (1, *ori)
    if K > 1:
        assert lab.dtype == torch.int64 and _labels_ok(lab, want)
    else:
        margin = (want - 0.3).abs() <= 1e-6
        assert lab.dtype == torch.float32
        assert bool(((lab.cpu() == (want > 0.3).float().cpu()) | margin.cpu()).all())
    # ties in the mean resolve to the lowest index
    if K > 1:
        same = torch.zeros(K, 4, 4, device="cuda")
        acc = torch.empty(K, 4, 4, device="cuda")
        ops.tta_accumulate(acc, same, True)
        assert torch.equal(ops.tta_finish(acc, 1, 0.3), torch.zeros(1, 4, 4, dtype=torch.int64, device="cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [6, 1])
def test_merge_preds_gpu_is_the_host_restatement(K):
    g = torch.Generator().manual_seed(40 + K)
    views = [[_Sample(torch.randn(K, 13, 17, generator=g).cuda() * 3) for _ in range(3)]]
    prob = _ref_softmax_mean([v.seg_logits.data for v in views[0]], K)
    got = _tta(K).merge_preds(views)[0].pred_sem_seg.data
    assert got.shape == (1, 13, 17)
    if K > 1:
        assert got.dtype == torch.int64 and _labels_ok(got, prob)
    else:
        margin = ((prob - 0.3).abs() <= 1e-6).cpu()
        assert bool(((got.cpu() == (prob > 0.3).float().cpu()) | margin).all())
