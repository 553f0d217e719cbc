"""The HIP kernels of the Hungarian-matched loss -- ops.mask_loss_sums (csrc/upsample.hip s2f_mask_loss_fwd/bwd), ops.mask_loss_seg
(csrc/maskloss.hip s2f_mask_loss_seg_fwd/bwd) and ops.mask_cost_bins (csrc/maskloss.hip) -- each against the plain fp64 reference
tests/loss_ref.py (itself checked on the CPU in tests/test_loss_ref_host.py), at the shapes, logits and hyper-parameters where
they can go wrong: every tap clamped, odd heights, w % 4 == 2, one and several backward tiles with remainders, forward chunks cut
in mid-row, logits past the underflow of exp(-|u|), gamma != 2 (the pow routes, pt == 0 exactly), one output weight at a time.

Bounds (none of them comes from what the kernels give):
  * the four sums: 1e-5 relative to fp64 (all four are sums of non-negative terms; ATen's fp32 evaluation of the same expression
    stays below 3e-7 on these inputs); sum t is an integer below 2^24 and must be exact, sum s t of an all-zero target exactly 0;
  * gradients, per prediction row: largest absolute error <= 1e-5 of the row's largest fp64 gradient (ATen fp32: 1.2e-6 at most);
  * rows without a match: sums and gradients exactly 0;
  * uniformly confident rows (|u| in 8..15 with the sign of a constant target): every term hangs on 1 - s = e^-|u|, which ATen's
    own fp32 evaluation only knows to 1e-4 .. 1e-3 (cancellation), so the bound there is max(1e-5, 4 x the error of an ATen fp32
    CPU evaluation of the same input against fp64), computed in the test from the reference;
  * cost bins: |got - want| <= 2e-5 x the bin's absolute-term sum + hw 2^-32 (2e-5 is the project's figure for the costs; the
    kernel rounds every term to a multiple of 2^-32 before its integer sums, at most half a quantum each for pos and neg)."""
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2),        # the smallest legal map: every tap clamped
          (3, 6),        # odd h, w % 4 == 2
          (8, 64),       # exactly one backward tile of the label-map kernel
          (9, 66),       # one row and two columns into the next tiles
          (17, 130),     # three tiles in x (remainder 2), three in y (remainder 1)
          (50, 62)]      # 3100 quads: 2 forward chunks of 1550 cut in mid-row, 4 backward chunks of the gathered kernel
HYPER = [(1.0, 0.6), (1.5, 0.25), (2.0, 0.25), (2.0, 0.6), (3.0, 0.25)]          # (gamma, alpha); gamma >= 1: below, ATen's own
LOGITS = ["regular", "saturated", "confident"]                                  # gradient is not finite at pt == 0
ONE_HOT = torch.eye(4, dtype=torch.float64)
FLT_MIN = 2.0 ** -126


def _ids(v):
    return "x".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _logits(kind, shape, g, sign=None, pin=False):
    """regular: N(0, 3).  saturated: half N(0, 3), half {0, +/-20, +/-50, +/-90, +/-120} + N(0, 1) -- across the underflow of
    exp(-|u|) in fp32 (|u| > 87) and of 1 - s (u > 17).  confident: |u| uniform in 8..15, sign[row] given by the caller.
    pin (maps [..., h, w]): the four corner logits of every map are N(0, 1/2).  The corner pixels of the up-sampled map have all
    their taps clamped onto them, so every row has undecided pixels there, and the targets below put a pixel of every non-empty
    target on a corner.  Without that a 1 x 2 or 3 x 6 map of these two classes is now and then confident in every pixel (of its
    target) by chance, and such a row belongs to the third class: its sums and d(sum s t) are made of 1 - s alone, which ATen's
    fp32 evaluation itself misses by far more than 1e-5 (measured on the CPU: up to 1e-2, and 1 for the gradient)."""
    if kind == "confident":
        return (8 + 7 * torch.rand(shape, generator=g)) * sign
    u = torch.randn(shape, generator=g) * 3
    if kind == "saturated":
        levels = torch.tensor([0., 20., -20., 50., -50., 90., -90., 120., -120.])
        big = levels[torch.randint(0, 9, shape, generator=g)] + torch.randn(shape, generator=g)
        u = torch.where(torch.rand(shape, generator=g) < 0.5, big, u)
    if pin:
        for i, j in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
            u[..., i, j] = torch.randn(shape[:-2], generator=g) * 0.5
    return u


def _region_map(H, W, values, g):
    """piecewise constant: a 3 x 4 grid of blocks with unequal, odd-placed borders, each block one of `values`"""
    ys = torch.tensor([0, (H + 2) // 3, (2 * H + 1) // 3 + (H > 4), H]).clamp(max=H)
    xs = torch.tensor([0, W // 4 + (W > 8), W // 2 + 3 * (W > 8), (3 * W) // 4 + (W > 8), W]).clamp(max=W)
    seg = torch.empty(H, W, dtype=torch.int64)
    pick = torch.randint(0, len(values), (12,), generator=g)
    for i in range(3):
        for j in range(4):
            seg[ys[i]:ys[i + 1], xs[j]:xs[j + 1]] = values[int(pick[i * 4 + j])]
    return seg


def _grads_ref(sums, pred):
    """d sums[:, k].sum() / d pred for k = 0, 1, 3 (sum t does not depend on pred: zeros) -> [4, *pred.shape]; the rows of `sums`
    depend on their own prediction row only, so this is every row's gradient of every sum."""
    out = torch.zeros(4, *pred.shape, dtype=sums.dtype)
    for k in (0, 1, 3):
        out[k], = torch.autograd.grad(sums[:, k].sum(), pred, retain_graph=True)
    return out


def _reference(fn, pred, confident):
    """fp64 sums and gradients; for the confident class also the error of ATen's fp32 CPU evaluation against them."""
    p64 = pred.double().requires_grad_(True)
    s64 = fn(p64, torch.float64)
    g64 = _grads_ref(s64, p64)
    aten = None
    if confident:
        p32 = pred.clone().requires_grad_(True)
        s32 = fn(p32, torch.float32)
        g32 = _grads_ref(s32, p32)
        aten = (s64.detach(), g64, s32.detach().double(), g32.double())
    return s64.detach(), g64, aten


def _row_max(x):
    return x.flatten(1).abs().max(1).values


WORST = {}


def _note(kernel, what, value):
    """largest figure seen per kernel and quantity, error / bound unless `what` says otherwise (printed: run with -s to collect)"""
    key = (kernel, what)
    if value > WORST.get(key, -1.0):
        WORST[key] = value
        print(f"[worst so far] {kernel} {what}: {value:.3g}")


def _check_sums(kernel, got, want, aten, pixels):
    """got [N, 4] from the kernel, want fp64.  1e-5 relative; confident class: max(1e-5, 4 x ATen fp32's own relative error), one
    figure per sum (the largest over the rows).  sum t exact.  A term below the smallest normal fp32 number (s = e^-120) cannot be
    held in fp32 at all: one FLT_MIN per pixel on top, 1e-34 on these maps."""
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all()
    assert torch.equal(got[:, 2], want[:, 2]), "sum t is an integer below 2^24: exact"
    tol = torch.full((4,), 1e-5, dtype=torch.float64)
    if aten is not None:
        s64, _, s32, _ = aten
        rel = ((s32 - s64).abs() / s64.abs().clamp(min=1e-300)).max(0).values
        _note(kernel, "ATen fp32's own relative error, sums", rel.max().item())
        tol = torch.maximum(tol, 4 * rel)
    err = (got - want).abs()
    bound = tol[None, :] * want.abs() + pixels * FLT_MIN * (want != 0)
    nz = bound > 0
    if nz.any():
        _note(kernel, "sums", (err[nz] / bound[nz]).max().item())
    assert (err <= bound).all(), (kernel, (err / bound.clamp(min=1e-300)).max(0).values.tolist(), tol.tolist())


def _check_grads(kernel, sums, pred, g64, aten):
    """Backward through the kernel once per output-weight row: the four one-hot rows (no term hides behind another) and a random one
    with a weight on sum t, which must have no effect.  Per prediction row: max |error| <= 1e-5 of the row's largest fp64 gradient
    (confident class: max(1e-5, 4 x ATen fp32's figure in the same metric)); 16 up-sampled pixels reach a logit, one FLT_MIN each
    for derivatives too small for fp32."""
    N = sums.shape[0]
    gen = torch.Generator().manual_seed(N)
    rand = torch.randn(N, 4, generator=gen, dtype=torch.float64)
    rand[:, 2] = 3.0 + rand[:, 2].abs()
    for name, w in [(f"e{k}", ONE_HOT[k].expand(N, 4)) for k in range(4)] + [("random", rand)]:
        got, = torch.autograd.grad(sums, pred, grad_outputs=w.float().to(sums.device), retain_graph=True)
        got = got.detach().double().cpu().reshape(N, -1)
        assert torch.isfinite(got).all()
        want = (w.T[:, :, None] * g64.reshape(4, N, -1)).sum(0)
        scale = _row_max(want)
        tol = 1e-5
        if aten is not None:
            a32 = (w.T[:, :, None] * aten[3].reshape(4, N, -1)).sum(0)
            nz = scale > 0
            if nz.any():
                tol = max(tol, 4 * (_row_max(a32 - want)[nz] / scale[nz]).max().item())
                _note(kernel, "ATen fp32's own error / row maximum, grad", tol / 4)
        err = _row_max(got - want)
        nz = scale > 0
        if nz.any():
            _note(kernel, "grad " + name, (err[nz] / (tol * scale[nz])).max().item())
        assert (err <= tol * scale + 16 * FLT_MIN * (scale > 0)).all(), (kernel, name, (err / scale.clamp(min=1e-300)).tolist(), tol)
        if name == "random":
            w0 = w.clone()
            w0[:, 2] = 0.0
            again, = torch.autograd.grad(sums, pred, grad_outputs=w0.float().to(sums.device), retain_graph=True)
            assert torch.equal(again.double().cpu().reshape(N, -1), got), "the weight of sum t reached the gradient"


# ------------------------------------------------------------------------------------------------ gathered kernel
@pytest.mark.parametrize("hyper", HYPER, ids=_ids)
@pytest.mark.parametrize("logits", LOGITS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_gathered_mask_loss_against_fp64(shape, logits, hyper):
    """ops.mask_loss_sums at P = 7 and P = 1, G = 3 targets reached through a non-identity gt_index with repeats.  Targets: per-pixel
    noise, regions and a constant one (all zero at alpha 0.25, all one at alpha 0.6); confident class: {ones, zeros, ones}.
    ATen fp32 on the confident inputs against fp64, measured on the CPU (the figure the bound of that class is 4 x of, one per
    case and quantity: the largest over the rows): focal sum 7e-5 .. 7e-4 relative at 8 x 64 and above, 2e-3 at 3 x 6, 6e-2 at
    1 x 2; gradients up to 7e-2 of a row's maximum (1 x 2).  On the other two classes, same inputs: sums 2.3e-7, gradients 1.2e-6
    (one-hot weights).
    On an MI355X the kernels' largest error / bound: sums 0.018, gradients 0.10 (focal, saturated) on the first two classes; 0.26 on
    the confident class (the kernels round s as ATen does, so their error there is ATen's: a quarter of the bound)."""
    from spike2former_amd import ops
    (h, w), (gamma, alpha) = shape, hyper
    g = _gen("gathered", shape, logits, hyper)
    H, W = 2 * h, 2 * w
    if logits == "confident":
        tgt = torch.stack([torch.ones(H, W), torch.zeros(H, W), torch.ones(H, W)]).to(torch.uint8)
    else:
        const = torch.zeros(H, W) if alpha == 0.25 else torch.ones(H, W)
        tgt = torch.stack([torch.randint(0, 2, (H, W), generator=g).float(), (_region_map(H, W, [0, 1, 0, 1, 1], g) == 1).float(),
                           const]).to(torch.uint8)
        tgt[:2, 0, 0] = 1                                                     # see _logits: an undecided pixel in every target
    gt_index = torch.tensor([2, 0, 1, 1, 2, 0, 2])
    sign = (tgt[gt_index].float().mean((1, 2)) * 2 - 1).view(-1, 1, 1)
    pred = _logits(logits, (7, h, w), g, sign, pin=True)

    def fn(p, dtype):
        return loss_ref.mask_sums(p, tgt, gt_index, alpha, gamma, dtype)
    want7, g7, aten7 = _reference(fn, pred, logits == "confident")
    for P in (7, 1):                                                          # a row's sums depend on that row alone
        want, g64, aten = want7[:P], g7[:, :P], None if aten7 is None else (aten7[0][:P], aten7[1][:, :P], aten7[2][:P], aten7[3][:, :P])
        dev = pred[:P].cuda().requires_grad_(True)
        sums = ops.mask_loss_sums(dev, tgt.cuda(), gt_index[:P].cuda(), alpha, gamma)
        _check_sums(f"mask_loss_sums[{logits}]", sums, want, aten, H * W)
        zero_target = (tgt[gt_index[:P]].flatten(1).sum(1) == 0)
        assert (sums.detach().cpu()[zero_target][:, [0, 2]] == 0).all(), "all-zero target: sum s t and sum t are exactly 0"
        _check_grads(f"mask_loss_sums[{logits}]", sums, dev, g64, aten)


# ------------------------------------------------------------------------------------------------ label-map kernel
def _label_maps(kind, H, W, K, g):
    """two different maps [2, H, W] with labels 0..K-1, ids >= K and 255, and the row classes [2, 5] to go with them"""
    values = list(range(K)) + [K, K + 1, 255]
    if kind == "constant":
        seg = torch.stack([torch.full((H, W), 2), torch.full((H, W), 4)])
        rc = torch.tensor([[2, -1, 4, 2, 0], [4, 2, -1, 255, 4]])            # the whole image; absent; unmatched
        return seg, rc
    if kind == "noise":
        seg = torch.tensor(values)[torch.randint(0, len(values), (2, H, W), generator=g)]
    else:
        seg = torch.stack([_region_map(H, W, values, g), _region_map(H, W, values[::-1], g)])
        seg[0, H // 2:H // 2 + 1, : (3 * W) // 4] = 255                       # a band of the ignored label
    seg[seg == 1] = 3                                                         # class 1 is absent from both images
    seg[1][seg[1] == 0] = 2                                                   # class 0 from the second only
    rc = torch.tensor([[0, -1, 1, 3, K], [2, 0, 255, -1, 3]])                 # (1, 1) = class 0: absent from ITS image only
    for b, corner_classes in enumerate(([0, 3, K], [2, 255, 3])):             # see _logits: an undecided pixel in every target
        seg[b, 0, 0], seg[b, 0, -1], seg[b, -1, 0] = corner_classes
    return seg, rc


@pytest.mark.parametrize("hyper", HYPER, ids=_ids)
@pytest.mark.parametrize("logits,maps", [("regular", "regions"), ("regular", "noise"), ("regular", "constant"), ("saturated", "regions"),
                                         ("saturated", "noise"), ("saturated", "constant"), ("confident", "constant")])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_label_map_mask_loss_against_fp64(shape, logits, maps, hyper):
    """ops.mask_loss_seg directly against loss_ref.seg_sums (not through the gathered kernel): B = 2 images with different maps,
    R = 5 rows each -- unmatched (-1), a class absent from its image (present in the other), ordinary classes, an id >= K, the
    ignored label as a class, and (constant maps) a class that covers the whole image.
    ATen fp32 on the confident inputs against fp64, measured on the CPU: focal sum 7e-5 .. 7e-4 relative at 8 x 64 and above,
    2e-3 at 3 x 6; at 1 x 2 with gamma >= 2 ATen's binary_cross_entropy_with_logits rounds to 0 on a row of logits near -15
    (relative error 1, gradients 0.75 of the row maximum), so the bound of that class says nothing about the focal sum of those two
    cases -- the larger maps carry it.  On an MI355X the kernels' largest error / bound: sums 0.025, gradients 0.12 (saturated) on
    the first two classes; confident: sums 0.11 (1 - s comes without cancellation forward), gradients 0.25."""
    from spike2former_amd import ops
    (h, w), (gamma, alpha) = shape, hyper
    B, R, K = 2, 5, 5
    g = _gen("seg", shape, logits, maps, hyper)
    seg, rc = _label_maps(maps, 2 * h, 2 * w, K, g)
    seg_u8 = seg.to(torch.uint8)
    hit = (seg[:, None] == rc[:, :, None, None]).float().mean((2, 3))          # 0 or 1 on constant maps
    pred = _logits(logits, (B, R, h, w), g, (hit * 2 - 1).view(B, R, 1, 1), pin=True)

    def fn(p, dtype):
        return loss_ref.seg_sums(p, seg_u8, rc, alpha, gamma, dtype)
    want, g64, aten = _reference(fn, pred, logits == "confident")
    dev = pred.cuda().requires_grad_(True)
    sums = ops.mask_loss_seg(dev, seg_u8.cuda(), rc.to(torch.int32).reshape(-1).cuda(), alpha, gamma)
    _check_sums(f"mask_loss_seg[{logits}]", sums, want, aten, 4 * h * w)
    got = sums.detach().cpu()
    unmatched = rc.reshape(-1) < 0
    absent = ((seg[:, None] == rc[:, :, None, None]).flatten(2).sum(2) == 0).reshape(-1) & ~unmatched
    assert unmatched.any() and absent.any()
    assert (got[unmatched] == 0).all() and (got[absent][:, [0, 2]] == 0).all()
    _check_grads(f"mask_loss_seg[{logits}]", sums, dev, g64.reshape(4, B * R, h, w), None if aten is None else
                 (aten[0], aten[1], aten[2], aten[3].reshape(4, B * R, h, w)))
    e, = torch.autograd.grad(sums, dev, grad_outputs=torch.ones_like(sums))
    assert (e.reshape(B * R, -1)[unmatched.cuda()] == 0).all(), "rows without a match: gradient exactly 0"


# ------------------------------------------------------------------------------------------------ cost bins
def _cost_labels(B, hw, K, g):
    """labels 0 .. min(K + 2, 255) - 1 and 255: per-pixel noise in the first half, runs of 5 (which straddle the 4-pixel quads a
    thread walks) in the second; class K - 1 is absent from the second image (relabelled K, an id past the classes)"""
    values = torch.tensor(list(range(min(K + 2, 255))) + [255])
    lab = values[torch.randint(0, len(values), (B, hw), generator=g)]
    runs = values[torch.randint(0, len(values), (B, hw // 5 + 1), generator=g)].repeat_interleave(5, 1)[:, :hw]
    lab[:, hw // 2:] = runs[:, hw // 2:]
    lab[1][lab[1] == K - 1] = K
    lab[0, 0], lab[0, hw - 1] = K, 255                                        # both kinds of label outside the classes exist
    return lab.to(torch.uint8)


@pytest.mark.parametrize("logits", ["regular", "saturated"])
@pytest.mark.parametrize("K", [1, 7, 150, 254])
@pytest.mark.parametrize("hw", [4, 12, 1028, 4096])
def test_cost_bins_against_fp64(hw, K, logits):
    """ops.mask_cost_bins before any normalisation: every bin against fp64 within 2e-5 of the bin's absolute-term sum (sum |pos| +
    sum |neg| of its pixels; the s bins: sum s) + hw 2^-32 for the fixed-point rounding; bins of absent classes exactly 0; labels
    >= K and 255 in no class bin (the reference leaves them out) but in the two totals.  hw = 1028: 257 quads, one thread takes
    two.  The kernel evaluates exp, log and 1/x with the native instructions: the largest error / bound seen on an MI355X is 0.12
    (an fp32 restatement of its arithmetic with ATen's functions, on the CPU: 0.013); printed with -s."""
    from spike2former_amd import ops
    B, R = 2, 3
    alpha, gamma, eps = 0.25, 2.0, 1e-12                                      # MaskFormerLoss.cost_focal_cfg
    g = _gen("bins", hw, K, logits)
    lab = _cost_labels(B, hw, K, g)
    pred = _logits(logits, (B, R, hw), g)
    want, absum = loss_ref.cost_bins(pred, lab, K, alpha, gamma, eps)
    got = ops.mask_cost_bins(pred.cuda(), lab.cuda(), K, alpha, gamma, eps).double().cpu()
    assert got.shape == (B, R, 2 * K + 2) and torch.isfinite(got).all()
    bound = 2e-5 * absum + hw * 2.0 ** -32
    err = (got - want).abs()
    _note(f"mask_cost_bins[{logits}]", "bins", (err / bound).max().item())
    assert (err <= bound).all(), (err / bound).max().item()
    count = torch.stack([(lab == c).sum(1) for c in range(K)], 1)              # [B, K]
    absent = (count == 0)[:, None, :].expand(B, R, K)
    assert absent[1, :, K - 1].all()
    assert (got[..., :K][absent] == 0).all() and (got[..., K:2 * K][absent] == 0).all(), "absent class: both bins exactly 0"
    outside = (lab.long() >= K).double()                                      # pixels in no class bin: still in the totals
    s = pred.double().sigmoid()
    in_bins = got[..., K:2 * K].sum(-1)
    assert outside.sum() > 0
    assert ((got[..., 2 * K + 1] - in_bins - (s * outside[:, None]).sum(-1)).abs() <= 2e-5 * absum[..., 2 * K + 1] + 2 * hw * 2.0 ** -32).all()


# ------------------------------------------------------------------------------------------------ refused shapes
def test_wrappers_refuse_odd_widths_and_ragged_rows():
    """odd w (the kernels read float2 / write uchar4 quads) and hw % 4 != 0 are refused by the entry points before any launch"""
    from spike2former_amd import ops
    from spike2former_amd._lib import S2FError
    pred = torch.zeros(1, 2, 3, device="cuda")
    with pytest.raises(S2FError, match="even w"):
        ops.mask_loss_sums(pred, torch.zeros(1, 4, 6, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"),
                           0.25, 2.0)
    with pytest.raises(S2FError, match="even width"):
        ops.mask_loss_seg(pred[None], torch.zeros(1, 4, 6, dtype=torch.uint8, device="cuda"),
                          torch.zeros(1, dtype=torch.int32, device="cuda"), 0.25, 2.0)
    with pytest.raises(S2FError, match="hw %"):
        ops.mask_cost_bins(torch.zeros(1, 1, 6, device="cuda"), torch.zeros(1, 6, dtype=torch.uint8, device="cuda"), 3, 0.25, 2.0, 1e-12)
    torch.cuda.synchronize()
