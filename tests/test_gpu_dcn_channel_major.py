"""The DCNv3 sampling core on channel-major maps (s2f_dcnv3_fwd_cm / s2f_dcnv3_bwd_cm, ops.dcnv3_core_cm, ops.cfg.DCN_CHANNEL_MAJOR):
one workgroup per (image, group) slice, the slice's planes staged in LDS, every plane stored with the lanes along the pixels.  The
arithmetic of a (pixel, group) is the NHWC kernels', so everything here is compared with torch.equal against the route it replaces:
transposition -> [N, H, W, C] entry point -> transposition."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EINVAL = -1          # include/s2f.h


@pytest.fixture(scope="module")
def ops():
    from spike2former_amd import ops
    return ops


def _inputs(N, H, W, G, Cg, K, seed):
    """x channel-major [N, C, H, W]; offsets of a few pixels with every fifth pair reaching far outside the map; a spike-like mask;
    ONE set of output gradients whose magnitudes span 2^-20 .. 2^20 (the accumulator-range defect of the fixed-point backward on
    small maps lived where one contribution is far above the others of its slice)."""
    g = torch.Generator().manual_seed(seed)
    C, P = G * Cg, K * K
    x = torch.randn(N, C, H, W, generator=g)
    off = torch.randn(N, H, W, G * P * 2, generator=g) * 2
    far = torch.rand(N, H, W, G * P * 2, generator=g) < 0.2
    off = torch.where(far, off * (H + W), off)
    m = torch.clamp(torch.round(torch.randn(N, H, W, G * P, generator=g) + 1), 0, 8) / 8
    e = torch.randint(-20, 21, (N, C, H, W), generator=g).float()
    gy = torch.randn(N, C, H, W, generator=g) * torch.exp2(e)
    return [t.cuda() for t in (x, off, m, gy)]


def _geo(N, H, W, G, Cg, K):
    return (N, H, W, G, Cg, K, K, 1, 1, K // 2, K // 2, 1, 1)


def _nhwc(ops, t):
    """[N, C, H, W] -> [N, H, W, C] with the transposition kernel the module's transposing route uses"""
    N, C, H, W = t.shape
    return ops.transpose_last2(t.reshape(N, C, H * W)).view(N, H, W, C)


def _nchw(ops, t):
    N, H, W, C = t.shape
    return ops.transpose_last2(t.reshape(N, H * W, C)).view(N, C, H, W)


# the issue's three geometries (Cg = 8, K = 3: the unrolled kernels; 32 x 32 x 32 groups x 8 images is the C2 launch, 256 workgroups
# of 1 024 pixels), then a Cg = 4 and a Cg = 3 map (the generic loops; NHWC side: the 16-byte and the scalar kernel) and a
# 40 x 40 map, whose 1 600 pixels take two rounds of the forward's 1 024-pixel staging chunk and seven of the backward's 256-pixel
# one, and a Cg = 16 map, whose backward chunks are too large for the register-prefetched form
SHAPES = [(2, 8, 8, 4, 8, 3), (1, 12, 20, 2, 8, 3), (8, 32, 32, 32, 8, 3), (1, 5, 7, 2, 4, 3), (2, 6, 5, 3, 3, 3),
          (1, 40, 40, 2, 4, 3), (1, 8, 9, 2, 16, 3)]


@pytest.mark.parametrize("N,H,W,G,Cg,K", SHAPES)
def test_channel_major_entry_points_equal_the_transposing_route(ops, N, H, W, G, Cg, K):
    from spike2former_amd._lib import lib
    x, off, m, gy = _inputs(N, H, W, G, Cg, K, seed=11 + H)
    geo = _geo(N, H, W, G, Cg, K)
    assert lib.s2f_dcnv3_cm_ok(N, H, W, G, Cg, K, K, 1, 1, K // 2, K // 2, 1, 1) == 1

    # the route it replaces: transposition, NHWC entry points, transposition
    xt, gyt = _nhwc(ops, x).contiguous(), _nhwc(ops, gy).contiguous()
    yt = torch.empty_like(xt)
    assert lib.s2f_dcnv3_fwd(xt.data_ptr(), off.data_ptr(), m.data_ptr(), yt.data_ptr(), *geo, 1.0, None) == 0
    gxt, goff_t, gm_t = torch.empty_like(xt), torch.empty_like(off), torch.empty_like(m)
    assert lib.s2f_dcnv3_bwd(xt.data_ptr(), off.data_ptr(), m.data_ptr(), gyt.data_ptr(), gxt.data_ptr(), goff_t.data_ptr(),
                             gm_t.data_ptr(), *geo, 1.0, None) == 0
    want_y, want_gx = _nchw(ops, yt), _nchw(ops, gxt)

    y = torch.full_like(x, float("nan"))
    assert lib.s2f_dcnv3_fwd_cm(x.data_ptr(), off.data_ptr(), m.data_ptr(), y.data_ptr(), *geo, 1.0, None) == 0
    gx, goff, gm = torch.full_like(x, float("nan")), torch.full_like(off, float("nan")), torch.full_like(m, float("nan"))
    assert lib.s2f_dcnv3_bwd_cm(x.data_ptr(), off.data_ptr(), m.data_ptr(), gy.data_ptr(), gx.data_ptr(), goff.data_ptr(),
                                gm.data_ptr(), *geo, 1.0, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, want_y), "output"
    assert torch.equal(gx, want_gx), "grad_input"
    assert torch.equal(goff, goff_t), "grad_offset"
    assert torch.equal(gm, gm_t), "grad_mask"
    assert y.abs().max().item() > 0 and gx.abs().max().item() > 0 and bool((y == 0).any())          # inside and outside taps both occur

    # the autograd wrapper is the same two calls
    xa, oa, ma = (t.clone().requires_grad_(True) for t in (x, off, m))
    ya = ops.dcnv3_core_cm(xa, oa, ma, K, K, 1, 1, K // 2, K // 2, 1, 1, G, Cg, 1.0)
    ya.backward(gy)
    assert torch.equal(ya.detach(), y) and torch.equal(xa.grad, gx) and torch.equal(oa.grad, goff) and torch.equal(ma.grad, gm)


def test_a_slice_that_does_not_fit_one_workgroup_is_refused_before_any_launch(ops):
    """64 x 32 (the C3 map, whose NHWC backward runs in bands): S2F_EINVAL from both entry points, the outputs untouched"""
    from spike2former_amd._lib import lib, S2FError
    N, H, W, G, Cg, K = 1, 64, 32, 2, 8, 3
    x, off, m, gy = _inputs(N, H, W, G, Cg, K, seed=3)
    geo = _geo(N, H, W, G, Cg, K)
    assert lib.s2f_dcnv3_cm_ok(N, H, W, G, Cg, K, K, 1, 1, 1, 1, 1, 1) == 0
    assert not ops.dcnv3_cm_ok(N, H, W, K, K, 1, 1, 1, 1, 1, 1, G, Cg)
    y = torch.full_like(x, 7.0)
    gx, goff, gm = torch.full_like(x, 7.0), torch.full_like(off, 7.0), torch.full_like(m, 7.0)
    assert lib.s2f_dcnv3_fwd_cm(x.data_ptr(), off.data_ptr(), m.data_ptr(), y.data_ptr(), *geo, 1.0, None) == EINVAL
    assert b"does not fit" in lib.s2f_last_error()
    assert lib.s2f_dcnv3_bwd_cm(x.data_ptr(), off.data_ptr(), m.data_ptr(), gy.data_ptr(), gx.data_ptr(), goff.data_ptr(),
                                gm.data_ptr(), *geo, 1.0, None) == EINVAL
    torch.cuda.synchronize()
    for t in (y, gx, goff, gm):
        assert bool((t == 7.0).all())
    with pytest.raises(S2FError):
        ops.dcnv3_core_cm(x, off, m, K, K, 1, 1, 1, 1, 1, 1, G, Cg, 1.0)


@pytest.mark.parametrize("H,W", [(8, 8), (32, 32), (64, 32)])
def test_module_is_bit_identical_with_the_switch_on_and_off(ops, H, W):
    """DCNv3_pytorch.forward_nchw in train mode: the switch only moves the transpositions out, so the output, the input gradient and
    the BatchNorm / bias gradients are the same bits, and the convolution weights' atomically summed gradients agree to the few ulp
    by which one route differs from itself (64 x 32: the map keeps the transposing route either way)."""
    import spike2former_amd as s2f
    from spike2former_amd.head_layers import DCNv3_pytorch
    torch.manual_seed(5)
    mod = DCNv3_pytorch(channels=64, kernel_size=3, group=8, dw_kernel_size=5, expension_ratio=2, norm_layer="BN")
    for conv in (mod.offset[0], mod.mask[0]):          # (the reference zero-initialises these: every tap would sit on the grid)
        torch.nn.init.normal_(conv.weight, std=0.2)
        torch.nn.init.normal_(conv.bias, std=0.5)
    mod = mod.cuda().train()
    state = {k: v.clone() for k, v in mod.state_dict().items()}
    T, N = 2, 2
    inp = torch.randn(T, N, 64, H, W, device="cuda")
    gy = torch.randn(T, N, 64, H, W, device="cuda")

    def run(flag):
        was = ops.cfg.DCN_CHANNEL_MAJOR
        ops.cfg.DCN_CHANNEL_MAJOR = flag
        try:
            mod.load_state_dict(state)
            mod.zero_grad(set_to_none=True)
            s2f.reset_net(mod)
            a = inp.clone().requires_grad_(True)
            y = mod.forward_nchw(a)
            y.backward(gy)
            ops.wgrad_join()
            torch.cuda.synchronize()
            return [y.detach().clone(), a.grad.clone()] + [torch.zeros(()) if p.grad is None else p.grad.clone()
                                                           for p in mod.parameters()]
        finally:
            ops.cfg.DCN_CHANNEL_MAJOR = was

    on, offs = run(True), [run(False) for _ in range(2)]
    assert on[0].abs().max().item() > 0 and on[1].abs().max().item() > 0
    names = ["output", "input gradient"] + [n for n, _ in mod.named_parameters()]
    for i, name in enumerate(names):
        spread = (offs[0][i] - offs[1][i]).abs().max().item()
        diff = (on[i] - offs[0][i]).abs().max().item()
        print(f"{H}x{W} {name}: switch-off against itself {spread:.3e}, switch on against off {diff:.3e}")
        if name.endswith(".0.weight"):
            # Convolution weights: their gradient kernels add split-contraction partials with fp32 atomics in arrival order, so ONE
            # route differs from itself from run to run by the rounding of those few partial sums (measured: 0 .. 2 ulp of the
            # largest element, the line above).  Both routes hand these kernels the same bits (the output and the input gradient
            # are compared exactly here), so they may differ by that much and no more: 64 ulp of the largest element, whatever
            # the two switch-off runs happened to show.
            assert diff <= 64 * 2.0 ** -24 * offs[0][i].abs().max().item(), name
        else:
            assert torch.equal(on[i], offs[0][i]), name
