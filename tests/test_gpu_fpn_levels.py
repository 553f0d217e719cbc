"""The pixel decoder's top-down level maps without their spare passes: the up-sampled residual formed inside the BatchNorm apply
kernel (s2f_bn_act_up_fwd) against the two launches, bit for bit; the finest level's neuron without its fp32 pre-activation; the
depthwise stencil's BatchNorm partials (s2f_dwconv_fwd_stats) against fp64 tile sums and against the statistics pass.  Every test
runs under the conftest's STRICT census."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from spike2former_amd import ops
    return ops


def _calls(monkeypatch, name):
    """count the calls of one C entry point (the ctypes function stays the callee)"""
    from spike2former_amd._lib import lib
    real, log = getattr(lib, name), []

    def spy(*a):
        log.append(a)
        return real(*a)
    monkeypatch.setattr(lib, name, spy)
    return log


# ------------------------------------------------------------------------------------------------ A: up-sampling in the residual read
# (2,3,16,16): L = 256, a tile is a whole plane and the channel changes every tile; (2,3,8,64): a tile is four image rows;
# (1,2,2,256): the source has one row, both vertical edges clamped; (1,2,2,512): W > 256, a row spans two tiles (lanes 0 / 63 load
# their outer taps); (1,2,6,40): L = 240 is no whole tile -- the two launches, still equal
_UP_SHAPES = [(2, 3, 16, 16), (2, 3, 8, 64), (1, 2, 4, 128), (1, 2, 2, 256), (1, 2, 2, 512), (1, 2, 6, 40)]


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("N,C,H,W", _UP_SHAPES)
def test_upsampled_residual_inside_bn_is_the_two_launches(ops, spike_mode, monkeypatch, N, C, H, W, bf16):
    """ops.bn_act(residual_lo=lo) == ops.bn_act(residual=ops.upsample_bilinear(lo)) in train mode with a neuron, torch.equal on
    everything the pair produces: u, spikes, mask words, running statistics, firing counters; gz, dgamma, dbeta and the gradient
    of the low-resolution map after a backward with a seeded g_y, without and with a gradient on the pass-through port."""
    spike_mode(bf16)
    fused_calls = _calls(monkeypatch, "s2f_bn_act_up_fwd")
    g = torch.Generator().manual_seed(N * 1000 + C * 100 + H + W)
    z0 = (torch.randn(N, C, H, W, generator=g) * 1.5 + 0.4).cuda()
    lo0 = torch.randn(N, C, H // 2, W // 2, generator=g).cuda()
    bias = torch.randn(C, generator=g).cuda()
    gamma0, beta0 = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.3 + 0.5).cuda()
    gy = torch.randn(N, C, H, W, generator=g).cuda()
    gt = torch.randn(N, C, H // 2, W // 2, generator=g).cuda()
    want_fused = (H * W) % 256 == 0
    assert ops.bn_up_ok(z0, lo0, True, 8) == want_fused

    def run(fused, port):
        z, lo = z0.clone().requires_grad_(True), lo0.clone().requires_grad_(True)
        gamma, beta = gamma0.clone().requires_grad_(True), beta0.clone().requires_grad_(True)
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        nbt = torch.zeros((), dtype=torch.int64, device="cuda")
        st = ops.new_stats(z.device)
        if fused:
            u, y, _, through = ops.bn_act(z, bias, gamma, beta, rm, rv, nbt, True, 0.1, 1e-5, lif=True, want_pre=True, stats=st,
                                          residual_lo=lo, lo_skip=True)
        else:
            up, through = ops.upsample_bilinear(lo, (H, W), skip=True)
            u, y, _ = ops.bn_act(z, bias, gamma, beta, rm, rv, nbt, True, 0.1, 1e-5, residual=up, lif=True, want_pre=True, stats=st)
        mask = u.grad_fn.saved_tensors[4]
        loss = (y.float() * gy).sum()
        if port:
            loss = loss + (through * gt).sum()
        loss.backward()
        return dict(u=u.detach(), y=y.data.detach(), mask=mask, rm=rm, rv=rv, nbt=nbt, stats=ops.read_stats(st), gz=z.grad,
                    dgamma=gamma.grad, dbeta=beta.grad, glo=lo.grad)

    for port in (False, True):
        before = len(fused_calls)
        a, b = run(False, port), run(True, port)
        assert len(fused_calls) - before == int(want_fused)          # the fused form ran exactly where it is claimed to
        assert a["y"].dtype == (torch.bfloat16 if bf16 else torch.float32)
        for k in a:
            assert torch.equal(a[k], b[k]), (k, port)
        assert a["glo"].abs().max().item() > 0 and int(a["stats"][0]) > 0 and int(a["nbt"]) == 1


def test_up_entry_point_refuses_what_the_predicate_refuses():
    """s2f_bn_up_ok is the gate of s2f_bn_act_up_fwd: eval mode, a plane that is no whole tile, a width that neither divides nor is a
    multiple of 256, an odd height and a single-pass shape are refused before any launch."""
    from spike2former_amd._lib import lib
    assert lib.s2f_bn_up_ok(2, 3, 16, 16, 1, 8) == 1 and lib.s2f_bn_up_ok(8, 256, 256, 256, 1, 8) == 1
    assert lib.s2f_bn_up_ok(1, 2, 2, 512, 1, 8) == 1 and lib.s2f_bn_up_ok(1, 2, 2, 768, 1, 8) == 1
    assert lib.s2f_bn_up_ok(2, 3, 16, 16, 0, 8) == 0          # eval mode
    assert lib.s2f_bn_up_ok(1, 2, 6, 40, 1, 8) == 0           # L = 240
    assert lib.s2f_bn_up_ok(1, 2, 8, 96, 1, 8) == 0           # L = 768 is whole tiles, W = 96 is no divisor of 256
    assert lib.s2f_bn_up_ok(1, 2, 3, 256, 1, 8) == 0          # odd H
    assert lib.s2f_bn_up_ok(2, 3, 16, 16, 1, 6) == 0          # D not a power of two
    assert lib.s2f_bn_up_ok(4, 64, 32, 32, 1, 8) == 0         # a single-pass shape keeps its own kernel
    P = 1 << 20
    assert lib.s2f_bn_act_up_fwd(P, None, P, P, None, None, None, P, P, P, None, None, P, None, None, None, 1, 2, 6, 40, 0.1, 1e-5, 1,
                                 1.0, 8, 1, None) == -1


# ------------------------------------------------------------------------------------------------ B: the finest level without u
def test_finest_level_hands_out_spikes_without_a_preactivation(ops, monkeypatch):
    """The pixel decoder's finest level asks the BatchNorm kernel for mask_feature_spike's spikes directly.  Against the same module
    with a forward hook on that neuron -- the route that stores the fp32 pre-activation u, as every step did before: the hook sees
    (u, fp32 spikes) with the spikes the head is handed; mask features, memory, the gradients of the input features and every
    parameter gradient a kernel forms in a fixed order (BatchNorm affine pairs, biases, scales) are torch.equal; and without the hook
    no launch on the finest map writes a pre-activation.  The convolutions' weight gradients are summed across workgroups with fp32
    atomics, whose order changes from run to run of the SAME route (measured on this module: 35 of 116 parameters, all of them
    convolution weights, differ between two identical runs by up to 3.6e-7 of max|g| = 3 ulp): they are held to 64 * 2^-24 of max|g|
    -- at most 64 workgroup partials per element on these maps, half an ulp of the running sum per reordered addition."""
    import spike2former_amd as s2f
    from spike2former_amd.init_utils import seeded_init
    w = s2f.WORKLOADS["C1_64"]
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C1_64"))).cuda().train()
    s2f.set_keep_membrane(model, False)
    pd = model.decode_head.pixel_decoder
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    img = torch.randn(w["B"], 3, w["H"], w["W"], generator=torch.Generator().manual_seed(5)).cuda()
    s2f.reset_net(model)
    with torch.no_grad():
        feats0 = [f.float().detach().clone() for f in model.extract_feat(img)]
    finest = feats0[0].shape[-2] * feats0[0].shape[-1]
    gen = torch.Generator().manual_seed(9)
    weights = {}

    def run(fold=False):
        model.load_state_dict(sd)
        s2f.reset_net(model)
        model.zero_grad(set_to_none=True)
        feats = [f.clone().requires_grad_(True) for f in feats0]
        mf, memory, out = pd(feats, None, fold_mask_feature=fold)
        if fold:
            return mf
        loss = 0
        for i, t in enumerate([mf, memory] + list(out)):
            if i not in weights:
                weights[i] = torch.randn(t.shape, generator=gen).cuda()
            loss = loss + (t * weights[i]).sum()
        loss.backward()
        return (mf.detach(), memory.detach(), {n: p.grad.clone() for n, p in pd.named_parameters() if p.grad is not None},
                [f.grad.clone() for f in feats])

    seen = []
    hook = pd.mask_feature_spike.register_forward_hook(lambda m, i, o: seen.append((i[0].detach().clone(), o.detach().clone())))
    mf0, mem0, gp0, gf0 = run()
    hook.remove()
    assert len(seen) == 1 and seen[0][0].dtype == torch.float32 and seen[0][0].shape == seen[0][1].shape
    fwd, up = _calls(monkeypatch, "s2f_bn_act_fwd"), _calls(monkeypatch, "s2f_bn_act_up_fwd")
    mf1, mem1, gp1, gf1 = run()
    on_finest = [a for a in fwd if a[16] * a[17] * a[18] == seen[0][0].numel() and a[18] == finest] + \
                [a for a in up if a[18] * a[19] == finest]
    assert len(on_finest) == 2                                            # the lateral BatchNorm and the output convolution's
    assert all(not a[10] for a in on_finest)                              # u_out == NULL: no fp32 pre-activation of the finest map
    assert all(a[12] for a in on_finest)                                  # both hand out spikes
    assert torch.equal(mf0, mf1) and torch.equal(mem0, mem1)
    assert set(gp0) == set(gp1) and len(gp0) > 100
    atomic = {n for n, p in pd.named_parameters() if p.dim() > 1}          # (convolution weights: atomically accumulated)
    assert len(set(gp0) - atomic) >= 70
    for n in gp0:
        if n in atomic:
            assert (gp0[n] - gp1[n]).abs().max().item() <= 64 * 2.0 ** -24 * gp0[n].abs().max().item(), n
        else:
            assert torch.equal(gp0[n], gp1[n]), n
    assert all(torch.equal(a, b) for a, b in zip(gf0, gf1)) and all(a.abs().max().item() > 0 for a in gf0)
    s0 = run(fold=True)                                                   # what the head's folded mask contraction is handed
    assert isinstance(s0, ops.Spikes)
    assert torch.equal(s0.float().detach().reshape(seen[0][1].shape), seen[0][1])


# ------------------------------------------------------------------------------------------------ C: depthwise partials
# (2,3,32,128): one row of 64 x 32 tiles; (1,2,64,192); (2,3,64,64): the 32 x 32-tile form; (1,2,40,72): partial tiles
_DW_SHAPES = [(2, 3, 32, 128), (1, 2, 64, 192), (2, 3, 64, 64), (1, 2, 40, 72)]


def _dw_tile_sums(y, th, tw):
    """fp64 (sum, sum of squares) per (channel, (n, tile)) of [N, C, H, W] cut into th x tw tiles (row-major), zero-padded"""
    N, C, H, W = y.shape
    ny, nx = -(-H // th), -(-W // tw)
    yp = torch.zeros(N, C, ny * th, nx * tw, dtype=torch.float64, device=y.device)
    yp[:, :, :H, :W] = y.double()
    t = yp.view(N, C, ny, th, nx, tw).permute(1, 0, 2, 4, 3, 5).reshape(C, N * ny * nx, th * tw)
    return torch.stack([t.sum(-1), (t * t).sum(-1)], -1)


@pytest.mark.parametrize("x_bf16", [True, False])
@pytest.mark.parametrize("N,C,H,W", _DW_SHAPES)
def test_dwconv_stats_partials_are_the_tile_sums(N, C, H, W, x_bf16):
    """s2f_dwconv_fwd_stats stores the y of s2f_dwconv_fwd bit for bit, and partials[c, (n, tile)] are the sum / sum of squares of
    the outputs that workgroup stored: fp32 sums of <= 2048 values against fp64, 1e-5 of the tile's sum of |.| (the bound of
    test_conv3x3_epilogue_partials_are_the_tile_sums); partial tiles count stored outputs only."""
    from spike2former_amd._lib import check, lib
    g = torch.Generator().manual_seed(N + C + H + W)
    w = (torch.randn(C, 3, 3, generator=g) / 3).cuda()
    if x_bf16:
        x = (torch.randint(0, 9, (N, C, H, W), generator=g).float() / 8).to(torch.bfloat16).cuda()
    else:
        x = torch.randn(N, C, H, W, generator=g).cuda()
    st = torch.cuda.current_stream().cuda_stream
    wide = W % 4 == 0 and W >= 128 and H >= 32
    th, tw = (32, 64) if wide else (32, 32)
    P = lib.s2f_dwconv_stats_slots(N, H, W)
    assert P == N * (-(-H // th)) * (-(-W // tw))
    y0 = torch.empty(N, C, H, W, device="cuda")
    check(lib.s2f_dwconv_fwd(x.data_ptr(), w.data_ptr(), None, y0.data_ptr(), N, C, H, W, 3, 1, int(x_bf16), st), "plain")
    y1 = torch.full((N, C, H, W), float("nan"), device="cuda")
    part = torch.full((C, P, 2), float("nan"), device="cuda")
    check(lib.s2f_dwconv_fwd_stats(x.data_ptr(), w.data_ptr(), y1.data_ptr(), part.data_ptr(), P, N, C, H, W, int(x_bf16), st), "stats")
    assert torch.equal(y0, y1)
    ref, scale = _dw_tile_sums(y1, th, tw), _dw_tile_sums(y1.abs(), th, tw)
    err = (part.double() - ref).abs()
    print("max partial error / bound:", (err / (1e-5 * scale + 1e-30)).max().item())
    assert (err <= 1e-5 * scale + 1e-30).all()
    assert lib.s2f_dwconv_fwd_stats(x.data_ptr(), w.data_ptr(), y1.data_ptr(), part.data_ptr(), P + 1, N, C, H, W, int(x_bf16), st) == -1


@pytest.mark.parametrize("N,C,H,W", _DW_SHAPES)
def test_bn_from_dwconv_partials_is_bn_from_the_statistics_pass(ops, spike_mode, N, C, H, W):
    """Depthwise stencil -> train-mode BatchNorm -> neuron with the statistics from the stencil's partials against the statistics
    pass (ops.BN_PARTIALS off), within the bounds of test_bn_from_partials_is_bn_from_the_statistics_pass: pre-activation 1e-5,
    running variance 1e-5, spikes differing by one level in <= 1e-4 of the elements.  (The statistics agree to fp32 round-off, 1e-7
    relative: a spike flips only where 8 u lies within ~1e-6 of a rounding boundary -- of randn-based data, whose density per unit of
    8 u is below 0.4 / sigma, a share of the order of 1e-6.)  y itself is the same tensor either way, and so are the gradients' routes."""
    spike_mode(True)
    g = torch.Generator().manual_seed(N * 7 + C + H + W)
    x = ops.Spikes((torch.randint(0, 9, (N, C, H, W), generator=g).float() / 8).to(torch.bfloat16).cuda(), None)
    w = (torch.randn(C, 1, 3, 3, generator=g) / 3 + 0.1).cuda()
    gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.3 + 0.5).cuda()
    outs = []
    was = ops.BN_PARTIALS
    try:
        for on in (False, True):
            ops.BN_PARTIALS = on
            rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
            nbt = torch.zeros((), dtype=torch.int64, device="cuda")
            before = list(ops.BN_PARTIALS_USED)
            z = ops.dwconv(x, w, 1, stats=True)
            assert (ops.stats_of(z) is not None) == on
            u, y, _ = ops.bn_act(z, None, gamma, beta, rm, rv, nbt, True, 0.1, 1e-5, lif=True, want_pre=True)
            used = [a - c for a, c in zip(ops.BN_PARTIALS_USED, before)]
            assert used == ([1, 0] if on else [0, 1])
            outs.append((z, u, y.float(), rm, rv))
    finally:
        ops.BN_PARTIALS = was
    (z0, u0, y0, rm0, rv0), (z1, u1, y1, rm1, rv1) = outs
    close = lambda a, c, tol: (a - c).abs().max().item() <= tol * max(c.abs().max().item(), 1e-6)
    assert torch.equal(z0, z1)
    d = (y1 - y0) * 8
    print("u", ((u1 - u0).abs().max() / u0.abs().max()).item(), "rv", ((rv1 - rv0).abs().max() / rv0.abs().max()).item(),
          "flipped share", (d != 0).float().mean().item())
    assert close(u1, u0, 1e-5) and close(rm1, rm0, 1e-6) and close(rv1, rv0, 1e-5)
    assert d.abs().max().item() <= 1 and (d != 0).float().mean().item() <= 1e-4
