"""The q, k, v projection chains of the decoder's self-attention as sibling launches (ops.cfg.DECODER_SIBLINGS): one grouped launch per
stage -- s2f_pgemm_nn_bf16_grouped, s2f_bn_act_fwd_grouped / _bwd_grouped, s2f_pgemm_dx_f32_grouped -- on a group-outermost buffer
[G][B][C][L].  The grouped kernels are the single kernels' bodies behind a pointer offset, so every check here is EQUALITY with the
single calls, bit for bit:

  (a) the grouped spike GEMM against G calls of s2f_pgemm_nn_bf16, on every tile of the register-staged form (cfg 6, 7, 8; one and
      two K steps per barrier), ragged M / N / K, two groups reading one map; argument errors before any launch;
  (b) the grouped BatchNorm (+ neuron) forward and backward against G calls of s2f_bn_act_fwd / s2f_bn_act_bwd;
  (c) the grouped input gradient in the group-outermost layout against G calls of s2f_pgemm_dx_f32;
  (d) one DetrTransformerDecoderLayer.forward_stream with the switch on and off, eager and as a captured graph.

Spike operands are draws on the spike grid k / 8, k = 0 .. 8, as in tests/attn_ref.py; everything else is randn."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

EINVAL, EALIGN = -1, -2          # include/s2f.h


@pytest.fixture(scope="module")
def ops():
    from spike2former_amd import ops
    return ops


def spikes(shape, g):
    return (torch.randint(0, 9, shape, generator=g).float() / 8).to(torch.bfloat16).cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t if isinstance(t, int) else t.data_ptr() for t in ts])


# ---------------------------------------------------------------------------------------------------------------- (a) the grouped GEMM
# (G, batch, M, N, K, maps): maps[g] = which spike map group g reads.  What the single product picks for the shape (pick_cfg_nn,
# nn_super_steps in csrc/pgemm.hip): M <= 64 and N < 128 -> cfg 6; 512 or more 128 x 128 tiles -> cfg 7; else cfg 8; two K steps per
# barrier when K / 32 is even and >= 4 and the product has <= 512 workgroups (never on cfg 6).
GEMM_CASES = [
    pytest.param(3, 8, 256, 100, 256, (0, 0, 1), id="decoder-q-k-share-a-map-cfg8-two-steps"),
    pytest.param(1, 3, 48, 12, 96, (0,), id="one-group-less-than-a-tile-partly-filled-rows-cfg6"),
    pytest.param(2, 3, 256, 132, 96, (0, 1), id="partly-filled-second-column-tile-odd-k-steps-cfg8"),
    pytest.param(4, 8, 48, 132, 256, (0, 1, 2, 3), id="four-groups-partly-filled-rows-cfg8-two-steps"),
    pytest.param(4, 3, 256, 12, 256, (0, 1, 1, 0), id="four-groups-two-shared-maps-less-than-a-tile"),
    pytest.param(2, 64, 1024, 100, 128, (0, 1), id="512-tiles-cfg7-two-steps"),
    pytest.param(2, 64, 1024, 12, 96, (0, 0), id="512-tiles-cfg7-one-step"),
]


def gemm_operands(ops, G, B, M, N, K, maps, seed):
    g = torch.Generator().manual_seed(seed)
    ws = [(torch.randn(M, K, generator=g) * K ** -0.5).cuda() for _ in range(G)]
    xs = [spikes((B, K, N), g) for _ in range(max(maps) + 1)]
    return [ops.pack_weight(w) for w in ws], [xs[m] for m in maps], ws


@pytest.mark.parametrize("G,B,M,N,K,maps", GEMM_CASES)
def test_grouped_gemm_equals_single_calls(ops, G, B, M, N, K, maps):
    from spike2former_amd._lib import check, lib
    assert N % 8 != 0 and lib.s2f_pgemm_nn_grouped_ok(B, M, N, K) == 1
    packs, xs, _ = gemm_operands(ops, G, B, M, N, K, maps, seed=G * 1000 + M + N + K)
    y = torch.full((G + 1, B, M, N), float("nan"), device="cuda")          # (one slice more: nothing is written past the last group)
    check(lib.s2f_pgemm_nn_bf16_grouped(ptrs(packs), ptrs(xs), G, y.data_ptr(), B * M * N, B, M, N, K, stream()), "grouped")
    assert bool(torch.isnan(y[G]).all())
    for g in range(G):
        y1 = torch.full((B, M, N), float("nan"), device="cuda")
        check(lib.s2f_pgemm_nn_bf16(packs[g].data_ptr(), xs[g].data_ptr(), None, y1.data_ptr(), B, M, N, K, 3, 0, stream()), "single")
        assert not bool(torch.isnan(y1).any())
        assert torch.equal(y[g], y1), g


@pytest.mark.parametrize("fault,want", [("null-pack", EINVAL), ("unaligned-pack", EALIGN)])
def test_grouped_gemm_bad_last_group_writes_nothing(ops, fault, want):
    from spike2former_amd._lib import lib
    G, B, M, N, K = 3, 8, 256, 100, 256
    packs, xs, _ = gemm_operands(ops, G, B, M, N, K, (0, 0, 1), seed=7)
    table = [p.data_ptr() for p in packs]
    table[G - 1] = 0 if fault == "null-pack" else table[G - 1] + 2
    y = torch.full((G, B, M, N), -7.0, device="cuda")
    assert lib.s2f_pgemm_nn_bf16_grouped(ptrs(table), ptrs(xs), G, y.data_ptr(), B * M * N, B, M, N, K, stream()) == want
    assert lib.s2f_last_error() != b""
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())


def test_grouped_gemm_refuses_a_shape_of_the_dma_form(ops):
    """K >= 1024 with N % 8 == 0 runs on the all-DMA kernel in s2f_pgemm_nn_bf16: no grouped form, S2F_EINVAL before any launch"""
    from spike2former_amd._lib import lib
    G, B, M, N, K = 2, 2, 64, 128, 1024
    assert lib.s2f_pgemm_nn_grouped_ok(B, M, N, K) == 0
    packs, xs, _ = gemm_operands(ops, G, B, M, N, K, (0, 1), seed=8)
    y = torch.full((G, B, M, N), -7.0, device="cuda")
    assert lib.s2f_pgemm_nn_bf16_grouped(ptrs(packs), ptrs(xs), G, y.data_ptr(), B * M * N, B, M, N, K, stream()) == EINVAL
    assert lib.s2f_pgemm_nn_bf16_grouped(ptrs(packs), ptrs(xs), 5, y.data_ptr(), B * M * N, B, M, 100, 256, stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------- (b) the grouped BatchNorm
BN_SHAPES = [pytest.param(8, 256, 100, id="decoder-100-tokens"), pytest.param(3, 32, 12, id="one-round-of-groups-smallest-C"),
             pytest.param(2, 64, 1000, id="N-L-2000-just-below-2048")]


@pytest.mark.parametrize("G,with_gu", [(2, True), (3, False)])
@pytest.mark.parametrize("N,C,L", BN_SHAPES)
def test_grouped_batchnorm_equals_single_calls(N, C, L, G, with_gu):
    """forward: u, spikes, mask words, stat, running statistics; backward (spike gradient [+ gradient of u]): gz, dgamma, dbeta"""
    from spike2former_amd._lib import check, lib
    assert lib.s2f_bn_grouped_ok(N, C, L) == 1 and N * L <= 2048
    g = torch.Generator().manual_seed(N + C + L + G)
    z = (torch.randn(G, N, C, L, generator=g) * 2).cuda()
    bias, beta = (torch.randn(G * C, generator=g).cuda() * 0.1 for _ in range(2))
    gamma, rv0 = (torch.rand(G * C, generator=g).cuda() + 0.5 for _ in range(2))
    rm0 = torch.randn(G * C, generator=g).cuda() * 0.1
    g_u, g_y = (torch.randn(G, N, C, L, generator=g).cuda() for _ in range(2))
    mom, eps, vth, D = 0.1, 1e-5, 1.0, 8
    W = int(lib.s2f_bn_mask_words(N, C, L))
    dev = dict(device="cuda")

    def buffers(n):
        return dict(stat=torch.full((n, 3 * C), float("nan"), **dev), u=torch.full((n, N, C, L), float("nan"), **dev),
                    y=torch.full((n, N, C, L), -1.0, dtype=torch.bfloat16, **dev), mask=torch.full((n * W,), -1, dtype=torch.int64, **dev),
                    rm=rm0.clone(), rv=rv0.clone(), gz=torch.full((n, N, C, L), float("nan"), **dev),
                    dg=torch.full((n * C,), float("nan"), **dev), db=torch.full((n * C,), float("nan"), **dev))
    a, b = buffers(G), buffers(G)
    gu_a = g_u.data_ptr() if with_gu else None
    check(lib.s2f_bn_act_fwd_grouped(z.data_ptr(), bias.data_ptr(), a["stat"].data_ptr(), a["rm"].data_ptr(), a["rv"].data_ptr(),
                                     gamma.data_ptr(), beta.data_ptr(), a["u"].data_ptr(), a["y"].data_ptr(), a["mask"].data_ptr(), G,
                                     N, C, L, mom, eps, vth, D, 1, stream()), "fwd grouped")
    check(lib.s2f_bn_act_bwd_grouped(z.data_ptr(), bias.data_ptr(), a["stat"].data_ptr(), gamma.data_ptr(), gu_a, g_y.data_ptr(),
                                     a["mask"].data_ptr(), a["gz"].data_ptr(), a["dg"].data_ptr(), a["db"].data_ptr(), G, N, C, L, vth, D,
                                     stream()), "bwd grouped")
    for i in range(G):
        v = slice(i * C, (i + 1) * C)
        check(lib.s2f_bn_act_fwd(z[i].data_ptr(), bias[v].data_ptr(), None, b["stat"][i].data_ptr(), b["rm"][v].data_ptr(),
                                 b["rv"][v].data_ptr(), None, gamma[v].data_ptr(), beta[v].data_ptr(), None, b["u"][i].data_ptr(), None,
                                 b["y"][i].data_ptr(), None, b["mask"][i * W:].data_ptr(), None, N, C, L, mom, eps, 1, vth, D, 1, stream()),
              "fwd single")
        check(lib.s2f_bn_act_bwd(z[i].data_ptr(), bias[v].data_ptr(), b["stat"][i].data_ptr(), gamma[v].data_ptr(),
                                 g_u[i].data_ptr() if with_gu else None, g_y[i].data_ptr(), None, b["mask"][i * W:].data_ptr(), None,
                                 b["gz"][i].data_ptr(), None, b["dg"][v].data_ptr(), b["db"][v].data_ptr(), N, C, L, 1, vth, D, stream()),
              "bwd single")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(b["u"]).any()) and not bool((b["y"].float() == -1).any()) and not bool(torch.isnan(b["gz"]).any())
    assert not torch.equal(b["rm"], rm0) and bool(((b["y"].float() * 8).round() == b["y"].float() * 8).all())
    for name in a:
        # (the mask words of rounds past a channel's groups are never written: both sides keep the fill there)
        assert torch.equal(a[name].view(torch.int16 if name == "y" else a[name].dtype), b[name].view(torch.int16 if name == "y" else b[name].dtype)), name


@pytest.mark.parametrize("N,C,L", [pytest.param(8, 256, 1024, id="whole-256-element-tiles"), pytest.param(8, 256, 400, id="N-L-above-2048"),
                                   pytest.param(8, 16, 100, id="fewer-than-32-channels")])
def test_grouped_batchnorm_refuses_other_shapes(N, C, L):
    from spike2former_amd._lib import lib
    assert lib.s2f_bn_grouped_ok(N, C, L) == 0
    G = 2
    z = torch.randn(G, N, C, L, device="cuda")
    vec = torch.ones(G * C, device="cuda")
    stat, u = torch.full((G, 3 * C), -7.0, device="cuda"), torch.full((G, N, C, L), -7.0, device="cuda")
    assert lib.s2f_bn_act_fwd_grouped(z.data_ptr(), None, stat.data_ptr(), None, None, vec.data_ptr(), vec.data_ptr(), u.data_ptr(), None,
                                      None, G, N, C, L, 0.1, 1e-5, 1.0, 8, 0, stream()) == EINVAL
    assert lib.s2f_bn_act_bwd_grouped(z.data_ptr(), None, stat.data_ptr(), vec.data_ptr(), z.data_ptr(), None, None, u.data_ptr(),
                                      stat.data_ptr(), stat.data_ptr(), G, N, C, L, 1.0, 8, stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool((u == -7.0).all()) and bool((stat == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------- (c) the grouped dX
@pytest.mark.parametrize("G,B,M,K,L", [pytest.param(3, 8, 256, 256, 100, id="decoder-single-picks-64-row-steps"),
                                       pytest.param(2, 3, 48, 96, 12, id="ragged-both-pick-32-row-steps"),
                                       pytest.param(4, 3, 64, 32, 132, id="32-output-rows-tile")])
def test_grouped_input_gradient_in_the_group_outer_layout(ops, G, B, M, K, L):
    """dX[g][b] = W_g^T dY[g][b] with group strides B M L and B K L.  Bit-identical to the single calls when both run the same tile
    configuration; the single product of the decoder's shape takes 64-row contraction steps (cfg 10) where the grouped entry takes
    32-row steps (cfg 7) -- the same products in the same order, so equality is expected there too, and where it fails both sides are
    held to the allowance of test_pgemm_input_gradient_matches_fp64 in tests/test_gpu_kernels.py against an fp64 product:
    2e-6 * max(|W|^T |dY|)."""
    from spike2former_amd._lib import check, lib
    g = torch.Generator().manual_seed(G + B + M + K + L)
    ws = [(torch.randn(M, K, generator=g) * M ** -0.5).cuda() for _ in range(G)]
    gy = torch.randn(G, B, M, L, generator=g).cuda()
    packs = [ops.pack_weight(w) for w in ws]
    dx = torch.full((G, B, K, L), float("nan"), device="cuda")
    check(lib.s2f_pgemm_dx_f32_grouped(ptrs(packs), G, gy.data_ptr(), M * L, B * M * L, dx.data_ptr(), K * L, B * K * L, None, 0, B, M, K,
                                       L, stream()), "grouped")
    for i in range(G):
        d1 = torch.full((B, K, L), float("nan"), device="cuda")
        check(lib.s2f_pgemm_dx_f32(packs[i].data_ptr(), gy[i].data_ptr(), 0, d1.data_ptr(), 0, B, M, K, L, 0.0, 0, stream()), "single")
        same = torch.equal(dx[i], d1)
        print(f"G={G} B={B} M={M} K={K} L={L} group {i}: {'bit-identical to the single call' if same else 'compared against fp64'}")
        if not same:
            ref = torch.matmul(ws[i].t().double(), gy[i].double())
            bound = 2e-6 * torch.matmul(ws[i].t().abs().double(), gy[i].abs().double()).max().item()
            for name, t in (("grouped", dx[i]), ("single", d1)):
                err = (t.double() - ref).abs().max().item()
                print(f"  {name}: error {err:.3e}, bound {bound:.3e}")
                assert err <= bound, name


# ---------------------------------------------------------------------------------------------------------------- (d) the layer
# the parent against itself on atomically accumulated weight gradients: max|d| / max|ref| of profiles/sdsa_bwd_grouped_outputs.txt
WEIGHT_GRAD_BOUND = 1.381e-6


def make_layer(C=64, heads=4):
    import spike2former_amd as s2f
    from spike2former_amd import head_layers
    from spike2former_amd.init_utils import seeded_init
    layer = seeded_init(head_layers.DetrTransformerDecoderLayer(
        self_attn_cfg=dict(embed_dims=C, num_heads=heads, batch_first=True), cross_attn_cfg=dict(embed_dims=C, num_heads=heads, batch_first=True),
        ffn_cfg=dict(embed_dims=C, feedforward_channels=128, num_fcs=2))).cuda().train()
    s2f.set_keep_membrane(layer, False)          # the training step's setting: every neuron starts from rest and keeps no membrane
    return layer


def layer_inputs(ops, T, B, C, Nq, L=64):
    g = torch.Generator(device="cuda").manual_seed(Nq)
    q0 = torch.randn(T, B, C, Nq, device="cuda", generator=g) * 2
    pos0 = torch.randn(B, C, Nq, device="cuda", generator=g)
    mem = torch.randn(T * B, C, L, device="cuda", generator=g) * 2
    kpos = torch.randn(B, C, L, device="cuda", generator=g)
    lvl = torch.randn(C, device="cuda", generator=g) * 0.1
    wq = torch.randn(T, B, Nq, C, device="cuda", generator=g)
    yk, yv = ops.sum2_lif(mem, lvl, kpos, B, 8, 1.0)          # the cross-attention's key / value spikes (no gradient wanted)
    return q0, pos0, (yk.view(T, B, C, L), yv.view(T, B, C, L)), wq


def buffers_of(layer):
    return {k: v.clone() for k, v in layer.named_buffers()}


def restore(layer, buffers):
    """running statistics and counters back in place (the parameters never change here: their cached packs stay valid)"""
    with torch.no_grad():
        for k, v in layer.named_buffers():
            v.copy_(buffers[k])


def run_layer(layer, q, pos, kv, wq):
    import spike2former_amd as s2f
    s2f.reset_net(layer)
    out, _ = layer.forward_stream(q, pos, kv_spikes=kv, last=True)
    (out * wq).sum().backward()
    return out


@pytest.mark.parametrize("Nq", [12, 100])
def test_decoder_layer_siblings_on_equals_off(ops, Nq, monkeypatch):
    """T B = 4, embed 64, 4 heads, train mode: outputs, running statistics and the gradients of query, pos and every 1-d parameter
    (BatchNorm affine pairs) bit-identical; weight gradients within the parent's own run-to-run bound"""
    from spike2former_amd import head_layers
    T, B, C = 2, 2, 64
    layer = make_layer(C)
    state0 = buffers_of(layer)
    q0, pos0, kv, wq = layer_inputs(ops, T, B, C, Nq)
    calls = []
    real = head_layers.MultiHeadAttentionBlock._project_siblings
    monkeypatch.setattr(head_layers.MultiHeadAttentionBlock, "_project_siblings", lambda self, *a: (calls.append(1), real(self, *a))[1])
    res = {}
    was = ops.cfg.DECODER_SIBLINGS
    try:
        for flag in (True, False):
            ops.cfg.DECODER_SIBLINGS = flag
            restore(layer, state0)
            layer.zero_grad(set_to_none=True)
            q, pos = q0.clone().requires_grad_(True), pos0.clone().requires_grad_(True)
            n_before = len(calls)
            out = run_layer(layer, q, pos, kv, wq)
            assert len(calls) - n_before == (1 if flag else 0)          # the self-attention alone takes the sibling path
            res[flag] = (out.detach().clone(), q.grad.clone(), pos.grad.clone(), buffers_of(layer),
                         {n: p.grad.clone() for n, p in layer.named_parameters() if p.grad is not None})
    finally:
        ops.cfg.DECODER_SIBLINGS = was
    on, off = res[True], res[False]
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]) and torch.equal(on[2], off[2])
    assert on[1].abs().max().item() > 0 and on[2].abs().max().item() > 0
    bns = [k for k in on[3] if k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
    assert len(bns) == 3 * 10 and all(torch.equal(on[3][k], off[3][k]) for k in bns)          # 4 + 4 attention BatchNorms, 2 of the FFN
    assert not torch.equal(on[3]["self_attn.attn.k_conv.1.running_mean"], state0["self_attn.attn.k_conv.1.running_mean"])
    assert all(int(on[3][k]) == 1 for k in bns if k.endswith("num_batches_tracked"))
    assert on[4].keys() == off[4].keys() and any(n.startswith("self_attn.attn.q_conv.1") for n in on[4])
    for n, a in on[4].items():
        b = off[4][n]
        if a.dim() == 1:
            assert torch.equal(a, b), n
        else:
            d, ref = (a - b).abs().max().item(), b.abs().max().item()
            print(f"Nq={Nq} {n}: max|d| {d:.3e}, max|ref| {ref:.3e}")
            assert d <= WEIGHT_GRAD_BOUND * ref, n


def test_decoder_layer_siblings_graph_replay_equals_eager(ops):
    """forward + backward of the layer captured once (one stream, no parallel branches) and replayed: outputs, gradients and updated
    running statistics equal the eager pass from the same state"""
    T, B, C, Nq = 2, 2, 64, 100
    layer = make_layer(C)
    state0 = buffers_of(layer)
    q0, pos0, kv, wq = layer_inputs(ops, T, B, C, Nq)
    q, pos = q0.clone().requires_grad_(True), pos0.clone().requires_grad_(True)

    def grads():
        return [q.grad.clone(), pos.grad.clone()] + [p.grad.clone() for p in layer.parameters() if p.grad is not None]

    def fresh():
        restore(layer, state0)
        layer.zero_grad(set_to_none=True)
        q.grad = pos.grad = None
    fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # eager, and the warm-up of the capture: weights packed, buffers laid out
        out_e = run_layer(layer, q, pos, kv, wq).detach().clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    grads_e = grads()
    state_e = buffers_of(layer)
    fresh()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g = run_layer(layer, q, pos, kv, wq)
    restore(layer, state0)                                          # (in place: the captured addresses stay)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_g, out_e)
    for k, v in layer.named_buffers():
        assert torch.equal(v, state_e[k]), k
    got = grads()
    assert len(got) == len(grads_e)
    for i, (a, b) in enumerate(zip(got, grads_e)):
        if a.dim() <= 1 or i < 2:
            assert torch.equal(a, b), i
        else:
            assert (a - b).abs().max().item() <= WEIGHT_GRAD_BOUND * b.abs().max().item(), i
    del graph
