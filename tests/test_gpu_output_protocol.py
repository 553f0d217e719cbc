"""The output protocol of the Functions that produce spike maps (ops.core._Outputs), read off each Function's raw `.apply`: exactly
the autograd handles, the fp32 spikes and the requested fp32 outputs hang off the node (grad_fn); every stand-in of an output that
was not requested, every bf16 data tensor and BatchNorm's border do not require grad.  Each Function runs with cfg.SPIKES_BF16 and
cfg.FANOUT_PORTS on and off, at one small shape per kernel form; a row asserts the predicate that puts it on that form."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

GRAD, FIXED, NONE = "differentiable", "data without a gradient", "stand-in"


@pytest.fixture(scope="module")
def ops():
    from spike2former_amd import ops
    return ops


@pytest.fixture(params=[(True, True), (True, False), (False, True), (False, False)], ids=lambda m: f"bf16={int(m[0])}-ports={int(m[1])}")
def mode(request, ops):
    was = ops.SPIKES_BF16, ops.FANOUT_PORTS
    ops.SPIKES_BF16, ops.FANOUT_PORTS = request.param
    yield request.param
    ops.SPIKES_BF16, ops.FANOUT_PORTS = was


def triple(lif, bf16, spare):
    """what _Outputs.spikes appends: (handle, bf16 data, spare handle), (fp32 spikes, -, -) or three stand-ins"""
    if not lif:
        return [NONE] * 3
    return [GRAD, FIXED, GRAD if spare else NONE] if bf16 else [GRAD, NONE, NONE]


def assert_protocol(outs, want, what):
    assert len(outs) == len(want), what
    for i, (o, w) in enumerate(zip(outs, want)):
        where = f"{what}: output {i} ({w})"
        assert (o.grad_fn is not None) == (w == GRAD) and o.requires_grad == (w == GRAD), where
        assert (o.numel() == 0) == (w == NONE), where


def leaf(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * 4).cuda().requires_grad_()


def flags(*names):
    return [dict(zip(names, v)) for v in itertools.product((False, True), repeat=len(names))]


# ------------------------------------------------------------------------------------------------------------------ neurons
@pytest.mark.parametrize("shape", [(2, 8, 16), (1, 3, 5)], ids=["one-mask-tile", "n-not-a-multiple-of-4"])
def test_lif(ops, mode, shape):
    from spike2former_amd.ops.neuron import _LIF
    n = shape[0] * shape[1] * shape[2]
    if shape == (2, 8, 16):
        assert ops.mask_words(n) == 4          # one 256-element tile
    bf16 = ops.spikes_bf16_ok(8) and n % 4 == 0          # (ops.lif: bf16 spikes are stored in 8-byte groups)
    assert bf16 == (mode[0] and shape == (2, 8, 16))
    s, _ = ops.lif(leaf(*shape), keep_v=False, spikes=True)          # the wrapper's own decision: bf16 asked for, fp32 where n % 4 != 0
    assert isinstance(s, ops.Spikes) and (s.tok is not None) == bf16 and s.data.dtype == (torch.bfloat16 if bf16 else torch.float32)
    assert (s.tok2 is not None) == (bf16 and mode[1]) and s.requires_grad and not (bf16 and s.data.requires_grad)
    for f in flags("keep_v", "skip", "v_in"):
        x, v_in = leaf(*shape), (leaf(*shape, seed=1) if f["v_in"] else None)
        outs = _LIF.apply(x * 1.0, v_in, 8, 1.0, f["keep_v"], None, bf16, f["skip"])
        want = triple(True, bf16, mode[1]) + [GRAD if f["keep_v"] else NONE, GRAD if f["skip"] else NONE]
        assert_protocol(outs, want, f"_LIF {f}")


def test_lif_leaky(ops, mode):
    from spike2former_amd.ops.neuron import _LIFLeaky
    assert ops.mask_words(2 * 8 * 16) == 4
    for f in flags("keep_v", "v_in"):
        x, v_in = leaf(2, 8, 16), (leaf(2, 8, 16, seed=1) if f["v_in"] else None)
        outs = _LIFLeaky.apply(x * 1.0, v_in, 8, 1.0, 2.0, True, f["keep_v"], None)
        assert_protocol(outs, [GRAD, GRAD if f["keep_v"] else NONE], f"_LIFLeaky {f}")


def test_sum2_lif(ops, mode):
    from spike2former_amd.ops.neuron import _Sum2LIF
    bf16 = ops.spikes_bf16_ok(8)
    for f in flags("skip"):
        x, e, pos = leaf(4, 8, 16), leaf(8), leaf(2, 8, 16)
        outs = _Sum2LIF.apply(x * 1.0, e, pos, 2, 8, 1.0, bf16, f["skip"])
        assert_protocol(outs, 2 * triple(True, bf16, mode[1]) + [GRAD if f["skip"] else NONE], f"_Sum2LIF {f}")


# ------------------------------------------------------------------------------------------------------------------ BatchNorm
def bn_params(C, dev="cuda"):
    g = torch.Generator().manual_seed(C)
    w = (torch.rand(C, generator=g) + 0.5).to(dev).requires_grad_()
    b = (torch.randn(C, generator=g) * 0.1).to(dev).requires_grad_()
    return w, b, torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.zeros((), dtype=torch.int64, device=dev)


BN_ROWS = [
    pytest.param((2, 32, 8, 8), None, lambda lib, N, C, L: lib.s2f_bn_grouped_ok(N, C, L) and lib.s2f_bn_single_pass(N, C, L),
                 id="short-rows"),
    pytest.param((2, 64, 16, 32), None, lambda lib, N, C, L: lib.s2f_bn2_fused_ok(N, C, L) and lib.s2f_bn_single_pass(N, C, L),
                 id="single-pass"),
    pytest.param((1, 8, 32, 32), (1, 8, 16, 16), lambda lib, N, C, L: not lib.s2f_bn_single_pass(N, C, L), id="row-walking-up"),
]


@pytest.mark.parametrize("shape,lo_shape,on_route", BN_ROWS)
def test_bn_act(ops, mode, shape, lo_shape, on_route):
    from spike2former_amd._lib import lib
    from spike2former_amd.ops.bn import _BNAct
    N, C = shape[:2]
    assert on_route(lib, N, C, shape[2] * shape[3])
    for f in flags("lif", "want_pre", "keep_v", "lo_skip"):
        if not (f["lif"] or f["want_pre"]) or (f["keep_v"] and not f["lif"]) or (f["lo_skip"] and lo_shape is None):
            continue          # (the kernel wants u or y; a membrane belongs to a neuron; the pass-through to a low-resolution residual)
        z, lo = leaf(*shape), (None if lo_shape is None else leaf(*lo_shape))
        if lo is not None:
            assert ops.bn_up_ok(z, lo, True, 8)
        w, b, rm, rv, nbt = bn_params(C)
        bf16 = f["lif"] and ops.spikes_bf16_ok(8) and z.numel() % 4 == 0          # (ops.bn_act)
        port = lo is not None and f["lo_skip"] and ops.FANOUT_PORTS
        outs = _BNAct.apply(z * 1.0, None, w, b, None, None, rm, rv, nbt, True, 0.1, 1e-5, f["lif"], f["want_pre"], f["keep_v"], 8, 1.0,
                            None, bf16, None, None if lo is None else lo * 1.0, port)
        want = ([GRAD if f["want_pre"] else NONE] + triple(f["lif"], bf16, mode[1])
                + [GRAD if f["keep_v"] else NONE, FIXED, GRAD if port else NONE])
        assert_protocol(outs, want, f"_BNAct {f}")
        assert outs[5].shape == (C,)          # border = BN(0), for BNAndPadLayer's padding: a value, no autograd edge


def test_bn_act_siblings(ops, mode):
    from spike2former_amd.ops.bn import _BNAct
    G, N, C, L = 3, 2, 32, 16
    for f in flags("lif", "want_pre")[1:]:          # (the kernel wants u or y)
        z = leaf(G, N, C, L)
        assert ops.bn_siblings_ok(z)
        w, b, rm, rv, _ = bn_params(G * C)
        bf16 = f["lif"] and ops.spikes_bf16_ok(8) and z[0].numel() % 4 == 0          # (ops.bn_act_siblings)
        outs = _BNAct.apply(z * 1.0, None, w, b, None, None, rm, rv, None, True, 0.1, 1e-5, f["lif"], f["want_pre"], False, 8, 1.0, None,
                            bf16, None, None, False, G)
        want = [GRAD if f["want_pre"] else NONE] + triple(f["lif"], bf16, False) + [NONE, FIXED, NONE]
        assert_protocol(outs, want, f"_BNAct siblings {f}")
        assert outs[5].shape == (G, C)


def test_bn2_act(ops, mode):
    from spike2former_amd.ops.bn import _BN2Act
    N, C, H, W = 2, 64, 16, 32
    for f in flags("lif", "want_pre", "keep_v"):
        if not (f["lif"] or f["want_pre"]) or (f["keep_v"] and not f["lif"]):
            continue
        z = leaf(N, C, H, W)
        assert ops.bn2_act_ok(z)
        (w1, b1, rm1, rv1, nbt1), (w2, b2, rm2, rv2, nbt2) = bn_params(C), bn_params(C)
        bf16 = f["lif"] and ops.spikes_bf16_ok(8) and z.numel() % 4 == 0          # (ops.bn2_act)
        outs = _BN2Act.apply(z * 1.0, w1, b1, w2, b2, None, None, rm1, rv1, nbt1, 0.1, 1e-5, rm2, rv2, nbt2, 0.1, 1e-5, f["lif"],
                             f["want_pre"], f["keep_v"], 8, 1.0, None, bf16)
        want = [GRAD if f["want_pre"] else NONE] + triple(f["lif"], bf16, False) + [GRAD if f["keep_v"] else NONE]
        assert_protocol(outs, want, f"_BN2Act {f}")


# ------------------------------------------------------------------------------------------------------------------ attention
def test_sdsa_spikes(ops, mode):
    """the smallest fused row of tests/test_gpu_attention.py (packed-d9): q | k | v stacked in one bf16 map with one handle"""
    from spike2former_amd.ops.attention import _SDSASpikes
    TB, heads, d, N = 2, 4, 9, 256
    C = heads * d
    assert 8 < d <= 32 and N % 256 == 0 and (C * N) % 8 == 0
    g = torch.Generator().manual_seed(9256)
    qkv = (torch.randint(0, 9, (TB, 3 * C, N), generator=g) * (torch.rand(TB, 3 * C, N, generator=g) < 0.3)).div(8).bfloat16().cuda()
    for fuse in (True, False):
        tok = ops._new_tok(qkv).clone().requires_grad_()
        outs = _SDSASpikes.apply(qkv, None, None, tok, None, None, heads, 0.125, True, fuse, 8, 1.0, None)
        assert_protocol(outs, triple(True, fuse, False), f"_SDSASpikes fuse={fuse}")
        assert outs[0].shape == (TB, C, N) and (outs[1].dtype == torch.bfloat16) == fuse
