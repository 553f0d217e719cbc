"""CPU: registry surface, checkpoint ABI (state_dict keys), neuron bookkeeping, no-fallback behaviour."""
import numpy as np
import pytest
import torch

import spike2former_amd as s2f
from oracle import s2f_oracle as so


@pytest.fixture(scope="module")
def tiny():
    return s2f.MODELS.build(s2f.model_cfg("C1_64"))


def test_registry_type_strings():
    for name in ("Spiking_vit_MetaFormer", "MaskFormerHead", "mmdet.DCNTransformerEncoderPixelDecoder",
                 "EncoderDecoder"):
        assert s2f.MODELS.get(name) is not None
    assert s2f.HOOKS.get("ResetModelHook") is not None
    with pytest.raises(KeyError):
        s2f.MODELS.build(dict(type="NoSuchModel"))
    with pytest.raises(TypeError):
        s2f.MODELS.build(dict(foo=1))


def test_state_dict_is_the_reference_checkpoint_abi(tiny):
    want = so.param_shapes(so.CONFIGS["C1_64"])
    got = {k: tuple(v.shape) for k, v in tiny.state_dict().items()}
    assert got == {k: tuple(v) for k, v in want.items()}
    full = s2f.MODELS.build(s2f.model_cfg("C2"))
    sd = full.state_dict()
    for k in ("backbone.block3.0.attn.q_conv.0.body.0.weight", "backbone.block3.0.attn.q_conv.0.body.1.bn.weight",
              "decode_head.pixel_decoder.encoder.layers.0.dcn.offset.0.weight", "decode_head.mask_embed.fc1.weight",
              "decode_head.w", "decode_head.transformer_decoder.layers.5.cross_attn.attn.k_conv.0.weight"):
        assert k in sd
    assert sd["decode_head.pixel_decoder.encoder.layers.0.dcn.offset.0.weight"].shape == (576, 256, 1, 1)
    assert sum(p.numel() for p in full.parameters()) == 34_361_112
    assert not any("spike" in k for k in sd)            # neurons contribute no keys


def test_seeded_state_loads_strictly(tiny):
    st = so.make_params(so.CONFIGS["C1_64"], requires_grad=False)
    tiny.load_state_dict(st, strict=True)


def test_neuron_order_matches_reference_named_modules(tiny, golden):
    g = golden("e2e_C1_64.npz")
    names = [n for n, m in tiny.named_modules() if isinstance(m, s2f.Q_IFNode)]
    assert names == list(g["lif_names_all"])
    assert len(names) == 151 and "decode_head.pixel_decoder.encoder_in_proj_spike" in names


def test_reset_and_membrane_bookkeeping(tiny):
    n = s2f.Q_IFNode(surrogate_function=s2f.Quant())
    assert n.v == 0.0 and n.D == 8 and "v" not in n.state_dict()
    n.v = torch.ones(3)
    s2f.reset_net(n)
    assert n.v == 0.0
    s2f.set_keep_membrane(tiny, False)
    assert not any(m.keep_membrane for m in tiny.modules() if isinstance(m, s2f.Q_IFNode))
    with pytest.raises(NotImplementedError):
        s2f.Q_IFNode(detach_reset=True)


def test_no_cpu_fallback(tiny):
    with pytest.raises(RuntimeError, match="GPU only"):
        s2f.Q_IFNode()(torch.zeros(8))
    with pytest.raises(RuntimeError, match="GPU only"):
        tiny(torch.zeros(1, 3, 64, 64))
    with pytest.raises(RuntimeError, match="GPU only"):         # the real loss runs the same (GPU-only) forward
        tiny(torch.zeros(1, 3, 64, 64), [torch.zeros(1, 64, 64, dtype=torch.long)], mode="loss")


def test_constructor_errors_mirror_the_reference():
    from spike2former_amd.backbone_sdtv2 import MS_Attention_RepConv_qkv_id
    from spike2former_amd.head_layers import DCNv3_pytorch
    with pytest.raises(AssertionError, match="should be divided by num_heads"):
        MS_Attention_RepConv_qkv_id(30, num_heads=8)
    with pytest.raises(ValueError, match="channels must be divisible by group"):
        DCNv3_pytorch(channels=30, group=4)


def test_workloads_agree_with_oracle_configs():
    for name, w in s2f.WORKLOADS.items():
        if "backbone" in w:            # E-SpikeFormer workloads (row f3): pinned by the reference's vectors, not by the oracle port
            continue
        c = so.CONFIGS[name]
        assert (w["H"], w["W"], w["T"], w["B"], w["K"]) == (c.H, c.W, c.T, c.B, c.num_classes)
        assert tuple(w["embed_dim"]) == tuple(c.embed_dim) and w["Fc"] == c.feat_channels and w["Q"] == c.num_queries
        assert w["pd"] == (c.pd_layers, c.pd_ffn) and w["dec"] == (c.dec_layers, c.dec_ffn) and w["G"] == c.group


def test_shard_batch():
    from spike2former_amd.dist import shard_batch
    assert [shard_batch(16, r, 8) for r in (0, 7)] == [(0, 2), (14, 2)]
    with pytest.raises(ValueError):
        shard_batch(6, 0, 4)


def test_flat_grad_buffer_sinks_and_compaction():
    """Gradient sinks (dist.FlatGradAllReduce.install_sinks / compact): parameters whose gradient is accumulated straight
    into the flat buffer by a kernel (p.grad stays None) are moved behind the others, packing the rest stays one batched
    copy over the leading region, and the sunk slices are left untouched; without sinks a missing gradient packs as zeros."""
    import torch

    from spike2former_amd import ops
    from spike2former_amd.dist import FlatGradAllReduce
    ps = [torch.nn.Parameter(torch.randn(n)) for n in (3, 5, 2, 4)]
    red = FlatGradAllReduce(ps, world_size=1)
    # no sinks: None -> zeros (not the stale content of the slice)
    red.flat.fill_(7.0)
    red.zero()
    ps[0].grad, ps[2].grad = torch.ones(3), torch.full((2,), 2.0)
    red.gather()
    # slots are padded to 16 bytes (4 floats): 3 -> 4, 5 -> 8, 2 -> 4, 4 -> 4; the pads stay zero
    Z = [0.0]
    assert red.offsets == [0, 4, 12, 16] and all(v.data_ptr() % 16 == 0 for v in red.views)
    assert red.flat.tolist() == [1.0] * 3 + Z + [0.0] * 8 + [2.0] * 2 + Z * 2 + [0.0] * 4
    try:
        red.install_sinks()
        assert set(ops.GRAD_SINKS) == {p.data_ptr() for p in ps}
        # step 1: "kernels" add into the sinks of parameters 1 and 3, autograd assigns the others
        red.zero()
        assert float(red.flat.abs().sum()) == 0.0
        ops._sink_for(ps[1]).add_(torch.arange(5.0))
        ops._sink_for(ps[3]).add_(1.5)
        ps[0].grad, ps[2].grad = torch.ones(3), torch.full((2,), 2.0)
        red.gather()                                       # not compacted yet: one copy per run
        assert red.flat.tolist() == [1.0] * 3 + Z + [0.0, 1.0, 2.0, 3.0, 4.0] + Z * 3 + [2.0] * 2 + Z * 2 + [1.5] * 4
        red.compact()
        assert [p.numel() for p in red.params] == [3, 2, 5, 4] and red._dense_elems == 8 and red.offsets == [0, 4, 8, 16]
        assert all(v.data_ptr() % 16 == 0 for v in red.views)
        # step 2 in the compacted layout
        red.zero()
        ops._sink_for(ps[1]).add_(torch.arange(5.0))
        ops._sink_for(ps[3]).add_(1.5)
        ps[0].grad, ps[2].grad = torch.ones(3), torch.full((2,), 2.0)
        red.gather()
        assert red.flat.tolist() == [1.0] * 3 + Z + [2.0] * 2 + Z * 2 + [0.0, 1.0, 2.0, 3.0, 4.0] + Z * 3 + [1.5] * 4
        for p, v in zip(red.params, red.views):
            assert v.shape == p.shape and ops._sink_for(p).data_ptr() == v.data_ptr()
        # a parameter that changes sides after compact() (unused on an iteration; a tensor gradient for a sunk weight) loses nothing:
        # the packing falls back to one copy per run of gradient tensors and leaves every slot without a tensor alone
        red.zero()
        ops._sink_for(ps[3]).add_(1.5)
        ps[0].grad, ps[2].grad, ps[1].grad = torch.ones(3), torch.full((2,), 2.0), torch.ones(5)      # sunk parameter, tensor gradient
        red.gather()
        assert red.flat.tolist() == [1.0] * 3 + Z + [2.0] * 2 + Z * 2 + [1.0] * 5 + Z * 3 + [1.5] * 4
        red.zero()
        ops._sink_for(ps[1]).add_(torch.arange(5.0))
        ops._sink_for(ps[2]).add_(4.0)               # a kernel added into a DENSE parameter's slot and autograd assigned no tensor
        ps[0].grad = torch.ones(3)
        red.gather()
        assert red.flat.tolist() == [1.0] * 3 + Z + [4.0] * 2 + Z * 2 + [0.0, 1.0, 2.0, 3.0, 4.0] + Z * 3 + [0.0] * 4
        # an address is not an identity: a sink is only handed to the parameter it was registered for, and dropping the
        # buffer detaches the (process-global) table
        stale = torch.nn.Parameter(torch.zeros(5))
        assert ops._sink_for(stale) is None
        red.close()
        assert ops.GRAD_SINKS is None and ops._sink_for(ps[1]) is None
    finally:
        ops.GRAD_SINKS = None


def test_register_upstream_fills_the_reference_registries(monkeypatch):
    """register_upstream() (registry level): with mmseg / mmdet importable, the classes of this package take the
    reference's type names in THEIR registries (`register_module(name=, module=, force=True)`, the mmengine Registry call the
    reference's own modules use: mmseg/models/backbones/sdtv2.py:424, mmdet/models/layers/pixel_decoder.py:316).  mmengine is not
    in this image, so stand-ins with that one method are put on sys.modules; the names must also build through them."""
    import sys
    import types
    import spike2former_amd as s2f

    class FakeRegistry:
        def __init__(self):
            self.modules, self.forced = {}, []

        def register_module(self, name=None, force=False, module=None):
            assert module is not None and isinstance(name, str)
            if name in self.modules and not force:
                raise KeyError(name)
            self.modules[name] = module
            self.forced.append(force)

    regs = {}
    for pkg in ("mmseg", "mmdet"):
        root, reg = types.ModuleType(pkg), types.ModuleType(pkg + ".registry")
        reg.MODELS = regs[pkg] = FakeRegistry()
        root.registry = reg
        monkeypatch.setitem(sys.modules, pkg, root)
        monkeypatch.setitem(sys.modules, pkg + ".registry", reg)
    regs["mmseg"].modules["MaskFormerHead"] = object          # the reference's own class is replaced (force=True), not an error
    done = s2f.register_upstream()
    assert set(regs["mmseg"].modules) == {"Spiking_vit_MetaFormer", "Spiking_vit_MetaFormerv2", "MaskFormerHead", "EncoderDecoder",
                                          "SegDataPreProcessor"}
    assert set(regs["mmdet"].modules) == {"DCNTransformerEncoderPixelDecoder"}
    assert all(regs["mmseg"].forced) and all(regs["mmdet"].forced) and len(done) == 6
    for reg in regs.values():
        for name, cls in reg.modules.items():
            assert cls is s2f.MODELS.get(name) and cls.__module__.startswith("spike2former_amd")
    # without the packages: nothing to do, no error
    for pkg in ("mmseg", "mmdet"):
        monkeypatch.setitem(sys.modules, pkg, None)
        monkeypatch.setitem(sys.modules, pkg + ".registry", None)
    assert s2f.register_upstream() == []


def test_spike_map_handles_for_a_second_reader():
    """ops.Spikes: `second()` hands out the producing neuron's spare autograd handle (cfg.FANOUT_PORTS: the backward kernel sums the
    two readers' gradients) and keeps handing out that one to later readers; views carry both handles; without a spare handle the map
    itself is returned (the autograd engine then adds, as before)."""
    import torch
    from spike2former_amd import ops
    data = torch.zeros(2, 4, 8, dtype=torch.bfloat16)
    tok, tok2 = torch.zeros(()).expand(2, 4, 8), torch.ones(()).expand(2, 4, 8)
    s = ops.Spikes(data, tok, tok2)
    assert s.second().tok is tok2 and s.second().second().tok is tok2 and s.second().data is data
    v = s.view(8, 8)
    assert v.tok.shape == (8, 8) and v.tok2.shape == (8, 8) and v.second().tok.shape == (8, 8)
    assert float(v.second().tok.sum()) == 64.0 and float(v.tok.sum()) == 0.0
    plain = ops.Spikes(data, tok)
    assert plain.second() is plain and plain.flatten(0, 1).tok2 is None
    assert ops.Spikes(data).second().tok is None


def test_bench_plain_run_and_dump_outputs(tmp_path, monkeypatch):
    """bench.py: the secondary measurements run only under --full; --dump-outputs writes float32 files of at most 64 MB in all,
    and a large output's sample is the same elements in every run."""
    import os
    import sys

    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7"])
    a = bench.parse()
    assert a.steps == 7 and not a.full and a.no_cpu_baseline and a.no_kernel_events
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    a = bench.parse()
    assert a.full and not a.no_cpu_baseline and not a.no_kernel_events
    big = torch.randn(40_000_000, generator=torch.Generator().manual_seed(0))
    outs = {"loss": torch.tensor(0.25), "cls": torch.ones(2, 3, dtype=torch.bfloat16), "grads": big}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["cls.npy", "grads_sample.npy", "loss.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64e6
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float32 and np.array_equal(x, y)
    assert np.load(tmp_path / "a" / "cls.npy").shape == (2, 3)
    s = np.load(tmp_path / "a" / "grads_sample.npy")
    assert np.isin(s, big.numpy()).all()


def _walk(shape, strides):
    """every operand's element offsets over the index space, in row-major index order"""
    idx = np.indices(shape).reshape(len(shape), -1) if shape else np.zeros((0, 1), dtype=np.int64)
    return [tuple(np.asarray(st, dtype=np.int64) @ idx) for st in strides]


@pytest.mark.parametrize("shape,strides,want_dims", [
    ((4, 5, 6), [(30, 6, 1), (30, 6, 1)], 1),                                  # contiguous: one dimension
    ((4, 1, 5, 1, 6), [(30, 30, 6, 6, 1), (30, 7, 6, 1, 1)], 1),                # extent-1 dimensions dropped, whatever their strides
    ((1, 1, 1), [(1, 1, 1), (5, 2, 9)], 1),                                    # nothing left: one dimension of extent 1
    ((4, 5, 6), [(30, 6, 1), (1, 4, 20)], 3),                                  # permuted operand: nothing merges
    ((4, 5, 6), [(30, 6, -1), (30, 6, 1)], 2),                                 # h_flip's inner flip: a negative stride does not merge
    ((4, 5, 6), [(-30, -6, -1), (30, 6, 1)], 1),                               # every dimension flipped: a reversed walk, one dimension
    ((4, 5, 6), [(-30, 6, 1), (30, 6, 1)], 2),                                 # outer flip: the inner pair still merges
    ((4, 5, 6), [(0, 6, 1), (30, 6, 1)], 2),                                   # broadcast outer: it stops a merge with the rest
    ((4, 5, 6), [(6, 0, 1), (30, 6, 1)], 3),                                   # broadcast middle
    ((4, 5, 6), [(0, 0, 0), (30, 6, 1)], 1),                                   # 0-dim operand broadcast everywhere
    ((4, 5, 6), [(0, 0, 1), (30, 6, 1)], 2),
    ((2, 3, 2, 3, 2, 3), [(1, 2, 6, 12, 36, 72), (108, 36, 18, 6, 3, 1)], 6),  # a fully reversed permutation keeps six dimensions
])
def test_glue_coalesce_keeps_every_operands_offsets(shape, strides, want_dims):
    """glue_mode._coalesce: merged dimensions address exactly the elements, in the same order, for every operand -- and adjacent
    dimensions merge only where every operand walks them contiguously (a broadcast or flipped operand stops a merge)"""
    from spike2former_amd.ops import glue
    size, cs = glue._coalesce(shape, [list(s) for s in strides])
    assert len(size) == want_dims and (all(n > 1 for n in size) or size == [1])
    assert int(np.prod(size)) == int(np.prod(shape))
    assert _walk(list(size), cs) == _walk(list(shape), strides)


def test_glue_coalesce_on_flip_strides():
    """the strides h_flip builds (negated on the flipped dimensions, base at the far corner) coalesce to the same walk"""
    from spike2former_amd.ops import glue
    x = torch.arange(120.).view(2, 3, 4, 5)
    for dims in [(3,), (0,), (0, 1, 2, 3), (1, 2), (-1, 0)]:
        sa, off = list(x.stride()), 0
        for d in {d % 4 for d in dims}:
            off += (x.shape[d] - 1) * sa[d]
            sa[d] = -sa[d]
        size, (ca, co) = glue._coalesce(tuple(x.shape), [sa, [60, 20, 5, 1]])
        got = torch.empty(120)
        got[np.array(_walk(size, [co])[0])] = x.flatten()[off + np.array(_walk(size, [ca])[0])]
        assert torch.equal(got, torch.flip(x, dims).flatten()), dims


def _aten_shape(fn):
    try:
        return list(fn().shape)
    except (RuntimeError, IndexError, ValueError):
        return None


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_glue_shape_checks_match_aten(device):
    """the host checks in front of GlueMode's cat / cat.out / stack / constant_pad_nd launches: the shape ATen computes, and None
    exactly where ATen refuses the call -- mismatched pieces never reach s2f_copy_segments / s2f_ew (they would write past `out`)"""
    from spike2former_amd.ops import glue
    mk = lambda *s: torch.empty(s, device=device)          # noqa: E731
    cats = [([(2, 3), (4, 3)], 0), ([(2, 3), (2, 5)], 1), ([(2, 3), (2, 5)], -1), ([(2, 3), (4, 4)], 0), ([(2, 3), (2, 4)], 0),
            ([(2, 3), (3,)], 0), ([(2, 3), (0,), (1, 3)], 0), ([(0,), (2, 3)], 1), ([(0,), (0,)], 0), ([(2, 3)], 2), ([(2, 3)], -3),
            ([(), ()], 0), ([(2, 3, 4), (2, 3, 4)], 1), ([(2, 3, 4), (2, 4, 4)], 2), ([(1, 4), (2, 4), (3, 4)], 0), ([(4, 0), (4, 2)], 1)]
    for shapes, dim in cats:
        want = _aten_shape(lambda: torch.cat([mk(*s) for s in shapes], dim))
        if want == [0]:
            want = None          # (only legacy empty pieces: nothing to route)
        assert glue.cat_shape(shapes, dim) == want, (shapes, dim)
        # cat.out: h_cat_out takes the call only for an `out` of exactly that shape
        if want is not None:
            out = mk(*want)
            assert list(torch.cat([mk(*s) for s in shapes], dim, out=out).shape) == want
    stacks = [([(2, 3), (2, 3)], 0), ([(2, 3), (2, 3)], 1), ([(2, 3), (2, 3)], 2), ([(2, 3), (2, 3)], -1), ([(2, 3), (2, 3)], 3),
              ([(2, 3), (2, 3)], -4), ([(2, 3), (3, 2)], 0), ([(2, 3), (2, 3, 1)], 0), ([], 0), ([(), ()], 0)]
    for shapes, dim in stacks:
        want = _aten_shape(lambda: torch.stack([mk(*s) for s in shapes], dim))
        assert glue.stack_shape(shapes, dim) == want, (shapes, dim)
    pads = [((2, 3), [1, 2]), ((2, 3), [1, 2, 3, 4]), ((2, 3), [1, 2, 3, 4, 5, 6]), ((2, 3), [1]), ((2, 3, 4), [0, 0, 2, 0]),
            ((5,), [3, 3]), ((5,), [1, 1, 1, 1]), ((), [1, 1]), ((2, 3), [])]
    for shape, pad in pads:
        want = _aten_shape(lambda: torch.constant_pad_nd(mk(*shape), pad))
        assert glue.pad_shape(shape, pad) == want, (shape, pad)
    # negative padding crops in ATen; the glue leaves it to ATen
    assert glue.pad_shape((4, 4), [-1, 0]) is None and _aten_shape(lambda: torch.constant_pad_nd(mk(4, 4), [-1, 0])) == [4, 3]


def test_glue_handlers_refuse_bad_shapes_before_any_launch(monkeypatch):
    """the handlers hand ATen-refused shapes back (NotImplemented) before they allocate or launch.  CPU tensors would not get that
    far (_ok wants CUDA), so stand-ins carry just the attributes the checks read: any allocation or launch would fail on them."""
    from spike2former_amd.ops import glue

    class Fake:
        is_cuda, dtype, device = True, torch.float32, torch.device("cuda", 0)

        def __init__(self, *shape):
            self.shape = torch.Size(shape)

        def numel(self):
            return int(np.prod(self.shape))

        def dim(self):
            return len(self.shape)

        def is_conj(self):
            return False

    is_tensor = torch.is_tensor
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, Fake) or is_tensor(t))
    assert glue.h_cat([Fake(2, 3), Fake(2, 4)], 0) is NotImplemented
    assert glue.h_cat([Fake(2, 3), Fake(4, 3)], 1) is NotImplemented
    assert glue.h_cat([Fake(2, 3), Fake(2, 3)], 2) is NotImplemented
    assert glue.h_cat_out([Fake(2, 3), Fake(2, 4)], 0, out=Fake(4, 3)) is NotImplemented
    assert glue.h_cat_out([Fake(2, 3), Fake(2, 3)], 0, out=Fake(5, 3)) is NotImplemented
    assert glue.h_stack([Fake(2, 3), Fake(3, 2)], 0) is NotImplemented
    assert glue.h_stack([Fake(2, 3), Fake(2, 3)], 3) is NotImplemented
    assert glue.h_constant_pad_nd(Fake(2, 3), [1, 1, 1, 1, 1, 1]) is NotImplemented
    assert glue.h_constant_pad_nd(Fake(2, 3), [1, 1, 1]) is NotImplemented
    assert glue.h_flip(Fake(2, 3), [0, 0]) is NotImplemented and glue.h_flip(Fake(2, 3), [2]) is NotImplemented
    assert glue.h_sum_dim(Fake(2, 3), [0, -2]) is NotImplemented and glue.h_sum_dim(Fake(2, 3), [2]) is NotImplemented
    assert glue.h_repeat(Fake(2, 3), [2]) is NotImplemented and glue.h_repeat(Fake(2, 3), [1, -1]) is NotImplemented


# the switches that are left after the settled A/B comparisons were retired (docs/EXPERIMENTS.md, "Retired switches")
_SWITCHES = ("KERNEL_EVENTS", "GRAD_SINKS", "WGRAD_STREAM", "BRANCH_STREAMS", "LONG_STREAMS", "LONG_WHAT", "SPIKES_BF16",
             "SPIKE_GEMM_TERMS", "SPIKE_GEMM_ENABLED", "SPIKE_GEMM_CHECK", "CONV3X3_IMPLICIT", "CONV3X3_IMPLICIT_MIN_PIXELS",
             "CONV3X3_DX_IMPLICIT", "DEFER_DW", "DW_PIPE", "BN_PARTIALS", "BN_PARTIALS_SINGLE", "DENSE_GROUPED", "RESPLIT_IN_GRAPH",
             "FANOUT_PORTS", "GLUE_MODE", "STRICT_GLUE", "STRICT", "GENERAL_RESIZE")
_RETIRED = ("PGEMM", "PGEMM_DX", "PGEMM_CONV", "PGEMM_MIN_N", "DEFER_DW_MAX_CONTRACTION", "CONV3X3_DX_MIN_PIXELS", "CONV3X3_DX_PIPE",
            "CONV_DW_DIRECT", "DW_PIPE_SINGLE", "DW_PIPE_CONV", "DWP_SCHEDULE", "DWP_WGS", "SPIKE_GEMM_DW", "MASK_EINSUM_DW_GROUPED",
            "MASK_EINSUM_DE_MFMA", "MASK_FWD_PGEMM", "MASK_BWD_FOLDED", "BN2_FUSED", "LINEAR_TM")


def test_config_fields_are_the_switches_that_are_left():
    from spike2former_amd.ops.config import Config
    assert tuple(Config.FIELDS) == _SWITCHES
    runtime = {"KERNEL_EVENTS", "GRAD_SINKS", "WGRAD_STREAM", "BRANCH_STREAMS", "LONG_STREAMS"}
    assert set(Config().snapshot()) == set(_SWITCHES) - runtime - {"STRICT", "STRICT_GLUE"}
    assert len(_RETIRED) == 19 and not set(_RETIRED) & set(Config.FIELDS)


def test_a_stale_switch_fails_loudly():
    from spike2former_amd import ops
    with pytest.raises(AttributeError, match="ops.cfg"):
        ops.PGEMM = False
    with pytest.raises(AttributeError):
        ops.cfg.DWP_SCHEDULE = 1
    with pytest.raises(AttributeError, match="ops.cfg"):
        ops.NO_SUCH_SWITCH = 1
    for name in _RETIRED + ("NO_SUCH_SWITCH",):
        assert name not in vars(ops) and not hasattr(ops.cfg, name)
        with pytest.raises(AttributeError):
            getattr(ops, name)
        with pytest.raises(AttributeError):
            setattr(ops, name, 1)
        with pytest.raises(AttributeError):
            setattr(ops.cfg, name, 1)
    strict, fallbacks = ops.STRICT, ops.FALLBACKS
    try:
        ops.STRICT = not strict                     # a switch: forwarded to ops.cfg
        assert ops.cfg.STRICT is (not strict) and "STRICT" not in vars(ops)
        ops.FALLBACKS = {}                          # an existing module attribute stays assignable
        assert ops.FALLBACKS == {}
    finally:
        ops.STRICT, ops.FALLBACKS = strict, fallbacks


def test_a_retired_environment_variable_changes_nothing():
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import json, sys; sys.path.insert(0, sys.argv[1]); from spike2former_amd.ops.config import Config; "
            "print('SNAPSHOT', json.dumps(Config().snapshot(), sort_keys=True))")
    retired = {"S2F_PGEMM": "0", "S2F_PGEMM_DX": "0", "S2F_PGEMM_CONV": "0", "S2F_DEFER_DW_MAX": "1", "S2F_CONV3_DX_PIPE": "2",
               "S2F_MASK_DW_GROUPED": "0", "S2F_MASK_FWD_PGEMM": "0", "S2F_MASK_BWD_FOLDED": "0", "S2F_DW_PIPE_SINGLE": "0",
               "S2F_DW_PIPE_CONV": "0", "S2F_DWP_SCHEDULE": "1", "S2F_DWP_WGS": "64", "S2F_BN2_FUSED": "0", "S2F_LINEAR_TM": "0",
               "S2F_CONV_DW_DIRECT": "1"}
    clean = {k: v for k, v in os.environ.items() if k not in retired}

    def snapshot(env):
        out = subprocess.run([sys.executable, "-c", code, root], env=env, check=True, capture_output=True, text=True).stdout
        return json.loads([l for l in out.splitlines() if l.startswith("SNAPSHOT ")][-1][len("SNAPSHOT "):])
    base = snapshot(clean)
    assert set(base) == set(_SWITCHES) - {"KERNEL_EVENTS", "GRAD_SINKS", "WGRAD_STREAM", "BRANCH_STREAMS", "LONG_STREAMS", "STRICT",
                                          "STRICT_GLUE"}
    assert snapshot(dict(clean, S2F_PGEMM="0")) == base
    assert snapshot(dict(clean, **retired)) == base
    assert snapshot(dict(clean, S2F_DW_PIPE="0")) == dict(base, DW_PIPE=False)          # a switch that stayed is still read


@pytest.mark.parametrize("keep_v", [False, True])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("spare", [False, True])
@pytest.mark.parametrize("skip", [False, True])
def test_output_collector_marks_exactly_the_outputs_without_a_gradient(keep_v, bf16, spare, skip):
    """ops.core._Outputs on a toy neuron: (spike triple, membrane, pass-through).  Exactly the handles, the fp32 spikes and the
    requested fp32 outputs are differentiable -- stand-ins and bf16 data are not, whichever of them the forward appended last (the
    context keeps only ONE call of mark_non_differentiable) -- and a gradient on every differentiable output reaches backward."""
    from spike2former_amd.ops.core import _Outputs, _grad_in, _grads, _spikes
    seen = []

    class Toy(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, factor, keep_v, bf16, spare, skip):
            ctx.factor = factor
            y = (x * factor).to(torch.bfloat16 if bf16 else torch.float32)
            return _Outputs(ctx, x).spikes(y, bf16, spare).grad(x + 1 if keep_v else None).through(x, skip).done()

        @staticmethod
        def backward(ctx, gy, gdata, gy2, gv, gskip):
            seen.append([g is not None for g in (gy, gdata, gy2, gv, gskip)])
            gx = sum(g * k for g, k in ((_grad_in(gy), ctx.factor), (_grad_in(gy2), ctx.factor), (gv, 1.0), (gskip, 1.0)) if g is not None)
            return _grads(ctx, gx)

    x = torch.arange(8.0).view(2, 4).requires_grad_()
    outs = Toy.apply(x * 1.0, 0.5, keep_v, bf16, spare, skip)
    want = [True, False, bf16 and spare, keep_v, skip]
    assert [o.requires_grad for o in outs] == want
    assert [o.grad_fn is not None for o in outs] == want
    assert [o.numel() == 0 for o in outs] == [False, not bf16, not (bf16 and spare), not keep_v, not skip]
    s = _spikes(*outs[:3])
    assert (s.data is outs[1] and s.tok is outs[0] and s.data.dtype == torch.bfloat16) if bf16 else (s.data is outs[0] and s.tok is None)
    assert s.tok2 is (outs[2] if bf16 and spare else None)
    assert torch.equal(s.data.float(), x.detach() * 0.5)
    sum((o * (i + 1)).sum() for i, (o, w) in enumerate(zip(outs, want)) if w).backward()
    assert seen == [want]          # no zero-filled gradient for an output nobody differentiated
    slope = 0.5 * (1 + 3 * (bf16 and spare)) + 4 * keep_v + 5 * skip
    assert torch.equal(x.grad, torch.full((2, 4), slope))


def test_bn_act_finds_up_lo_in_its_own_signature():
    """_BNAct's backward places the gradient of `up_lo` by the argument's position in forward, read from the signature"""
    import inspect
    from spike2former_amd.ops import bn
    names = list(inspect.signature(bn._BNAct.forward).parameters)
    assert names[0] == "ctx" and names[1 + bn._UP_LO] == "up_lo"
