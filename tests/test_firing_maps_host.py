"""CPU: the firing maps without a GPU -- the CPU implementations of ops.firing_map / ops.firing_draw against tests/firingmap_ref.py
(equality of integers and bytes: both sides are integer arithmetic, no tolerance exists), the argument errors of the two entry points
before any launch, the geometry rule, the default colour table, and FiringMaps' hooks on a stub model."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import firingmap_cases as K  # noqa: E402
import firingmap_ref as R  # noqa: E402

EINVAL, EALIGN = -1, -2


# ------------------------------------------------------------------------------------------------ 1. ops.firing_map on CPU tensors
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("P", K.MAP_P)
def test_cpu_firing_map_matches_the_restatement(P, bf16):
    from spike2former_amd import ops
    for ci, C in enumerate(K.MAP_C):
        for ti, (TB, B) in enumerate(K.MAP_TB_B):
            D = K.MAP_D[(ci + ti) % len(K.MAP_D)]
            off = (ci + ti) % 4
            x, host = K.spike_map(TB, C, P, D, seed=P * 100 + ci * 10 + ti, bf16=bf16)
            big, stats = K.sentinel_stats(B, P)
            got = ops.firing_map(K.at_offset(x, off), B, D, stats, assign=True)
            assert got is stats
            want = R.firing_map(host, B, D)
            assert np.array_equal(stats.numpy(), want), (C, TB, B, D)
            y, host2 = K.spike_map(TB, C, P, D, seed=7 + P + ci + ti, bf16=bf16)
            ops.firing_map(y, B, D, stats)          # accumulates; plane 2 is a running maximum
            want2 = R.firing_map(host2, B, D, stats=want)
            assert np.array_equal(stats.numpy(), want2)
            ops.firing_map(y, B, D, stats, assign=True)          # overwrites
            assert np.array_equal(stats.numpy(), R.firing_map(host2, B, D))
            b = big.numpy()
            assert (b[:3] == -123456789).all() and (b[3 + 4 * B * P:] == -123456789).all()


@pytest.mark.parametrize("D", K.MAP_D)
def test_every_special_value_lands_in_its_plane(D):
    """one pixel per value, one plane (T = B = C = 1): the planes by hand, then the restatement and the CPU op against them"""
    from spike2former_amd import ops
    sp = K.specials(D)          # -0.0, 0.3, -1/D, 65536/D, subnormal, NaN, inf, -inf, 65535/D
    levels = np.arange(D + 1, dtype=np.float32) / np.float32(D)
    x = np.concatenate([sp, levels]).astype(np.float32)[None, None]
    n_sp = len(sp)
    want = np.zeros((1, 4, x.shape[2]), np.int64)
    want[0, 1, 1:n_sp] = 1                      # everything but -0.0 is non-zero
    want[0, 3, 1:n_sp - 1] = 1                  # 0.3, -1/D, 65536/D, subnormal, NaN, +-inf: off the grid
    want[0, 0, n_sp - 1] = want[0, 2, n_sp - 1] = 65535
    want[0, 0, n_sp:] = want[0, 2, n_sp:] = np.arange(D + 1)
    want[0, 1, n_sp + 1:] = 1
    assert np.array_equal(R.firing_map(x, 1, D), want)
    stats = torch.zeros(1, 4, x.shape[2], dtype=torch.int32)
    ops.firing_map(torch.from_numpy(x), 1, D, stats, assign=True)
    assert np.array_equal(stats.numpy(), want)


def test_firing_map_argument_errors_before_any_launch():
    from spike2former_amd._lib import lib
    A = 1 << 20          # an aligned dummy address: never dereferenced on the host
    ok = dict(x=A, dtype=0, TB=4, B=2, C=3, P=16, D=8, stats=A, flags=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.s2f_firing_map(a["x"], a["dtype"], a["TB"], a["B"], a["C"], a["P"], a["D"], a["stats"], a["flags"], None)
    for bad in (dict(x=None), dict(stats=None), dict(TB=0), dict(B=0), dict(C=0), dict(TB=3), dict(P=-1), dict(D=0), dict(dtype=2),
                dict(dtype=-1), dict(flags=2), dict(flags=-1), dict(TB=2, B=2, C=32769), dict(TB=4, B=2, C=16385)):
        assert call(**bad) == EINVAL, bad
        assert b"s2f_firing_map" in lib.s2f_last_error()
    for bad in (dict(x=A + 2), dict(x=A + 1, dtype=1), dict(stats=A + 2)):
        assert call(**bad) == EALIGN, bad
    assert call(P=0) == 0          # launches nothing


def test_firing_draw_argument_errors_before_any_launch():
    from spike2former_amd._lib import lib
    A = 1 << 20
    ok = dict(image=A + 1, plane=A, h=2, w=3, full=5, lut=A + 3, a8=128, flags=0, H=7, W=13, out=A + 2, row=39)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.s2f_firing_draw(a["image"], a["plane"], a["h"], a["w"], a["full"], a["lut"], a["a8"], a["flags"], a["H"], a["W"],
                                   a["out"], a["row"], None)
    for bad in (dict(image=None), dict(plane=None), dict(lut=None), dict(out=None), dict(h=0), dict(w=0), dict(H=0), dict(W=-1),
                dict(a8=-1), dict(a8=257), dict(full=0), dict(full=-3), dict(flags=1), dict(flags=8), dict(row=38)):
        assert call(**bad) == EINVAL, bad
        assert b"s2f_firing_draw" in lib.s2f_last_error()
    assert call(plane=A + 2) == EALIGN


# ------------------------------------------------------------------------------------------------ 2. ops.firing_draw on CPU tensors
@pytest.mark.parametrize("hw,HW", K.DRAW_SIZES)
def test_cpu_firing_draw_matches_the_restatement(hw, HW):
    from spike2former_amd import ops
    from spike2former_amd.visualization import SegLocalVisualizer
    (h, w), (H, W) = hw, HW
    rng = np.random.default_rng(h * 31 + W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    plane = K.draw_plane(h, w, seed=H + w)
    top = int(plane.max())
    lut = SegLocalVisualizer.default_firing_lut()
    n = 0
    for a8 in K.DRAW_A8:
        for full in (1, top, 2 * top, max(1, top // 3)):
            for bgr in (False, True):
                off = 1 + n % 3
                n += 1
                big, out, _ = K.draw_window(H, W, off)
                got = ops.firing_draw(torch.from_numpy(img), torch.from_numpy(plane), full, torch.from_numpy(lut), a8 / 256, bgr=bgr,
                                      out=out)
                assert got is out
                want = R.firing_draw(img, plane, full, lut, a8, bgr)
                assert np.array_equal(big.numpy(), K.expect_window(H, W, off, want)), (a8, full, bgr)


def test_large_values_do_not_overflow():
    """plane values and `full` near 2^31 - 1: the restatement in Python integers of any size against the int64 one and the CPU op"""
    from spike2former_amd import ops
    top = 2 ** 31 - 1
    plane = np.array([[top, top - 1, 0], [top // 2, -top, top]], np.int32)
    H, W = 5, 9
    idx = R.firing_index(plane, top, H, W)
    s = np.maximum(plane.astype(object), 0)
    for Y in range(H):
        for X in range(W):
            ny, nx = max(0, (2 * Y + 1) * 2 - H), max(0, (2 * X + 1) * 3 - W)
            y0, x0 = ny // (2 * H), nx // (2 * W)
            fy, fx = (ny - y0 * 2 * H) * 256 // (2 * H), (nx - x0 * 2 * W) * 256 // (2 * W)
            y1, x1 = min(y0 + 1, 1), min(x0 + 1, 2)
            v = (256 - fy) * ((256 - fx) * s[y0, x0] + fx * s[y0, x1]) + fy * ((256 - fx) * s[y1, x0] + fx * s[y1, x1])
            assert idx[Y, X] == min(255, (255 * v + 32768 * top) // (65536 * top)), (Y, X)
    assert idx.max() == 255 and idx.min() == 0
    lut = np.stack([np.arange(256, dtype=np.uint8)] * 3, 1)
    img = np.zeros((H, W, 3), np.uint8)
    got = ops.firing_draw(torch.from_numpy(img), torch.from_numpy(plane), top, torch.from_numpy(lut), 1.0)
    assert np.array_equal(got.numpy()[:, :, 0], idx.astype(np.uint8))


def test_identity_resampling_and_the_blend_ends():
    from spike2former_amd import ops
    from spike2former_amd.visualization import SegLocalVisualizer
    # h = H, w = W: every weight is 0, idx = min(255, (255 s + full / 2) / full) with full / 2 rounded down by the common factor
    rng = np.random.default_rng(1)
    plane = rng.integers(0, 900, (6, 11)).astype(np.int32)
    for full in (1, 7, 500, 899, 2000):
        want = np.minimum(255, (2 * 255 * plane.astype(np.int64) + full) // (2 * full))
        assert np.array_equal(R.firing_index(plane, full, 6, 11), want), full
    # a ramp 0 .. 255 with full = 255 hits every row of the table once
    ramp = np.arange(256, dtype=np.int32).reshape(16, 16)
    assert np.array_equal(R.firing_index(ramp, 255, 16, 16).reshape(-1), np.arange(256))
    lut = SegLocalVisualizer.default_firing_lut()
    img = rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)
    t = torch.from_numpy
    # a8 = 0 returns the picture (RGB; swapped with bgr), a8 = 256 the table colour
    assert np.array_equal(ops.firing_draw(t(img), t(ramp), 255, t(lut), 0.0).numpy(), img)
    assert np.array_equal(ops.firing_draw(t(img), t(ramp), 255, t(lut), 0.0, bgr=True).numpy(), img[:, :, ::-1])
    assert np.array_equal(ops.firing_draw(t(img), t(ramp), 255, t(lut), 1.0).numpy(), lut.reshape(16, 16, 3))
    # alpha -> a8 = floor(alpha 256 + 0.5)
    assert np.array_equal(ops.firing_draw(t(img), t(ramp), 255, t(lut), 0.8).numpy(), R.firing_draw(img, ramp, 255, lut, 205))


def test_default_table():
    from spike2former_amd.visualization import SegLocalVisualizer
    lut = SegLocalVisualizer.default_firing_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256, 3)
    assert tuple(lut[0]) == (0, 0, 128) and tuple(lut[255]) == (128, 0, 0)
    for ch in range(3):          # piecewise monotone: up to a plateau of 255, then down -- the sign of the steps changes at most once
        d = np.diff(lut[:, ch].astype(int))
        signs = np.sign(d[d != 0])
        assert (np.diff(signs) != 0).sum() <= 1 and lut[:, ch].max() == 255, ch
    assert len({tuple(r) for r in lut}) == 256          # every level has a colour of its own


# ------------------------------------------------------------------------------------------------ 3. the geometry rule
def test_geometry_rule():
    from spike2former_amd.firingmaps import map_geometry
    T, B, H, W = 2, 3, 64, 96
    for shape in ((2, 3, 5, 16, 24), (6, 5, 16, 24), (2, 3, 5, 384), (6, 5, 384)):
        assert map_geometry(shape, T, B, H, W) == (5, 16, 24, 4), shape
    assert map_geometry((2, 3, 7, 64, 96), T, B, H, W) == (7, 64, 96, 1)
    assert map_geometry((6, 7, 6), T, B, H, W) == (7, 2, 3, 32)
    # B = 1
    for shape in ((2, 1, 5, 8, 12), (2, 5, 8, 12), (2, 1, 5, 96), (2, 5, 96)):
        assert map_geometry(shape, 2, 1, H, W) == (5, 8, 12, 8), shape
    # no reading fits: an N with no stride, a stride that is no power of two or differs by axis, other leading dimensions, ranks
    for shape in ((6, 5, 100), (2, 3, 5, 100), (6, 5, 16, 32), (2, 3, 5, 32, 24), (5, 5, 16, 24), (3, 2, 5, 16, 24), (6, 5, 383)):
        assert isinstance(map_geometry(shape, T, B, H, W), str), shape
    assert "no power-of-two stride" in map_geometry((6, 5, 100), T, B, H, W)
    assert map_geometry((6, 5, 64 * 96 // 9), T, B, H, W).startswith("no ")          # s = 3
    assert map_geometry((2, 3), T, B, H, W).startswith("rank 2") and map_geometry((1,) * 6, T, B, H, W).startswith("rank 6")
    # two readings that fit are not guessed between
    assert map_geometry((2, 1, 4, 16), 2, 1, 4, 16).startswith("ambiguous")


def _stub_model(outputs, T=2):
    """a model whose backbone holds one Q_IFNode per entry of `outputs` (name -> tensor or callable(x)) and calls each once"""
    from spike2former_amd.neuron import Q_IFNode

    class Node(Q_IFNode):
        def forward(self, x):
            return self.out(x) if callable(self.out) else self.out

    class Backbone(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.T = T
            for name, out in outputs.items():
                node = Node()
                node.out = out
                parts = name.split(".")
                holder = self
                for p in parts[:-1]:
                    if not hasattr(holder, p):
                        setattr(holder, p, torch.nn.Module())
                    holder = getattr(holder, p)
                setattr(holder, parts[-1], node)

        def forward(self, x):
            for m in self.modules():
                if isinstance(m, Node):
                    m(x)
            return x

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.backbone = Backbone()

        def forward(self, x):
            return self.backbone(x)
    return Model()


def _hook_counts(model):
    return sum(len(m._forward_hooks) + len(m._forward_pre_hooks) for m in model.modules())


def test_firing_maps_on_a_stub_model():
    import spike2former_amd as s2f
    T, B, H, W, D = 2, 2, 8, 12, 8
    x1, h1 = K.spike_map(T * B, 5, 4 * 6, D, seed=1, special=False)
    x2, h2 = K.spike_map(T * B, 3, 8 * 12, D, seed=2, special=False)
    outputs = {"stage.a": x1.view(T, B, 5, 4, 6), "stage.b": x2.view(T * B, 3, 96), "stage.odd": torch.zeros(T * B, 3, 50),
               "stage.strided": torch.zeros(T, B, 5, 4, 12)[..., ::2], "transformer_decoder.q": torch.zeros(T, B, 6, 24),
               "stage.rank2": torch.zeros(4, 4)}
    model = _stub_model(outputs, T)
    assert _hook_counts(model) == 0
    pic = torch.zeros(B, 3, H, W)
    with s2f.FiringMaps(model) as maps:
        assert maps.attached and _hook_counts(model) == len(outputs) + 1
        model(pic)
        model(pic)
        read = maps.read()
    assert not maps.attached and _hook_counts(model) == 0
    assert read.names == ["backbone.stage.a", "backbone.stage.b"]
    assert set(maps.skipped) == {"backbone.stage.odd", "backbone.stage.strided", "backbone.transformer_decoder.q", "backbone.stage.rank2"}
    assert maps.skipped["backbone.transformer_decoder.q"].startswith("token-major")
    assert maps.skipped["backbone.stage.strided"] == "not contiguous" and maps.skipped["backbone.stage.rank2"].startswith("rank 2")
    assert read.meta["backbone.stage.a"] == (T, 5, D, 2) and read.meta["backbone.stage.b"] == (T, 3, D, 2)
    once = R.firing_map(h1, B, D)
    want = R.firing_map(h1, B, D, stats=once)
    got = read.planes["backbone.stage.a"]
    assert got.dtype == np.int32 and got.shape == (B, 4, 4, 6) and np.array_equal(got.reshape(B, 4, 24), want)
    assert read.planes["backbone.stage.b"].shape == (B, 4, 8, 12)
    assert np.array_equal(read.rate("backbone.stage.a"), want[:, 0].reshape(B, 4, 6) / (T * 5 * D * 2))
    assert np.array_equal(read.active("backbone.stage.a"), want[:, 1].reshape(B, 4, 6) / (T * 5 * 2))
    assert read.off_grid("backbone.stage.a") == 0 and read.rate("backbone.stage.a").max() <= 1.0
    summary = read.summary()
    assert list(summary) == read.names and set(summary["backbone.stage.b"]) == {"mean", "max", "silent", "shape"}
    # detach() / attach() by hand, a regex and a predicate, clear(), and another input size clearing the maps
    maps = s2f.FiringMaps(model, layers=r"stage\.(a|b)$")
    assert list(maps.nodes) == ["backbone.stage.a", "backbone.stage.b"] and _hook_counts(model) == 0
    assert list(s2f.FiringMaps(model, layers=lambda n: n.endswith(".b")).nodes) == ["backbone.stage.b"]
    maps.attach()
    assert _hook_counts(model) == 3
    model(pic)
    assert maps.passes == {"backbone.stage.a": 1, "backbone.stage.b": 1}
    maps.clear()
    assert not maps.passes and maps.read().names == []
    model(pic)
    model(torch.zeros(1, 3, H, W))          # another batch: both outputs no longer fit -> cleared, then skipped
    assert not maps.passes and set(maps.skipped) == {"backbone.stage.a", "backbone.stage.b"}
    maps.detach()
    assert _hook_counts(model) == 0
    model(pic)
    assert not maps.passes
    with pytest.raises(ValueError):
        s2f.FiringMaps(model, layers="nothing_matches")


def test_a_prefired_call_shown_twice_counts_once():
    """fused.py shows a neuron that a producer kernel applied to the hooks from its own site, and the consumer's module call shows the
    pre-fired spikes again on the same unchanged input: one pass; a call on another tensor, or on the same one changed, is another"""
    import spike2former_amd as s2f
    x, host = K.spike_map(2, 3, 16, 8, seed=4, special=False)
    model = _stub_model({"a": x.view(2, 1, 3, 4, 4)})
    node = model.backbone.a
    with s2f.FiringMaps(model) as maps:
        pic = torch.zeros(1, 3, 4, 4)
        u = torch.zeros(5)
        model.backbone._forward_pre_hooks[next(iter(model.backbone._forward_pre_hooks))](model.backbone, (pic,))
        for hook in list(node._forward_hooks.values()):          # the producer's site
            hook(node, (u,), node.out)
        node(u.view(5))                                          # the consumer's module call: an echo
        assert maps.passes == {"backbone.a": 1}
        node(u)                                                  # a call of its own
        u.add_(1)
        node(u)                                                  # the same tensor, changed
        node(torch.zeros(5))
        assert maps.passes == {"backbone.a": 4}
        assert np.array_equal(maps.read().planes["backbone.a"].reshape(1, 4, 16), 4 * R.firing_map(host, 1, 8) // [[[1], [1], [4], [1]]])


def test_passes_bound_is_raised_on_the_host():
    """T C 65535 passes must stay below 2^31: 16384 planes admit two passes, the third raises before its launch"""
    import spike2former_amd as s2f
    from spike2former_amd import ops
    assert ops.firing_map_sum_ok(32768) and not ops.firing_map_sum_ok(32769) and not ops.firing_map_sum_ok(16384, 3)
    model = _stub_model({"a": torch.zeros(1, 1, 16384, 2, 2)}, T=1)
    with s2f.FiringMaps(model) as maps:
        model(torch.zeros(1, 3, 2, 2))
        model(torch.zeros(1, 3, 2, 2))
        with pytest.raises(OverflowError):
            model(torch.zeros(1, 3, 2, 2))
        assert maps.passes == {"backbone.a": 2}
    with pytest.raises(ValueError):
        ops.firing_map(torch.zeros(1, 32769, 1), 1, 8, torch.zeros(1, 4, 1, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ 4. drawing on the host, registry
def test_draw_firing_on_cpu_tensors(tmp_path, monkeypatch):
    import spike2former_amd as s2f
    from PIL import Image
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # (the CPU implementation on any machine)
    T, B, D = 2, 2, 8
    rng = np.random.default_rng(3)
    planes, meta = {}, {}
    for i, (n, (h, w), C) in enumerate((("a", (4, 6), 5), ("b", (8, 12), 3), ("c", (2, 3), 7))):
        x, host = K.spike_map(T * B, C, h * w, D, seed=i, special=False)
        planes[n] = R.firing_map(host, B, D).astype(np.int32).reshape(B, 4, h, w)
        meta[n] = (T, C, D, 1)
    read = s2f.FiringMapRead(list(planes), planes, meta)
    pic = rng.integers(0, 256, (16, 24, 3), dtype=np.uint8)
    vis = s2f.SegLocalVisualizer(save_dir=str(tmp_path))
    lut = vis.default_firing_lut()
    panel = vis.draw_firing(pic, read, image=1, name="x", step=3).numpy()
    assert panel.shape == (2 * 16, 2 * 24, 3)
    for i, n in enumerate("abc"):
        r, c = divmod(i, 2)
        want = R.firing_draw(pic, planes[n][1, 0], max(1, int(planes[n][1, 0].max())), lut, 128)
        assert np.array_equal(panel[r * 16:(r + 1) * 16, c * 24:(c + 1) * 24], want), n
    assert (panel[16:, 24:] == 0).all()          # the unused tile is black
    assert np.array_equal(np.asarray(Image.open(tmp_path / "vis_image" / "x_3.png")), panel)
    # one absolute rate for all tiles, plane 1, a chosen arrangement and subset, BGR, a file of its own
    out = tmp_path / "own.png"
    panel = vis.draw_firing(pic, read, image=0, names=["c", "a"], which="active", arrangement=(1, 3), alpha=0.25, vmax=0.5,
                            image_is_bgr=True, out_file=str(out)).numpy()
    assert panel.shape == (16, 3 * 24, 3) and out.exists()
    for i, n in enumerate("ca"):
        full = max(1, int(np.floor(0.5 * T * meta[n][1] + 0.5)))
        want = R.firing_draw(pic, planes[n][0, 1], full, lut, 64, bgr=True)
        assert np.array_equal(panel[:, i * 24:(i + 1) * 24], want), n
    assert vis.firing_full(read, "a", 0, "rate", 0.5) == (0, T * 5 * D // 2)
    with pytest.raises(ValueError):
        vis.draw_firing(pic, read, arrangement=(1, 2))
    with pytest.raises(KeyError):
        vis.draw_firing(pic, read, names=["nope"])


def test_registry_and_exports():
    import spike2former_amd as s2f
    from spike2former_amd import ops
    assert s2f.HOOKS.get("FiringMapHook") is s2f.FiringMapHook and s2f.VISUALIZERS.get("SegLocalVisualizer") is s2f.SegLocalVisualizer
    model = _stub_model({"a": torch.zeros(2, 1, 1, 2, 2)})
    hook = s2f.HOOKS.build(dict(type="FiringMapHook", maps=s2f.FiringMaps(model), interval=2))
    assert isinstance(hook, s2f.FiringMapHook) and not hook.maps.attached
    assert s2f.FiringMapHook(s2f.FiringMaps(model), interval=1).maps.attached          # the first batch is due
    assert ops.FIRING_MAP_ASSIGN == 1 and callable(ops.firing_map) and callable(ops.firing_draw)
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s2f.h")).read()
    assert int(re.search(r"^#define S2F_FIRING_MAP_ASSIGN[ \t]+(\d+)", src, flags=re.M).group(1)) == ops.FIRING_MAP_ASSIGN
    assert int(re.search(r"#define S2F_ABI_VERSION (\d+)", src).group(1)) >= 55
