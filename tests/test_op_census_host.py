"""CPU: the operand census without a GPU -- the torch route of ops.operand_census against the numpy restatement tests/census_ref.py
in exact integers, the MAC formulas against an independent count from forward hooks on torch.nn layers, the report arithmetic of
EnergyReport on a hand-written table, the row keys OpCensus derives from weight addresses, and the argument errors of
s2f_operand_census (before any launch, so no GPU is needed)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import census_ref as R  # noqa: E402


def special_values(D):
    """levels 0 .. D, counts above D (alpha * spikes: 4.0 at D = 8 is level 32), the last level on the grid and the first beyond it,
    and everything that is off the grid or not a number"""
    on = [k / D for k in range(D + 1)] + [4.0, 32.0 / D, 65535.0 / D, -0.0]
    off = [65536.0 / D, -1.0 / D, -2.0, 0.3, 1e-40, -1e-42, float("inf"), float("-inf"), float("nan"), 3e38]
    return on + off


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [8, 1, 4, 3, 10])
def test_cpu_route_equals_the_restatement(dtype, D):
    from spike2former_amd import ops
    g = torch.Generator().manual_seed(D)
    vals = torch.tensor(special_values(D), dtype=torch.float32)
    rnd = torch.randint(0, 4 * D, (301,), generator=g).float() / D
    rnd[::17] += 0.01
    x = torch.cat([vals, rnd]).to(dtype)
    row = torch.zeros(8, dtype=torch.int64)
    assert ops.operand_census(x, row, D) is row
    want = R.census(x.float().numpy(), D)
    assert row.tolist() == want.tolist()
    assert row[R.ELEMENTS] == x.numel() and row[R.CALLS] == 1 and row[R.RESERVED] == 0
    if dtype == torch.float32 and D == 8:
        # by hand: 0/8 .. 8/8, 4.0 (32), 32/8 (32), 65535/8, -0.0 on the grid; ten special values and every 17th random one off it
        sp = R.census(vals.numpy(), 8)
        assert sp[R.LEVEL_SUM] == sum(range(9)) + 32 + 32 + 65535 and sp[R.MAX_LEVEL] == 65535
        assert sp[R.OFF_GRID] == 10 and sp[R.NONFINITE] == 3 and sp[R.NONZERO] == len(vals) - 2          # (0/8 and -0.0)
    # a second call into the same row adds; the maximum stays a maximum
    ops.operand_census(x[:5], row, D)
    want = R.census(x[:5].float().numpy(), D, want)
    assert row.tolist() == want.tolist() and row[R.CALLS] == 2


def test_cpu_route_edges():
    from spike2former_amd import ops
    row = torch.zeros(2, 8, dtype=torch.int64)
    ops.operand_census(torch.zeros(0), row[0], 8)                                   # n == 0: one call and nothing else
    assert row[0].tolist() == [0, 0, 0, 0, 0, 0, 1, 0] and row[1].tolist() == [0] * 8
    y = torch.full((4, 6), 0.5, dtype=torch.bfloat16)
    ops.operand_census(ops.Spikes(y), row[1], 8)                                    # a Spikes: its stored data
    assert row[1].tolist() == [24, 96, 24, 0, 4, 0, 1, 0]
    ops.operand_census(torch.full((3, 5), 0.25).t(), row[1], 8)                     # a non-contiguous operand
    assert row[1].tolist() == [39, 126, 39, 0, 4, 0, 2, 0]
    one_third = torch.tensor([1.0 / 3.0])                                           # the rule for D that is no power of two
    r = torch.zeros(8, dtype=torch.int64)
    assert ops.operand_census(one_third, r, 3).tolist() == [1, 1, 1, 0, 1, 0, 1, 0]
    with pytest.raises(TypeError):
        ops.operand_census(torch.zeros(3, dtype=torch.float64), r, 8)
    with pytest.raises(ValueError):
        ops.operand_census(torch.zeros(3), r, 0)
    with pytest.raises(ValueError):
        ops.operand_census(torch.zeros(3), torch.zeros(7, dtype=torch.int64), 8)
    strict, before = ops.STRICT, dict(ops.FALLBACKS)
    ops.STRICT = True                                                               # the CPU route is no fall-back site
    try:
        ops.operand_census(torch.ones(3), r, 8)
    finally:
        ops.STRICT = strict
    assert dict(ops.FALLBACKS) == before


def test_argument_errors_are_reported_without_a_gpu():
    from spike2former_amd import _lib
    lib = _lib.lib
    assert lib.s2f_version() >= 49 and len(_lib.SIGNATURES["s2f_operand_census"][1]) == 6
    call = lib.s2f_operand_census
    P = 1 << 20          # an aligned dummy address: never dereferenced on the host, and every call below returns before a launch
    for args, word in (((None, 0, 4, 8, P, None), b"null"), ((P, 0, 4, 8, None, None), b"null"), ((P, 0, -1, 8, P, None), b"below 0"),
                       ((P, 0, 4, 0, P, None), b"below 1"), ((P, 1, 4, -3, P, None), b"below 1"), ((P, 2, 4, 8, P, None), b"dtype"),
                       ((P, -1, 4, 8, P, None), b"dtype")):
        assert call(*args) == -1, args
        assert word in lib.s2f_last_error(), (args, lib.s2f_last_error())
    assert call(P + 2, 0, 4, 8, P, None) == -2 and call(P + 1, 1, 4, 8, P, None) == -2 and call(P, 0, 4, 8, P + 4, None) == -2


# ---------------------------------------------------------------------------------------------------- MAC formulas
def hooked_macs(layer, x):
    """output elements x fan-in, read off the layer and its output by a forward hook"""
    seen = []

    def hook(m, inp, out):
        fan_in = m.in_features if isinstance(m, torch.nn.Linear) else (m.in_channels // m.groups) * int(np.prod(m.kernel_size))
        seen.append(out.numel() * fan_in)
    h = layer.register_forward_hook(hook)
    with torch.no_grad():
        layer(x)
    h.remove()
    return seen[0]


class Recorder:
    """stands in for a live census at ops/core.py `_TAP`: keeps what the taps report.  The ops are then called on CPU tensors: every
    tap reports before its op refuses a host tensor (no launch), so the arithmetic under test is the taps' own."""

    def __init__(self):
        self.seen = []

    def __call__(self, kind, weight, macs, operands):
        self.seen.append((kind, macs, [o[0] for o in operands]))

    def __enter__(self):
        from spike2former_amd import ops
        assert ops.core._TAP[0] is None
        ops.core._TAP[0] = self
        return self

    def __exit__(self, *exc):
        from spike2former_amd import ops
        ops.core._TAP[0] = None
        return False

    def run(self, fn, *args, **kwargs):
        """-> [(kind, macs, operand names)] the call reported; a host tensor is refused behind the tap"""
        self.seen = []
        try:
            fn(*args, **kwargs)
        except (RuntimeError, RuntimeWarning):
            pass
        return self.seen


def ones_macs(*products):
    """an independent count: a product of all-ones matrices sums to its number of multiply-accumulates"""
    return [int(p.sum().item()) for p in products]


@pytest.mark.parametrize("cin,cout,k,stride,pad,groups", [
    (6, 10, 3, 1, 1, 1),          # dense
    (6, 10, 7, 2, 3, 1),          # strided, padded (the stem)
    (8, 12, 3, 2, 1, 4),          # grouped
    (8, 8, 5, 1, 2, 8),           # depthwise
    (8, 8, 3, 1, 0, 8),           # depthwise, no padding
    (6, 10, 1, 1, 0, 1),          # 1x1
    (5, 7, 3, 3, 2, 1),           # stride 3 on an odd map
])
def test_conv_taps_against_hook_count(cin, cout, k, stride, pad, groups):
    from spike2former_amd import ops
    x = torch.zeros(2, cin, 13, 11)
    conv = torch.nn.Conv2d(cin, cout, k, stride, pad, groups=groups, bias=False)
    want = hooked_macs(conv, x)
    assert ops.conv_macs(2, cin, 13, 11, cout, k, k, stride, pad, groups) == want
    with Recorder() as tap, torch.no_grad():
        assert tap.run(ops.conv_dense, x, conv.weight, None, stride, pad, False) == [("conv", want, ["x"])]          # (groups from the weight's shape)
        if groups == cin == cout and stride == 1:
            assert tap.run(ops.dwconv, x, conv.weight, pad) == [("dwconv", want, ["x"])]
        if k == 1:
            x3, w2d = x.flatten(2), conv.weight.view(cout, cin)
            assert tap.run(ops.spike_gemm, x3, w2d) == [("gemm", want, ["x"])]
            assert tap.run(ops.dense_gemm, x3, w2d) == [("gemm", want, ["x"])]
        if k == 3 and stride == 1 and pad == 1 and groups == 1:
            assert ops.conv_macs(2, cin, 13, 11, cout, 3, 3, 1, 1) == want          # what conv3x3_bn_lif_eval's tap calls


def test_linear_and_grouped_taps_against_hook_count():
    from spike2former_amd import ops
    x = torch.zeros(3, 5, 12)
    lin = torch.nn.Linear(12, 7)
    c1 = torch.nn.Conv1d(6, 10, 1, bias=False)
    grouped = torch.nn.Conv1d(3 * 6, 3 * 10, 1, groups=3, bias=False)
    xg = torch.zeros(4, 18, 9)
    with Recorder() as tap, torch.no_grad():
        assert tap.run(ops.linear_tm, x, lin.weight, lin.bias) == [("linear", hooked_macs(lin, x), ["x"])]
        assert tap.run(ops.spike_gemm, xg[:, :6], c1.weight.view(10, 6)) == [("gemm", hooked_macs(c1, xg[:, :6]), ["x"])]
        # three weights on the three channel groups of one map (the attention twins' second 1x1): one report each, a third of the whole
        got = tap.run(ops.dense_gemm, xg, list(grouped.weight.view(3, 10, 6).unbind(0)))
        assert got == [("gemm", hooked_macs(grouped, xg) // 3, ["x"])] * 3
        a, b = torch.ones(2, 5, 7), torch.ones(2, 7, 3)
        assert tap.run(ops.bmm_small, a, b) == [("bmm", ones_macs(a @ b)[0], ["a", "b"])]


def test_attention_taps_against_an_independent_count():
    """the two associations: q (k^T v) without a mask (csrc/sdsa.hip), (q k^T) v with one (csrc/sdsa_masked.hip)"""
    from spike2former_amd import ops
    TB, heads, d, Nq, Nk = 2, 4, 8, 20, 12
    q, k, v = torch.ones(TB, heads * d, Nq), torch.ones(TB, heads * d, Nk), torch.ones(TB, heads * d, Nk)
    qh, kh, vh = (t.view(TB, heads, d, -1) for t in (q, k, v))          # [TB, heads, d, N]
    kv = kh @ vh.transpose(2, 3)                                        # [TB, heads, d, d], contracted over N_k
    want_kv, want_qkv = ones_macs(kv, qh.transpose(2, 3) @ torch.ones_like(kv))
    scores = qh.transpose(2, 3) @ kh                                    # [TB, heads, Nq, Nk], contracted over d
    want_qk, want_av = ones_macs(scores, torch.ones_like(scores) @ vh.transpose(2, 3))
    assert want_kv != want_qkv and want_qk == want_av == TB * heads * Nq * Nk * d
    with Recorder() as tap, torch.no_grad():
        assert tap.run(ops.sdsa, q, k, v, heads, 1.0) == [("sdsa:kv", want_kv, ["k", "v"]), ("sdsa:q_kv", want_qkv, ["q"])]
        packed = torch.ones(TB, 3 * heads * d, Nk)
        kv_p, qkv_p = ones_macs(kv, vh.transpose(2, 3) @ torch.ones_like(kv))          # (N_q = N_k in the packed form)
        assert tap.run(ops.sdsa_packed, packed, heads, 1.0) == [("sdsa:kv", kv_p, ["k", "v"]), ("sdsa:q_kv", qkv_p, ["q"])]
        mask = torch.zeros(1, heads, Nq, Nk, dtype=torch.bool)
        assert tap.run(ops.sdsa_masked, q, k, v, mask, heads, 1.0, 1) == [("sdsa_masked:qk", want_qk, ["q", "k"]),
                                                                           ("sdsa_masked:av", want_av, ["v"])]


def test_dcnv3_and_contraction_taps_against_an_independent_count():
    import torch.nn.functional as F
    from spike2former_amd import ops
    N, H, W, G, Cg, kh, kw = 2, 5, 6, 4, 3, 3, 3
    K = kh * kw
    x = torch.ones(N, H, W, G * Cg)
    offset, mask = torch.zeros(N, H, W, G * K * 2), torch.ones(N, H, W, G * K)
    # the core as the reference evaluates it: per (image, group) one bilinear grid_sample of the Cg-channel map at H W K points -- four
    # taps per sampled value -- then one product with the mask per sampled value
    sampled = F.grid_sample(torch.ones(N * G, Cg, H, W), torch.zeros(N * G, H * W, K, 2), mode="bilinear", align_corners=False)
    want_sample, want_mod = 4 * sampled.numel(), (sampled * mask.view(N, H * W, G, K).permute(0, 2, 1, 3).reshape(N * G, 1, H * W, K)).numel()
    with Recorder() as tap, torch.no_grad():
        geo = (kh, kw, 1, 1, 1, 1, 1, 1, G, Cg, 1.0)
        for core in (ops.dcnv3_core, ops.dcnv3_core_cm):
            assert tap.run(core, x, offset, mask, *geo) == [("dcnv3:sample", want_sample, ["x"]), ("dcnv3:modulate", want_mod, ["mask"])]
        T, B, Q, C, HW, Kc = 2, 3, 5, 8, 12, 4
        e, mf = torch.ones(T, B, Q, C), torch.ones(T, B, C, HW)
        want = ones_macs(torch.einsum("tbqc,tbcp->bqp", e, mf))[0]
        assert tap.run(ops.mask_einsum, e, mf, 0.5) == [("mask_einsum", want, ["e", "mask_features"])]
        cls, probs = torch.ones(B, Q, Kc), torch.ones(B, Q, 3, 4)
        want = ones_macs(torch.einsum("bqc,bqhw->bchw", cls, probs))[0]
        assert tap.run(ops.class_mask_product, cls, probs) == [("class_mask_product", want, ["cls_score", "mask_probs"])]


# ---------------------------------------------------------------------------------------------------- report arithmetic
def operand(name, elements, level_sum, off_grid, spikes=False, max_level=8):
    return dict(name=name, spikes=spikes, elements=elements, level_sum=level_sum, nonzero=min(elements, level_sum), off_grid=off_grid,
                max_level=max_level, nonfinite=0)


TABLE = [
    dict(key="backbone.stage1.0.pwconv1.weight", kind="gemm", calls=2, macs=1000, operands=[operand("x", 200, 50, 0, True)]),
    dict(key="backbone.stage1.0.pwconv2.weight", kind="gemm", calls=2, macs=2000, operands=[operand("x", 400, 10, 7)]),
    dict(key="backbone.stage2.0.attn:sdsa:kv", kind="sdsa:kv", calls=2, macs=400,
         operands=[operand("k", 100, 50, 0, True), operand("v", 100, 20, 0, True)]),
    dict(key="decode_head.pixel_decoder.x:dcnv3:modulate", kind="dcnv3:modulate", calls=2, macs=300, operands=[operand("mask", 64, 0, 0, True)]),
    dict(key="decode_head.cls_embed.weight", kind="linear", calls=2, macs=500, operands=[operand("x", 10, 80, 0, max_level=32)]),
    dict(key="decode_head:mask_einsum", kind="mask_einsum", calls=2, macs=800,
         operands=[operand("e", 50, 100, 0), operand("mask_features", 80, 3, 80)]),
    dict(key="decode_head.bad.weight", kind="gemm", calls=2, macs=100, operands=[operand("x", 10, 5, 2, True)]),
]


def test_report_arithmetic_on_a_hand_written_table(tmp_path):
    from spike2former_amd import EnergyReport
    e_mac, e_ac = 4.6e-12, 0.9e-12
    rep = EnergyReport(TABLE, params=1234, passes=2, e_mac=e_mac, e_ac=e_ac)
    want_rows, want_totals = R.report(TABLE, e_mac, e_ac)
    for r, w in zip(rep.rows, want_rows):
        assert (r["klass"], r["rate"], r["sops"], r["energy_J"]) == (w["klass"], w["rate"], w["sops"], w["energy_J"]), r["key"]
    # by hand: the classes, min(rate) over two on-grid operands, an on-grid operand beside a real one, a silent operand
    assert [r["klass"] for r in rep.rows] == ["ac", "real", "ac", "ac", "ac", "ac", "real"]
    assert rep.rows[0]["rate"] == 0.25 and rep.rows[0]["sops"] == 250.0
    assert rep.rows[1]["rate"] is None and rep.rows[1]["off_share"] == 7 / 400 and rep.rows[1]["energy_J"] == e_mac * 2000
    assert rep.rows[2]["rate"] == 0.2 and rep.rows[2]["sops"] == 80.0          # min(50 / 100, 20 / 100)
    assert rep.rows[3]["sops"] == 0.0 and rep.rows[3]["energy_J"] == 0.0
    assert rep.rows[4]["rate"] == 8.0 and rep.rows[4]["sops"] == 4000.0        # alpha * spikes: more than one accumulate per element
    assert rep.rows[5]["rate"] == 2.0 and rep.rows[5]["off_share"] == 80 / 130
    sops = 250.0 + 80.0 + 0.0 + 4000.0 + 1600.0
    assert rep.totals == dict(params=1234, macs=5100, real_macs=2100, sops=sops, energy_mJ=1e3 * sum(r["energy_J"] for r in rep.rows),
                              passes=2)
    assert rep.totals["energy_mJ"] == pytest.approx(1e3 * (e_mac * 2100 + e_ac * sops), rel=1e-12)
    for k in ("macs", "real_macs", "sops"):
        assert rep.totals[k] == want_totals[k]
    assert rep.totals["energy_mJ"] == pytest.approx(want_totals["energy_mJ"], rel=1e-12)
    # the invariant check: only the row whose operand came as Spikes and is off the grid
    assert [r["key"] for r in rep.spikes_off_grid()] == ["decode_head.bad.weight"]
    # by_stage: the first two components of the key's module path
    st = rep.by_stage()
    assert list(st) == ["backbone.stage1", "backbone.stage2", "decode_head.pixel_decoder", "decode_head.cls_embed", "decode_head",
                        "decode_head.bad"]
    assert st["backbone.stage1"] == dict(rows=2, macs=3000, real_macs=2000, sops=250.0, energy_J=e_ac * 250.0 + e_mac * 2000)
    assert sum(s["macs"] for s in st.values()) == rep.totals["macs"]
    # JSON and CSV round trips
    again = EnergyReport.from_json(rep.to_json())
    assert again.rows == rep.rows and again.totals == rep.totals
    assert json.loads(rep.to_json())["totals"]["real_macs"] == 2100
    path = tmp_path / "energy.csv"
    rep.to_csv(path)
    lines = open(path).read().splitlines()
    assert len(lines) == 1 + len(TABLE) and lines[0].startswith("key,kind,klass,calls,macs,rate,sops")
    assert EnergyReport.rows_from_csv(path) == rep.rows
    # the table: one line per row, the totals line with params, MACs, real MACs, SOPs and mJ, the note on what is not counted
    text = str(rep).splitlines()
    assert len(text) == 1 + len(TABLE) + 2
    for word in ("params", "MACs", "real MACs", "SOPs", "mJ", "passes 2"):
        assert word in text[-2], (word, text[-2])
    assert "not counted" in text[-1] and "BatchNorm" in text[-1]
    assert len({len(line) for line in text[:1 + len(TABLE)]}) == 1          # fixed width
    # other prices are arguments
    assert EnergyReport(TABLE, e_mac=1.0, e_ac=0.0).totals["energy_mJ"] == 1e3 * 2100


# ---------------------------------------------------------------------------------------------------- OpCensus: keys, passes, switches
class Toy(torch.nn.Module):
    """two sibling weights laid out back to back (as the attention twins are), a lone one, and forwards that report what a real
    op's tap would"""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Conv1d(4, 6, 1, bias=False)
        self.b = torch.nn.Conv1d(4, 6, 1, bias=False)
        self.c = torch.nn.Linear(6, 3)
        self.inner = torch.nn.Identity()
        from spike2former_amd import ops
        ops.flatten_together([self.a.weight, self.b.weight])

    def forward(self, x):
        from spike2former_amd import ops
        tap = ops.core._TAP[0]
        self.inner(x)
        if tap is not None:
            both = ops.cat_params([self.a.weight, self.b.weight]).view(12, 4)
            tap("gemm", both, x.shape[0] * x.shape[2] * 4 * 12, (("x", ops.Spikes(x)),))
            tap("linear", self.c.weight, 5 * 6 * 3, (("x", torch.full((5, 6), 0.3)),))
            tap("sdsa:kv", None, 77, (("k", x), ("v", x * 2)))
            tap("gemm", self.b.weight.view(6, 4)[2:4], 99, (("x", x),))          # rows 2 .. 3 of b: still b's row
        return x


def test_opcensus_keys_passes_and_switches():
    import spike2former_amd as s2f
    from spike2former_amd import maskformer_head, ops
    model = Toy().train()
    x = (torch.arange(2 * 4 * 5) % 9).float().view(2, 4, 5) / 8
    before = (maskformer_head.FOLD_MASK_FEATURE, maskformer_head.PREDICT_LAST_ONLY)
    with s2f.OpCensus(model, max_passes=2, D=8) as census:
        assert ops.census_active() and not model.training and not torch.is_grad_enabled()
        assert (maskformer_head.FOLD_MASK_FEATURE, maskformer_head.PREDICT_LAST_ONLY) == (False, False)
        with pytest.raises(RuntimeError):
            s2f.OpCensus(model).__enter__()
        model(x)
        model(x)
        assert ops.census_active()
        model(x)                                    # the third forward: the taps have gone quiet, the switches are back
        assert not ops.census_active()
        assert (maskformer_head.FOLD_MASK_FEATURE, maskformer_head.PREDICT_LAST_ONLY) == before
        rep = census.report()
    assert model.training and torch.is_grad_enabled() and not ops.census_active()
    assert [r["key"] for r in rep.rows] == ["a.weight", "b.weight", "c.weight", ":sdsa:kv"]
    a, b, c, kv = rep.rows
    assert rep.totals["passes"] == 2 and rep.totals["params"] == 24 + 24 + 18 + 3
    assert a["macs"] == 2 * 5 * 4 * 6 and a["calls"] == 2 and b["macs"] == a["macs"] + 99 and b["calls"] == 4
    want = R.census(x.numpy(), 8)
    got = a["operands"][0]
    assert (got["elements"], got["level_sum"], got["nonzero"], got["off_grid"], got["max_level"]) == \
        (2 * want[R.ELEMENTS], 2 * want[R.LEVEL_SUM], 2 * want[R.NONZERO], 0, 8) and got["spikes"]
    assert a["klass"] == "ac" and a["rate"] == want[R.LEVEL_SUM] / want[R.ELEMENTS]
    assert c["klass"] == "real" and c["off_share"] == 1.0 and c["macs"] == 90
    assert kv["klass"] == "ac" and [o["name"] for o in kv["operands"]] == ["k", "v"] and kv["rate"] == a["rate"]
    assert rep.spikes_off_grid() == []


def test_a_membrane_of_another_size_is_refused_before_any_launch():
    """A neuron reads one kept membrane value per input element.  The census switches change the shapes the SDME block's neurons see
    (all L + 1 decoder layers instead of the last), so OpCensus resets the membranes at both of its borders, and a neuron that still
    meets a membrane of another size raises instead of handing the kernel a buffer that is too short."""
    import spike2former_amd as s2f
    n = s2f.Q_IFNode(surrogate_function=s2f.Quant())
    n.v = torch.zeros(1, 2, 10, 4)
    with pytest.raises(RuntimeError, match="membrane kept from the last pass"):
        n(torch.zeros(3, 2, 10, 4))

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.n = n
            self.w = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):
            return x
    net = Net()
    with s2f.OpCensus(net, max_passes=1):
        assert isinstance(n.v, float)          # reset when the census begins
        n.v = torch.zeros(3, 2, 10, 4)
        net(torch.zeros(1))
        net(torch.zeros(1))                    # the second forward: the census goes quiet ...
        assert isinstance(n.v, float)          # ... and resets again


def test_report_refuses_ops_counted_outside_a_call_of_the_model():
    """a pass is one call of the model: ops reported from a method driven directly have no pass to average over"""
    import spike2former_amd as s2f
    model = Toy()
    x = torch.zeros(2, 4, 5)
    with s2f.OpCensus(model, D=8) as census:
        model.forward(x)
        with pytest.raises(RuntimeError, match="no forward went through the model's call"):
            census.report()
        model(x)
        assert census.report().totals["passes"] == 1
