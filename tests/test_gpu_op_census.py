"""GPU: the operand census -- s2f_operand_census (csrc/opcensus.hip) against the numpy restatement tests/census_ref.py in exact
integers at the wave, vector, workgroup and grid-stride boundaries and at unaligned starts; OpCensus on the tiny configuration C1_64
against the oracle's own layer list (MACs and on-grid / real class per parameter name) and against the neurons' forward hooks of the
same forward (levels); the census around `evaluate` and beside a GraphedPredict."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import census_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

D = 8
SIZES = (0, 1, 7, 63, 64, 65, 255, 256, 257, 4096 + 3, 2 ** 20 + 5)
PAD = 16          # elements of NaN in front of and behind every operand: what surrounds it must not be counted


# ---------------------------------------------------------------------------------------------------- the kernel
def values(n, seed):
    """fp32 [n]: random levels 0 .. 39 on the grid 1 / 8 (exact in bf16 too), with off-grid, negative, subnormal and non-finite
    values sprinkled in"""
    rng = np.random.default_rng(seed)
    x = (rng.integers(0, 40, n) * (rng.random(n) < 0.6)).astype(np.float32) / D
    odd = np.array([0.3, -0.125, np.nan, np.inf, -np.inf, 1e-40, -0.0, 8192.0, 65535.0 / D, 2.0 ** -130], np.float32)
    where = rng.random(n) < 0.05
    x[where] = odd[rng.integers(0, len(odd), int(where.sum()))]
    return x


def framed(x, offset, dtype):
    """-> (buffer, the operand as a view of it `offset` elements behind a 16-byte boundary): NaN all around"""
    buf = torch.full((PAD + offset + x.size + PAD,), float("nan"), dtype=dtype, device="cuda")
    view = buf[PAD + offset:PAD + offset + x.size]
    view.copy_(torch.from_numpy(x))
    assert buf.data_ptr() % 16 == 0 and (view.numel() == 0 or view.data_ptr() == buf.data_ptr() + (PAD + offset) * buf.element_size())
    return buf, view


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_kernel_equals_the_restatement(dtype, offset):
    from spike2former_amd import ops
    cases = [framed(values(n, 1000 + n + offset), offset, dtype) for n in SIZES]
    # row 2 i: operand i, once; row 2 i + 1: must stay zero.  The last two rows: operands 3 and 9 added into one row; untouched.
    tables = [torch.zeros(2 * len(cases) + 2, 8, dtype=torch.int64, device="cuda") for _ in range(2)]
    for table in tables:          # the second table: the same launches again -- the same bits
        for i, (_, view) in enumerate(cases):
            assert view.numel() == SIZES[i]
            ops.operand_census(view, table[2 * i], D)
        ops.operand_census(cases[3][1], table[-2], D)
        ops.operand_census(cases[9][1], table[-2], D)
    got = tables[0].cpu().numpy()
    want = np.zeros_like(got)
    for i, (_, view) in enumerate(cases):
        R.census(view.float().cpu().numpy(), D, want[2 * i])          # (what the operand holds: bf16 rounds 0.3 and 65535 / 8)
    R.census(cases[3][1].float().cpu().numpy(), D, want[-2])
    R.census(cases[9][1].float().cpu().numpy(), D, want[-2])
    for i in range(len(want)):
        assert got[i].tolist() == want[i].tolist(), (i, SIZES[i // 2] if i // 2 < len(SIZES) else "pair", got[i], want[i])
    assert want[2 * 10][R.OFF_GRID] > 0 and want[2 * 10][R.NONFINITE] > 0 and want[2 * 10][R.LEVEL_SUM] > 0
    assert want[-2][R.CALLS] == 2 and want[0].tolist() == [0, 0, 0, 0, 0, 0, 1, 0]
    assert torch.equal(tables[0], tables[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_kernel_beyond_one_sweep_of_the_grid(dtype):
    """The launch is at most 512 workgroups of 1024 threads, two 16-byte groups in flight per thread: operands with more than 2^19
    groups (the second load of a thread is real for some threads only), and with more than 2^20 (the grid-stride loop comes round)"""
    from spike2former_amd import ops
    vec = 16 // torch.empty(0, dtype=dtype).element_size()
    table = torch.zeros(2, 8, dtype=torch.int64, device="cuda")
    for i, groups in enumerate((2 ** 19 + 300, 2 ** 20 + 1024 + 77)):
        buf, view = framed(values(vec * groups + 5, 7 + i), 1, dtype)
        ops.operand_census(view, table[i], D)
        assert table[i].tolist() == R.census(view.float().cpu().numpy(), D).tolist(), groups


def test_partial_sums_hold_the_largest_level():
    """2^20 + 5 elements of level 65535: the sum is 16 times 2^32, and a 32-bit sum per thread, wave or workgroup would wrap"""
    from spike2former_amd import ops
    n = 2 ** 20 + 5
    buf, view = framed(np.full(n, 65535.0 / D, np.float32), 1, torch.float32)
    row = torch.zeros(8, dtype=torch.int64, device="cuda")
    ops.operand_census(view, row, D)
    assert row.tolist() == [n, 65535 * n, n, 0, 65535, 0, 1, 0] and 65535 * n > 15 * 2 ** 32


def test_spikes_and_a_strided_operand():
    from spike2former_amd import ops
    y = (torch.arange(6 * 10, device="cuda") % 9).float().view(6, 10) / D
    rows = torch.zeros(2, 8, dtype=torch.int64, device="cuda")
    ops.operand_census(ops.Spikes(y.bfloat16()), rows[0], D)
    ops.operand_census(y.t()[2:7], rows[1], D)          # neither contiguous nor aligned
    assert rows[0].tolist() == R.census(y.cpu().numpy(), D).tolist()
    assert rows[1].tolist() == R.census(y.t()[2:7].cpu().numpy(), D).tolist()


# ---------------------------------------------------------------------------------------------------- the tiny model
@pytest.fixture(scope="module")
def tiny():
    import spike2former_amd as s2f
    from oracle import s2f_oracle as so
    cfg = so.CONFIGS["C1_64"]
    st = so.make_params(cfg, requires_grad=False)
    model = s2f.MODELS.build(s2f.model_cfg("C1_64"))
    model.load_state_dict(st, strict=True)
    model.cuda().eval()
    return s2f, so, cfg, st, model, so.synthetic_image(dataclasses.replace(cfg, B=1))          # one picture


def plain_logits(s2f, model, img):
    with torch.no_grad():
        s2f.reset_net(model)
        return model(img.cuda(), mode="logits").clone()


def oracle_layers(so, cfg, st, img):
    """The oracle's own layer list: subclass OracleNet, override its conv2d / conv1d primitives -> {weight key: [MACs, on grid, fed]}
    (MACs = output elements x fan-in, summed over the calls; on grid: x * D is an integer in [0, 65535] everywhere, in every call;
    fed: the input has a non-zero element in some call)"""
    seen = {}

    class Counting(so.OracleNet):
        def _note(self, name, x, y):
            w = self.p[name + ".weight"]
            p = x.detach() * cfg.D
            on = bool(((p == p.round()) & (p >= 0) & (p <= 65535)).all())
            rec = seen.setdefault(name + ".weight", [0, True, False])
            rec[0] += y.numel() * (w.numel() // w.shape[0])
            rec[1] = rec[1] and on
            rec[2] = rec[2] or bool((x != 0).any())
            return y

        def conv2d(self, name, x, stride=1, padding=0, groups=1):
            return self._note(name, x, super().conv2d(name, x, stride, padding, groups))

        def conv1d(self, name, x):
            return self._note(name, x, super().conv1d(name, x))

    with torch.no_grad():
        Counting({k: v.clone() for k, v in st.items()}, cfg, training=False).predict(img)
    return seen


@pytest.fixture(scope="module")
def census_pass(tiny):
    """ONE census pass of model(img, mode='logits') on the tiny model with a forward hook on every neuron (its own census of the same
    forward) -> (report, logits, {neuron: [level sum, non-zero, elements]}, the plain logits before, the plain logits after)"""
    s2f, so, cfg, st, model, img = tiny
    from spike2former_amd import maskformer_head
    before = plain_logits(s2f, model, img)
    switches = (maskformer_head.FOLD_MASK_FEATURE, maskformer_head.PREDICT_LAST_ONLY)
    fired = {}

    def grab(mod, inp, out, n):
        if n not in fired:          # (as spike_census of tests/test_gpu_model.py: a neuron fired by its producer's kernel reports twice)
            o = out.detach().float()
            fired[n] = [int((o * mod.D).round().sum().item()), int((o != 0).sum().item()), o.numel()]
    hooks = [m.register_forward_hook(lambda m_, i_, o_, n=n: grab(m_, i_, o_, n)) for n, m in model.named_modules()
             if isinstance(m, s2f.Q_IFNode)]
    s2f.reset_net(model)
    with s2f.OpCensus(model, max_passes=5) as census:
        assert (maskformer_head.FOLD_MASK_FEATURE, maskformer_head.PREDICT_LAST_ONLY) == (False, False)
        hooked = model(img.cuda(), mode="logits").clone()
        rep = census.report()
    for h in hooks:
        h.remove()
    assert (maskformer_head.FOLD_MASK_FEATURE, maskformer_head.PREDICT_LAST_ONLY) == switches
    # the census alone (no hooks: the neurons keep their fused routes)
    s2f.reset_net(model)
    with s2f.OpCensus(model) as census:
        logits = model(img.cuda(), mode="logits").clone()
        rep_alone = census.report()
    assert (maskformer_head.FOLD_MASK_FEATURE, maskformer_head.PREDICT_LAST_ONLY) == switches
    after = plain_logits(s2f, model, img)
    print(rep_alone)
    return dict(rep=rep, rep_alone=rep_alone, hooked=hooked, logits=logits, fired=fired, before=before, after=after)


def test_every_oracle_layer_has_a_row_with_its_macs_and_class(tiny, census_pass):
    """Every layer the oracle runs has a row with equal MACs and the same class.  The stem is real, every pwconv1 and SepConv
    depthwise convolution accumulate-only.  `pwconv2` is real exactly where its depthwise convolution saw a spike: on these seeded
    weights in eval mode that is ConvBlock1_1 only (spike2 rate 0.0035); in ConvBlock1_2, 2_1 and 2_2 spike2 is silent for every
    picture tried, the depthwise output is identically zero -- on the grid, by the oracle's count too -- and the row is
    accumulate-only with 0 SOPs."""
    s2f, so, cfg, st, model, img = tiny
    want = oracle_layers(so, cfg, st, img)
    assert len(want) > 100
    for rep in (census_pass["rep"], census_pass["rep_alone"]):
        rows = {r["key"]: r for r in rep.rows}
        assert len(rows) == len(rep.rows) and rep.totals["passes"] == 1
        missing = sorted(k for k in want if k not in rows)
        assert not missing, missing
        wrong = [(k, rows[k]["macs"], m) for k, (m, _, _) in want.items() if rows[k]["macs"] != m]
        assert not wrong, wrong[:10]
        klass = [(k, rows[k]["klass"], on) for k, (_, on, _) in want.items() if (rows[k]["klass"] == "ac") != on]
        assert not klass, klass[:10]
        # the layers that read no neuron are real, the ones behind a neuron accumulate-only
        assert rows["backbone.downsample1_1.encode_conv.weight"]["klass"] == "real"
        pw2 = [k for k in rows if k.endswith("pwconv2.weight") and k.startswith("backbone.")]
        pw1 = [k for k in rows if k.endswith("pwconv1.weight") or k.endswith(".Conv.dwconv.weight")]
        assert len(pw2) == 4 and len(pw1) == 8 and all(rows[k]["klass"] == "ac" for k in pw1)
        # SepConv.pwconv2 reads the depthwise convolution's output: real-valued wherever that convolution saw a spike.  In eval mode
        # on these seeded weights spike2 of ConvBlock1_2, 2_1 and 2_2 is silent for every picture tried (12 seeds, the picture times
        # 4, 16 and 64, on the oracle): their depthwise output is identically zero, and a map of zeros IS on the grid -- the oracle's
        # class above says so too.  So: real exactly where the depthwise convolution's own operand has a spike, which it has in
        # ConvBlock1_1 (rate 0.0035 there)
        for k in pw2:
            spiking = want[k.replace("pwconv2", "dwconv")][2]          # by the ORACLE's count: spike2 fired somewhere
            assert (rows[k]["klass"] == "real") == spiking, (k, rows[k]["klass"], spiking)
            assert spiking or (rows[k]["operands"][0]["nonzero"] == 0 and rows[k]["sops"] == 0.0)
        assert rows["backbone.ConvBlock1_1.0.Conv.pwconv2.weight"]["klass"] == "real"
        # every weight of the model that a convolution or a linear layer applies has a row; the weightless products are there too
        kinds = {r["kind"] for r in rep.rows}
        assert {"sdsa:kv", "sdsa:q_kv", "dcnv3:sample", "dcnv3:modulate", "mask_einsum", "class_mask_product", "linear"} <= kinds, kinds
        for k in ("decode_head.cls_embed.weight", "decode_head.mask_embed.fc1.weight", "decode_head.mask_embed.fc_out.weight"):
            assert rows[k]["klass"] == "ac", k          # alpha * spikes: multiples of 1 / 2
        assert rep.totals["params"] == sum(v.numel() for k, v in st.items() if k in dict(model.named_parameters()))
        assert rep.totals["macs"] == sum(r["macs"] for r in rep.rows) and 0 < rep.totals["real_macs"] < rep.totals["macs"]


def test_pwconv2_is_real_wherever_the_oracle_sees_a_spike_in_front_of_it(tiny):
    """The same picture 16 times as bright: spike2 now fires in ConvBlock1_1 AND ConvBlock1_2 (rates 0.30 and 0.012 on the oracle; in
    ConvBlock2_1 and 2_2 it stays silent at every amplitude tried, 1 to 64).  Which pwconv2 is real is read off the oracle, not off
    the census."""
    s2f, so, cfg, st, model, img = tiny
    bright = 16.0 * img
    want = oracle_layers(so, cfg, st, bright)
    s2f.reset_net(model)
    with s2f.OpCensus(model) as census:
        model(bright.cuda(), mode="logits")
        rows = {r["key"]: r for r in census.report().rows}
    pw2 = [k for k in want if k.endswith("pwconv2.weight") and k.startswith("backbone.")]
    fed = [k for k in pw2 if want[k.replace("pwconv2", "dwconv")][2]]
    assert len(pw2) == 4 and sorted(fed) == ["backbone.ConvBlock1_1.0.Conv.pwconv2.weight", "backbone.ConvBlock1_2.0.Conv.pwconv2.weight"]
    for k in pw2:
        assert rows[k]["macs"] == want[k][0] and (rows[k]["klass"] == "real") == (k in fed) == (not want[k][1]), (k, rows[k]["klass"])
    for k in want:
        if k.endswith("pwconv1.weight") or k.endswith(".Conv.dwconv.weight"):
            assert rows[k]["klass"] == "ac" and want[k][1], k
    assert rows["backbone.downsample1_1.encode_conv.weight"]["klass"] == "real"


def test_weightless_rows_are_keyed_by_module_path_and_count_what_the_kernels_contract(tiny, census_pass):
    s2f, so, cfg, st, model, img = tiny
    rows = {r["key"]: r for r in census_pass["rep_alone"].rows}
    T, B = cfg.T, 1
    a = "backbone.block3.0.attn"
    assert a + ":sdsa:kv" in rows and a + ":sdsa:q_kv" in rows, [k for k in rows if "sdsa" in k][:6]
    C = st[a + ".q_conv.0.body.0.weight"].shape[0]
    d = C // cfg.num_heads
    N = rows[a + ":sdsa:q_kv"]["operands"][0]["elements"] // (T * B * C)
    assert rows[a + ":sdsa:kv"]["macs"] == T * B * cfg.num_heads * N * d * d == rows[a + ":sdsa:q_kv"]["macs"]
    assert [o["name"] for o in rows[a + ":sdsa:kv"]["operands"]] == ["k", "v"] and rows[a + ":sdsa:kv"]["klass"] == "ac"
    me = [r for r in rows.values() if r["kind"] == "mask_einsum"]
    assert len(me) == 1 and me[0]["key"] == "decode_head:mask_einsum"
    e, mf = me[0]["operands"]
    L1, Q = cfg.dec_layers + 1, cfg.num_queries
    assert e["elements"] % (T * B * L1 * Q) == 0          # every layer's prediction: PREDICT_LAST_ONLY stepped aside
    Cm = e["elements"] // (T * B * L1 * Q)
    assert me[0]["macs"] == T * B * L1 * Q * Cm * (mf["elements"] // (T * B * Cm))
    assert e["off_grid"] == 0 and e["max_level"] <= 4 * D and mf["off_grid"] > 0 and me[0]["klass"] == "ac"
    cm = [r for r in rows.values() if r["kind"] == "class_mask_product"]
    assert len(cm) == 1 and cm[0]["macs"] == B * cfg.num_classes * Q * cfg.H * cfg.W and cm[0]["klass"] == "real"
    dcn = [r for r in rows.values() if r["kind"] == "dcnv3:sample"]
    mod = {r["key"].replace("modulate", "sample"): r for r in rows.values() if r["kind"] == "dcnv3:modulate"}
    # the encoder runs its layers through a method of theirs: one path, the second layer's products carry the ordinal 1
    pd = "decode_head.pixel_decoder:dcnv3:"
    assert [r["key"] for r in dcn] == [pd + "sample", pd + "sample:1"] and sorted(mod) == [pd + "sample", pd + "sample:1"]
    for r in dcn:
        m = mod[r["key"]]
        assert r["calls"] == 1 and r["macs"] == 4 * m["macs"] and m["klass"] == "ac" and m["operands"][0]["spikes"]          # the mask neuron's output


PAIRS = [          # (neuron, the op that reads its output and nothing else), one per block type
    ("backbone.ConvBlock1_1.0.Conv.spike1", "backbone.ConvBlock1_1.0.Conv.pwconv1.weight"),
    ("backbone.ConvBlock1_1.0.Conv.spike2", "backbone.ConvBlock1_1.0.Conv.dwconv.weight"),
    ("backbone.ConvBlock2_1.0.spike1", "backbone.ConvBlock2_1.0.conv1.weight"),
    ("backbone.downsample2.encode_spike", "backbone.downsample2.encode_conv.weight"),
    ("backbone.block3.0.attn.head_spike", "backbone.block3.0.attn.k_conv.0.body.0.weight"),
    ("backbone.block3.1.mlp.fc2_spike", "backbone.block3.1.mlp.fc2_conv.weight"),
    ("decode_head.pixel_decoder.last_feat_conv_spike", "decode_head.pixel_decoder.encoder_in_proj.0.weight"),
    ("decode_head.pixel_decoder.encoder.layers.0.ffn.fc1_spike", "decode_head.pixel_decoder.encoder.layers.0.ffn.fc1_conv.weight"),
    ("decode_head.pixel_decoder.mask_feature_spike", "decode_head.pixel_decoder.mask_feature.weight"),
    ("decode_head.transformer_decoder.layers.0.cross_attn.attn.attn_spike", "decode_head.transformer_decoder.layers.0.cross_attn.attn.out_conv.0.weight"),
    ("decode_head.transformer_decoder.layers.1.ffn.fc2_spike", "decode_head.transformer_decoder.layers.1.ffn.fc2.weight"),
]


def test_levels_equal_the_neurons_own_census_of_the_same_forward(census_pass):
    rows = {r["key"]: r for r in census_pass["rep"].rows}
    fired = census_pass["fired"]
    for neuron, key in PAIRS:
        assert neuron in fired and key in rows, (neuron, key)
        op = rows[key]["operands"]
        assert len(op) == 1
        assert [op[0]["level_sum"], op[0]["nonzero"], op[0]["elements"]] == fired[neuron], (neuron, key)
        assert op[0]["off_grid"] == 0 and op[0]["max_level"] <= D
    assert sum(fired[n][0] for n, _ in PAIRS) > 0


def test_spike_maps_are_on_the_grid_and_the_census_leaves_the_model_as_it_was(census_pass):
    c = census_pass
    assert c["rep"].spikes_off_grid() == [] and c["rep_alone"].spikes_off_grid() == []
    assert any(o["spikes"] for r in c["rep_alone"].rows for o in r["operands"])
    assert not any(o["nonfinite"] for r in c["rep_alone"].rows for o in r["operands"])
    # the tolerance of the fused-against-unfused comparison of the eval routes (tests/test_gpu_round5.py): 1e-4 of the logits' range,
    # the same arg-max on 99.9 % of the pixels
    rng = (c["before"].max() - c["before"].min()).item()
    for name in ("logits", "hooked"):
        gap = (c[name] - c["before"]).abs().max().item()
        print(f"census pass ({name}) against the plain pass: max |d| {gap:.3e}, range {rng:.3e}")
        assert gap <= 1e-4 * rng, (name, gap, rng)
        assert (c[name].argmax(1) == c["before"].argmax(1)).float().mean().item() >= 0.999
    assert torch.equal(c["after"], c["before"])          # a following plain pass: bit for bit the earlier one
    text = str(c["rep_alone"])
    assert "total: params" in text and "real MACs" in text and "mJ" in text


def test_a_census_straight_after_a_plain_pass_starts_from_reset_membranes(tiny, census_pass):
    """A plain `predict` leaves the SDME block's neurons with membranes of ONE decoder layer's rows; a census pass evaluates all
    L + 1 layers.  OpCensus resets the membranes when it begins and when it ends, so a census entered without a reset_net of the
    caller's counts what a reset pass counts, and the plain pass after it is the plain pass again."""
    s2f, so, cfg, st, model, img = tiny
    plain_logits(s2f, model, img)
    assert not isinstance(model.decode_head.decoder_out_spike.v, float)          # a membrane is kept: [1, T, B, Q, C]
    with s2f.OpCensus(model) as census:
        logits = model(img.cuda(), mode="logits").clone()
        assert model.decode_head.decoder_out_spike.v.shape[0] == cfg.dec_layers + 1
        rep = census.report()
    assert isinstance(model.decode_head.decoder_out_spike.v, float)
    assert torch.equal(logits, census_pass["logits"])
    want = {r["key"]: (r["macs"], r["operands"]) for r in census_pass["rep_alone"].rows}
    assert {r["key"]: (r["macs"], r["operands"]) for r in rep.rows} == want
    with torch.no_grad():
        assert torch.equal(model(img.cuda(), mode="logits"), census_pass["before"])          # (no reset_net of the caller's here either)


def test_census_around_evaluate_counts_two_passes_and_changes_no_metric(tiny, census_pass):
    s2f, so, cfg, st, model, img = tiny
    from spike2former_amd.data_preprocessor import SegDataSample
    K = cfg.num_classes
    gen = torch.Generator().manual_seed(3)
    batches = []
    for i in range(3):
        lab = torch.randint(0, K, (cfg.H // 8, cfg.W // 8), generator=gen).repeat_interleave(8, 0).repeat_interleave(8, 1).to(torch.uint8)[None]
        meta = dict(img_shape=(cfg.H, cfg.W), ori_shape=(cfg.H, cfg.W), pad_shape=(cfg.H, cfg.W), padding_size=[0, 0, 0, 0], flip=False)
        batches.append(dict(inputs=[so.synthetic_image(cfg, seed=10 + i)[0]], data_samples=[SegDataSample(gt_sem_seg=lab.contiguous(), metainfo=meta)]))

    def metric():
        m = s2f.IoUMetric(iou_metrics=["mIoU"])
        m.dataset_meta = dict(classes=[str(i) for i in range(K)])
        return m
    plain = s2f.evaluate(model, batches, metric())
    with s2f.OpCensus(model, max_passes=2) as census:
        got = s2f.evaluate(model, batches, metric())
        rep = census.report()
    assert list(got) == list(plain)
    for k in plain:
        assert got[k] == plain[k] or (np.isnan(got[k]) and np.isnan(plain[k])), (k, got[k], plain[k])
    assert rep.totals["passes"] == 2
    single = {r["key"]: r["macs"] for r in census_pass["rep_alone"].rows}
    assert {r["key"]: r["macs"] for r in rep.rows} == single
    assert all(r["calls"] % 2 == 0 for r in rep.rows)


def test_a_graphed_predict_runs_the_census_pass_eager_and_replays_afterwards(tiny):
    s2f, so, cfg, st, model, img = tiny
    x = img.cuda().contiguous()
    was = model.test_cfg
    model.test_cfg = dict(mode="whole", graph=dict(capture_after=1))
    model.__dict__.pop("_graphed_predict", None)
    try:
        with torch.no_grad():
            with s2f.OpCensus(model) as census:
                model(x, mode="logits")
                model(x, mode="logits")
                rep = census.report()
            gp = model.graphed_predict()
            assert gp.census == dict(captures=0, replays=0, evictions=0, eager={"op_census": 2})
            assert rep.totals["passes"] == 2 and len(rep.rows) > 100
            first = model(x, mode="logits").clone()          # the census is over: captured ...
            again = model(x, mode="logits").clone()          # ... and replayed
            assert gp.census == dict(captures=1, replays=1, evictions=0, eager={"op_census": 2})
            assert torch.equal(first, again)
    finally:
        model.test_cfg = was
        model.__dict__.pop("_graphed_predict", None)
    assert torch.equal(plain_logits(s2f, model, img), first)
