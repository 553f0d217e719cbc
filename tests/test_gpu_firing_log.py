"""GPU: the firing log -- s2f_firing_log_append (csrc/firinglog.hip) against the numpy restatement tests/firing_ref.py in exact
integers, its streaks and its latch, the launch inside a captured graph, and FiringLog inside GraphedHungarianStep and TrainLoop on
the tiny configuration C1_64 (the rig of tests/step_rig.py, with a FiringLog).  Rigs are built once for the module:
    still -- optimizer=None: the weights stand still (the BatchNorm running statistics, which the forward reads, still move)
    train -- with a FlatAdamW, a TrainLog and a FiringLog: what TrainLoop drives"""
import json
import logging
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import firing_ref as R  # noqa: E402
from step_rig import reset, rigs_fixture  # noqa: E402

pytestmark = pytest.mark.gpu

SLOTS = 256
GUARD = -0x5A5A5A5A5A5A5A5A


# ---------------------------------------------------------------------------------------------------- (a), (b): the kernel
class Device:
    """the state of one log on the device next to the restatement's"""

    def __init__(self, n, window, silent=None):
        self.ring, self.silent, self.head = R.new_state(n, window, silent)
        self.ring[:] = GUARD          # rows no launch has written yet must stay what they were
        self.d_ring, self.d_silent, self.d_head = (torch.from_numpy(a.copy()).cuda() for a in (self.ring, self.silent, self.head))
        self.d_counters = torch.zeros(n, SLOTS, 2, dtype=torch.int64, device="cuda")

    def append(self, counters, patience):
        """one launch on `counters` (int64 [n, SLOTS, 2], numpy), one step of the restatement; everything compared exactly"""
        from spike2former_amd import ops
        self.d_counters.copy_(torch.from_numpy(counters))
        ops.firing_log_append(self.d_counters, self.d_ring, self.d_silent, self.d_head, patience)
        R.append(counters.copy(), self.ring, self.silent, self.head, patience)
        torch.cuda.synchronize()
        assert int(self.d_counters.ne(0).sum()) == 0
        head = self.d_head.cpu().numpy()
        assert head[2] == 0 and head.tolist() == self.head.tolist(), (head, self.head)
        assert np.array_equal(self.d_ring.cpu().numpy(), self.ring)          # the new row AND every other row, untouched
        assert np.array_equal(self.d_silent.cpu().numpy(), self.silent)


def synthetic(rng, n, it):
    """int64 [n, SLOTS, 2]: by neuron and iteration one of -- silent; only slot 0; only slot 255; all slots -- and in every
    second firing neuron one slot holding values at or above 2^33 whose low halves carry into the high ones when added
    (per-neuron totals stay below 2^62)"""
    c = np.zeros((n, SLOTS, 2), np.int64)
    for i in range(n):
        kind = (i + it) % 4
        if kind == 0:
            continue
        slots = [0] if kind == 1 else [SLOTS - 1] if kind == 2 else list(range(SLOTS))
        c[i, slots, 1] = rng.integers(1, 1 << 31, len(slots))
        c[i, slots, 0] = c[i, slots, 1] * rng.integers(1, 9, len(slots))
        if i % 2 == 0:
            c[i, slots[0]] += [(1 << 52) + (1 << 33) + 0xffffffff, (1 << 33) + 0xfffffff0]
            c[i, slots[-1], 0] += 0xffffffff          # (a second all-ones low half: low halves alone overflow 32 bits)
        assert int(c[i, :, 0].sum()) < 1 << 62
    return c


@pytest.mark.parametrize("n", [1, 3, 64, 65, 300])
def test_kernel_equals_the_restatement(n):
    rng = np.random.default_rng(100 + n)
    dev = Device(n, window=3)
    for it in range(7):
        dev.append(synthetic(rng, n, it), patience=5)
    assert dev.d_head.tolist()[0] == 7
    # all slots holding large values: every lane's partial sum carries
    big = np.full((n, SLOTS, 2), (1 << 33) + 0xfffffff1, np.int64)
    dev.append(big, patience=5)
    assert dev.ring[7 % 3, 0].tolist() == [SLOTS * ((1 << 33) + 0xfffffff1)] * 2


@pytest.mark.parametrize("patience", [1, 3])
def test_streaks_and_latch(patience):
    n = 70
    start = np.zeros(n, np.int32)
    start[[1, 66]] = -1
    dev = Device(n, window=2, silent=start)
    fire = np.zeros((n, SLOTS, 2), np.int64)
    fire[:, 9] = [24, 3]

    def row(quiet):
        c = fire.copy()
        c[list(quiet)] = 0
        return c
    # neurons 1 and 66 are not watched and never fire; 5 and 68 go silent together; 2 fires once in between; 0 goes silent later
    for _ in range(patience - 1):
        dev.append(row([1, 66, 5, 68, 2]), patience)
        assert R.first_dead(dev.head) is None
    dev.append(row([1, 66, 5, 68]), patience)          # 2 fires: its streak starts again; 5 and 68 reach the patience
    assert R.first_dead(dev.head) == (patience - 1, 5)          # two neurons in one row: the lower index
    assert dev.silent[[1, 66]].tolist() == [-1, -1] and dev.silent[[5, 68]].tolist() == [patience, patience] and dev.silent[2] == 0
    for _ in range(patience + 1):
        dev.append(row([1, 66, 5, 68, 0, 2]), patience)          # later events (neurons 0 and 2) do not replace the latch
    assert R.first_dead(dev.head) == (patience - 1, 5) and int(dev.d_head[1]) == ((patience - 1) << 32) + 5
    assert dev.silent[[0, 2]].tolist() == [patience + 1] * 2 and dev.silent[[1, 66]].tolist() == [-1, -1]
    dev.append(row([1, 66]), patience)          # a spike resets the streak; the latch stays
    assert dev.silent[[0, 2, 5, 68]].tolist() == [0] * 4 and R.first_dead(dev.head) == (patience - 1, 5)
    assert np.array_equal(dev.d_silent.cpu().numpy(), dev.silent)


# ---------------------------------------------------------------------------------------------------- (c): under capture
def test_append_in_a_captured_graph_equals_eager():
    from spike2former_amd import ops
    g = torch.Generator().manual_seed(9)
    xs = [(torch.randn(4096, generator=g) * s).cuda() for s in (0.5, 2.0, 6.0)]

    def new():
        buf = types.SimpleNamespace(counters=torch.zeros(3, SLOTS, 2, dtype=torch.int64, device="cuda"),
                                    ring=torch.zeros(8, 3, 2, dtype=torch.int64, device="cuda"),
                                    silent=torch.zeros(3, dtype=torch.int32, device="cuda"),
                                    head=torch.tensor([0, -1, 0, 0], dtype=torch.int64, device="cuda"))
        return buf

    def step(b):
        with torch.no_grad():
            for i, x in enumerate(xs):
                ops.lif(x, None, 8, 1.0, False, b.counters[i])
            ops.firing_log_append(b.counters, b.ring, b.silent, b.head, 2)
    eager, graphed = new(), new()
    for _ in range(5):
        step(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(graphed)          # (warm-up: the allocator's pools)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphed.counters.zero_(), graphed.ring.zero_(), graphed.silent.zero_()
    graphed.head.copy_(torch.tensor([0, -1, 0, 0]))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(graphed)
    torch.cuda.synchronize()
    assert graphed.head.tolist() == [0, -1, 0, 0]          # recording ran nothing
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    assert graphed.head.tolist() == eager.head.tolist() == [5, -1, 0, 0]
    assert torch.equal(graphed.ring, eager.ring) and int(graphed.counters.ne(0).sum()) == 0
    rows = graphed.ring[:5].cpu()
    assert bool((rows[:, :, 1] > 0).all()) and bool((rows == rows[0]).all()) and int(graphed.ring[5:].ne(0).sum()) == 0
    assert int(rows[0, 0, 0]) < int(rows[0, 1, 0]) < int(rows[0, 2, 0])          # three different neurons' counts


# ---------------------------------------------------------------------------------------------------- (d) - (f): the step
# a BatchNorm that feeds a neuron (backbone_sdtv2.py SepConv.forward: pwconv1 -> bn1 -> spike2), early in named_modules() order: the
# tiny configuration has neurons that never fire of its own (block3's attn_spike), and the latch keeps the lowest index of a row
DEAD_BN, DEAD_NEURON = "backbone.ConvBlock1_1.0.Conv.bn1", "backbone.ConvBlock1_1.0.Conv.spike2"


FIRING = dict(window=8, patience=3)
recipes = dict(still=dict(optimizer=False, log=False, firing=FIRING), train=dict(firing=FIRING))
rigs = rigs_fixture(recipes)


def test_row_zero_is_the_forward_of_the_step(rigs):
    import spike2former_amd as s2f
    from spike2former_amd import ops
    r = rigs("still")
    reset(r)
    fl = r.firing
    assert r.step.firing is fl and fl.attached and r.step.two_graphs is False
    watched = fl.elems > 0
    assert int(watched.sum()) >= 100 and fl.read().count == 0          # the warm-up passes' spikes are not row 0
    # one eager train-mode forward on the step's input, counted by the same counters
    s2f.reset_net(r.model)
    out = r.model(r.step.static_in)
    torch.cuda.synchronize()
    want = ops.read_stats(fl.counters).cpu().numpy()
    del out
    # back to the reset state, log cleared: a train-mode forward moves the BatchNorm running statistics, and the forward READS them
    # (the RepConv branches pad with their BatchNorm's response to zero, backbone_sdtv2.py BNAndPadLayer)
    reset(r)
    r.step()
    read = fl.read()
    assert read.count == 1 and read.sums.shape == (1, fl.n, 2) and read.first_dead is None
    differ = [(fl.names[i], want[i].tolist(), read.sums[0][i].tolist()) for i in np.flatnonzero((read.sums[0] != want).any(1))]
    assert not differ, f"{len(differ)} neurons' rows are not the eager forward's counters (name, eager, row 0): {differ[:8]}"
    assert np.array_equal(read.sums[0][watched.numpy()], want[watched.numpy()])
    assert int(want[~watched.numpy()].sum()) == 0 and int(read.sums[0][~watched.numpy()].sum()) == 0
    assert int(fl.counters.ne(0).sum()) == 0
    r.step()
    r.step()
    read = fl.read()
    assert int(fl.counters.ne(0).sum()) == 0 and read.count == 3 and np.array_equal(read.sums[0], want)
    D = np.array([m.D for m in fl.nodes.values()], np.int64)
    for row in read.sums:
        s, z, e = row[:, 0], row[:, 1], read.elems
        assert (z <= e).all() and (z <= s).all() and (s <= D * z).all()
    assert (read.sums[0][watched.numpy(), 1] > 0).any()
    rates = read.rates()
    assert np.isnan(rates[:, ~watched.numpy()]).all() and (rates[:, watched.numpy()] >= 0).all()
    # the elements per neuron are what a FiringRecorder forward counts
    fl.detach()
    try:
        s2f.reset_net(r.model)
        with torch.no_grad(), s2f.FiringRecorder(r.model) as rec:
            r.model(r.step.static_in)
            elems = {n: int(m.stats_elems) for n, m in rec.nodes.items()}
    finally:
        fl.attach()
    assert {n: int(e) for n, e in zip(fl.names, fl.elems) if isinstance(fl.nodes[n], s2f.Q_IFNode)} == elems
    fl.clear()


def test_a_dead_layer_is_found(rigs):
    r = rigs("still")
    reset(r)
    fl = r.firing
    bn = dict(r.model.named_modules())[DEAD_BN]
    i = fl.names.index(DEAD_NEURON)
    assert fl.elems[i] > 0
    with torch.no_grad():
        bn.weight.zero_()
        bn.bias.fill_(-10.0)
    try:
        for _ in range(4):
            r.step()
        read = fl.read()
    finally:
        reset(r)
    assert read.first_dead == (2, DEAD_NEURON), read.first_dead
    assert read.silent[i] == 4 and (read.sums[:, i] == 0).all()
    fired = (read.sums[-1, :, 0] > 0)
    assert fired.sum() >= 10 and (read.silent[fired] == 0).all()


def test_the_loop_writes_the_rows_it_read(rigs, tmp_path, caplog):
    import spike2former_amd as s2f
    r = rigs("train")
    reset(r)
    loop = s2f.TrainLoop(r.step, r.opt, r.sched, r.aug, rigs.batches, max_iters=6,
                         hooks=[dict(type="LoggerHook", interval=3, window_size=3)], work_dir=str(tmp_path))
    with caplog.at_level(logging.INFO, logger="spike2former_amd"):
        loop.run()
    read = r.firing.read()
    assert read.count == 6 and len(read.sums) == 6
    with open(tmp_path / "vis_data" / "firing.jsonl") as f:
        lines = [json.loads(line) for line in f]
    with open(tmp_path / "vis_data" / "scalars.json") as f:
        scalars = [json.loads(line) for line in f]
    assert [rec["iter"] for rec in lines] == [3, 6] and [rec["iter"] for rec in scalars] == [3, 6]
    rates, nz, watched = read.rates(), read.nonzero(), read.elems > 0
    for k, (rec, sc) in enumerate(zip(lines, scalars)):
        want, want_nz = rates[3 * k:3 * k + 3].mean(0), nz[3 * k:3 * k + 3].mean(0)
        assert list(rec["rates"]) == [n for n, w in zip(read.names, watched) if w] and rec["rows"] == 3
        for i in np.flatnonzero(watched):
            assert rec["rates"][read.names[i]] == want[i] and rec["nonzero"][read.names[i]] == want_nz[i]
        assert sc["firing/mean"] == float(want[watched].mean()) and sc["firing/min"] == float(want[watched].min())
        assert 0 < sc["firing/mean"] and sc["firing/min_name"] in read.names and np.isfinite(sc["loss"])
    assert not np.array_equal(read.sums[0], read.sums[5])          # the weights and the inputs move: other rows
    assert int(r.firing.counters.ne(0).sum()) == 0
    reset(r)


def test_graphed_step_takes_a_firing_log_too():
    """GraphedStep (the headline loss, one graph) on a model of its own: the row of a replay is the eager forward's counters"""
    import spike2former_amd as s2f
    from spike2former_amd import ops
    from spike2former_amd.graph import GraphedStep
    from spike2former_amd.init_utils import seeded_init
    w = s2f.WORKLOADS["C1_64"]
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C1_64"))).cuda().train()
    s2f.set_keep_membrane(model, False)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(2, 3, w["H"], w["W"], generator=torch.Generator().manual_seed(6)).cuda()
    fl = s2f.FiringLog(model, window=4, patience=2)
    gs = GraphedStep(model, s2f.headline_loss, x, warmup=1, firing=fl)
    try:
        assert fl.attached and fl.read().count == 0 and int((fl.elems > 0).sum()) >= 100
        model.load_state_dict(sd0)
        gs()
        gs()
        read = fl.read()
        assert read.count == 2 and int(fl.counters.ne(0).sum()) == 0
        model.load_state_dict(sd0)
        s2f.reset_net(model)
        with torch.no_grad():
            model(x)
        torch.cuda.synchronize()
        want = ops.read_stats(fl.counters).cpu().numpy()
        assert np.array_equal(read.sums[0], want) and (read.sums[0][:, 1] > 0).any()
        assert (read.sums[:, :, 1] <= read.elems).all()
    finally:
        fl.detach()
        for p in model.parameters():
            p.grad = None
