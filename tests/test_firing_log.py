"""CPU: the firing log without a GPU -- the ABI row and its argument errors, the torch route of ops.firing_log_append against the
numpy restatement (tests/firing_ref.py), FiringLog over a toy tree of Q_IFNodes whose counters the test fills by hand, and
LoggerHook's firing keys, firing.jsonl and its one warning, driven by a fake step (runner.py)."""
import json
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import firing_ref as R  # noqa: E402

P = 1 << 20          # a 16-byte aligned dummy address: never dereferenced on the host
SLOTS = 256


# ---------------------------------------------------------------------------------------------------- ABI
def test_abi_row_and_argument_errors():
    from spike2former_amd import _lib, ops
    lib = _lib.lib
    assert lib.s2f_version() >= 45 and len(_lib.SIGNATURES["s2f_firing_log_append"][1]) == 8 and ops.STAT_SLOTS == SLOTS
    call = lib.s2f_firing_log_append
    for k in (0, 2, 4, 6):
        args = [P, 3, P, 2, P, 1, P, None]
        args[k] = None
        assert call(*args) == -1 and b"null" in lib.s2f_last_error()
    for n in (0, -2):
        assert call(P, n, P, 2, P, 1, P, None) == -1 and b"n " in lib.s2f_last_error()
    assert call(P, 3, P, 0, P, 1, P, None) == -1 and b"window" in lib.s2f_last_error()
    assert call(P, 3, P, 2, P, 0, P, None) == -1 and b"patience" in lib.s2f_last_error()
    assert call(P + 8, 3, P, 2, P, 1, P, None) == -2 and call(P, 3, P + 4, 2, P, 1, P, None) == -2
    assert call(P, 3, P, 2, P + 2, 1, P, None) == -2 and call(P, 3, P, 2, P, 1, P + 4, None) == -2


# ---------------------------------------------------------------------------------------------------- the op's CPU route
def fresh_counters(rng, n, it):
    """int64 [n, SLOTS, 2]: neuron i of iteration `it` is silent for three iterations in every five; big single-slot values among them"""
    c = np.zeros((n, SLOTS, 2), np.int64)
    for i in range(n):
        if (i + it) % 5 < 3:
            continue
        kind = (i + 2 * it) % 3
        slots = [0] if kind == 0 else [SLOTS - 1] if kind == 1 else list(range(SLOTS))
        c[i, slots, 1] = rng.integers(1, 1 << 20, len(slots))
        c[i, slots, 0] = c[i, slots, 1] * rng.integers(1, 9, len(slots))
        if i % 4 == 1:
            c[i, slots[0]] += [(1 << 33) + (1 << 32) - 1, 1 << 33]
    return c


def test_cpu_route_matches_the_restatement():
    from spike2former_amd import ops
    rng = np.random.default_rng(7)
    for n, patience in ((1, 1), (5, 2), (65, 3)):
        window = 3
        start = np.where(np.arange(n) % 5 == 4, -1, 0)
        ring, silent, head = R.new_state(n, window, start)
        t_ring, t_silent, t_head = (torch.from_numpy(a.copy()) for a in (ring, silent, head))
        for it in range(7):
            c = fresh_counters(rng, n, it)
            t_c = torch.from_numpy(c.copy())
            R.append(c, ring, silent, head, patience)
            ops.firing_log_append(t_c, t_ring, t_silent, t_head, patience)
            assert int(t_c.abs().sum()) == 0
            assert np.array_equal(t_ring.numpy(), ring) and np.array_equal(t_silent.numpy(), silent)
            assert t_head.tolist() == head.tolist() and t_head.tolist()[0] == it + 1
        assert bool((t_silent[torch.from_numpy(start) == -1] == -1).all())
        assert R.first_dead(head) is not None
    with pytest.raises(ValueError):
        ops.firing_log_append(torch.zeros(2, SLOTS, 2, dtype=torch.int64), torch.zeros(3, 3, 2, dtype=torch.int64),
                              torch.zeros(2, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), 1)
    with pytest.raises(ValueError):
        ops.firing_log_append(torch.zeros(2, SLOTS, 2, dtype=torch.int64), torch.zeros(3, 2, 2, dtype=torch.int64),
                              torch.zeros(2, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), 0)


def test_restatement_latches_the_lowest_neuron_of_the_earliest_row():
    ring, silent, head = R.new_state(4, 2, [0, -1, 0, 0])
    fired = np.zeros((4, SLOTS, 2), np.int64)
    fired[:, 3] = [16, 2]
    quiet = fired.copy()
    quiet[[1, 2, 3]] = 0
    R.append(quiet.copy(), ring, silent, head, 2)
    assert R.first_dead(head) is None and silent.tolist() == [0, -1, 1, 1]
    R.append(quiet.copy(), ring, silent, head, 2)
    assert R.first_dead(head) == (1, 2) and silent.tolist() == [0, -1, 2, 2]          # neurons 2 and 3 in one row: the lower one
    quiet[0] = 0
    for _ in range(2):
        R.append(quiet.copy(), ring, silent, head, 2)
    assert R.first_dead(head) == (1, 2) and silent.tolist() == [2, -1, 4, 4] and head[0] == 4          # neuron 0's event is later
    R.append(fired.copy(), ring, silent, head, 2)
    assert silent.tolist() == [0, -1, 0, 0] and ring[0, :, 0].tolist() == [16, 16, 16, 16]          # (every neuron's row is written)


# ---------------------------------------------------------------------------------------------------- FiringLog on a toy tree
def toy():
    import spike2former_amd as s2f

    class Block(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lif1, self.lin, self.lif2 = s2f.Q_IFNode(), torch.nn.Linear(2, 2), s2f.LIFNode()

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.stem, self.a, self.b = s2f.Q_IFNode(surrogate_function=s2f.Quant(D=4)), Block(), Block()
    return Toy()


ELEMS = {"stem": 40, "a.lif1": 10, "a.lif2": 0, "b.lif1": 30, "b.lif2": 20}


def fake_forward(model, fl, sums):
    """what a forward does to the counters: every neuron adds its {sum, nonzero} into two slots, and counts its elements"""
    def run():
        for (name, m), (s, z) in zip(fl.nodes.items(), sums):
            if ELEMS[name]:
                m.stats_elems += ELEMS[name]
                m.stats[5, 0] += s // 2
                m.stats[200, 0] += s - s // 2
                m.stats[7, 1] += z
    return run


def test_firing_log_attach_read_rates_and_wrap():
    import spike2former_amd as s2f
    model = toy()
    fl = s2f.FiringLog(model, window=3, patience=2, device="cpu")
    assert fl.names == list(ELEMS) and fl.counters.shape == (5, SLOTS, 2)
    assert fl.head.data_ptr() == fl._buf.data_ptr() and fl.ring.data_ptr() == fl._buf.data_ptr() + 8 * (4 + 3)
    with pytest.raises(RuntimeError):
        fl.measure(lambda: None)          # before attach
    fl.attach()
    for i, m in enumerate(fl.nodes.values()):
        assert m.stats.data_ptr() == fl.counters[i].data_ptr() and m.stats.shape == (SLOTS, 2)
    other = s2f.FiringLog(model, device="cpu")
    with pytest.raises(RuntimeError, match="already record"):
        other.attach()
    with pytest.raises(RuntimeError, match="already record"):          # ... and the reverse: a recorder's counters are in place
        fl.detach()
        with s2f.FiringRecorder(model):
            fl.attach()
    assert all(m.stats is None for m in fl.nodes.values())
    fl.attach()
    fl.measure(fake_forward(model, fl, [(8, 4)] * 5))
    assert fl.elems.tolist() == list(ELEMS.values()) and fl.silent.tolist() == [0, 0, -1, 0, 0]
    fl.clear()
    assert int(fl.counters.abs().sum()) == 0 and fl.head.tolist() == [0, -1, 0, 0] and fl.silent.tolist() == [0, 0, -1, 0, 0]
    empty = fl.read()
    assert empty.sums.shape == (0, 5, 2) and empty.count == 0 and empty.first_dead is None and empty.rates().shape == (0, 5)
    rows = [[(40, 20), (10, 5), (0, 0), (0, 0), (160, 20)],
            [(80, 40), (0, 0), (0, 0), (0, 0), (20, 20)],
            [(4, 4), (3, 3), (0, 0), (60, 30), (1, 1)],
            [(8, 8), (6, 6), (0, 0), (0, 0), (2, 2)]]
    for k, row in enumerate(rows):
        fake_forward(model, fl, row)()
        fl.append()
        read = fl.read()
        assert read.count == k + 1 and read.sums.shape == (min(k + 1, 3), 5, 2) and read.sums.dtype == np.int64
        assert read.sums[-1].tolist() == [list(p) for p in row]
    assert read.names == list(ELEMS) and read.elems.tolist() == list(ELEMS.values())
    assert read.sums[:, :, 0].tolist() == [[r[i][0] for i in range(5)] for r in rows[1:]]          # the window wrapped: oldest first
    assert read.first_dead == (1, "b.lif1") and read.silent.tolist() == [0, 0, -1, 1, 0]
    rates, nz = read.rates(), read.nonzero()
    assert rates.shape == nz.shape == (3, 5) and np.isnan(rates[:, 2]).all() and np.isnan(nz[:, 2]).all()
    assert rates[0, 0] == 80 / 40 * 8 / 4 and rates[2, 1] == 6 / 10 * 8 / 8 and rates[1, 3] == 60 / 30 and rates[0, 4] == 20 / 20
    assert nz[0, 0] == 1.0 and nz[2, 1] == 0.6 and nz[1, 3] == 1.0 and nz[0, 3] == 0.0
    fl.detach()
    assert all(m.stats is None for m in fl.nodes.values())


# ---------------------------------------------------------------------------------------------------- LoggerHook
class FakeAugment:
    rng = np.random.default_rng(0)

    def __call__(self, images, segs, out=None):
        pass


class FakeStep:
    """what the loop sees of a captured step with a TrainLog and a FiringLog: one scripted row into each per call"""

    def __init__(self, model, log, firing, script):
        self.model, self.log, self.firing, self.script, self.calls = model, log, firing, script, 0
        self.static_in, self.static_seg = torch.zeros(1), torch.zeros(1, dtype=torch.uint8)
        self.vals = {k: torch.zeros(()) for k in ("loss", "grad_norm", "clip_coef")}
        log.bind(self.vals)
        firing.attach()
        firing.measure(fake_forward(model, firing, [(8, 4)] * 5))
        firing.clear()

    def __call__(self):
        self.vals["loss"].fill_(1.0 + self.calls)
        fake_forward(self.model, self.firing, self.script[self.calls])()
        self.log.append()
        self.firing.append()
        self.calls += 1


def make_loop(tmp_path, script, interval, window=4, patience=3, **kw):
    import spike2former_amd as s2f
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.train import FlatAdamW, LinearThenPoly
    model = toy()
    opt = FlatAdamW(model, FlatGradAllReduce(model.parameters(), 1), lr=0.01)
    sched = LinearThenPoly(opt, warmup=2, total=50, start_factor=0.1)
    step = FakeStep(model, s2f.TrainLog(window=8, device="cpu", capacity=4),
                    s2f.FiringLog(model, window=window, patience=patience, device="cpu"), script)
    return s2f.TrainLoop(step, opt, sched, FakeAugment(), [(None, None)], max_iters=len(script),
                         hooks=[dict(type="LoggerHook", interval=interval, window_size=2)], work_dir=str(tmp_path), **kw)


def test_logger_hook_firing_keys_lines_and_one_warning(tmp_path, caplog):
    # stem always fires; a.lif1 stops after iteration 2 (silent 3 at iteration 5, row 4); b.lif1 is the quietest that fires
    script = [[(40 + 4 * it, 20), (10 if it < 2 else 0, 5 if it < 2 else 0), (0, 0), (3, 3), (20 + it, 10)] for it in range(10)]
    loop = make_loop(tmp_path, script, interval=4)
    with caplog.at_level(logging.INFO, logger="spike2former_amd"):
        loop.run()
    with open(tmp_path / "vis_data" / "scalars.json") as f:
        lines = [json.loads(line) for line in f]
    with open(tmp_path / "vis_data" / "firing.jsonl") as f:
        firing = [json.loads(line) for line in f]
    assert [r["iter"] for r in lines] == [4, 8, 10] and [r["iter"] for r in firing] == [4, 8, 10]
    assert [r["rows"] for r in firing] == [4, 4, 2]
    elems = np.array(list(ELEMS.values()), float)
    scale = np.array([8 / 4, 1, 1, 1, 1], float)
    watched = [0, 1, 3, 4]
    first = 0
    for rec, fr in zip(lines, firing):
        rows = np.array([[p[0] for p in script[it]] for it in range(first, rec["iter"])], float)
        nzs = np.array([[p[1] for p in script[it]] for it in range(first, rec["iter"])], float)
        first = rec["iter"]
        with np.errstate(invalid="ignore"):
            want = (rows / elems * scale).mean(0)
            want_nz = (nzs / elems).mean(0)
        assert set(rec) >= {"firing/mean", "firing/min", "firing/min_name", "firing/silent", "loss", "lr", "iter"}
        assert list(fr["rates"]) == [n for n in ELEMS if ELEMS[n]] and list(fr["nonzero"]) == list(fr["rates"])
        names = list(ELEMS)
        for i in watched:
            assert fr["rates"][names[i]] == pytest.approx(want[i], rel=1e-12)
            assert fr["nonzero"][names[i]] == pytest.approx(want_nz[i], rel=1e-12)
        assert rec["firing/mean"] == pytest.approx(want[watched].mean(), rel=1e-12)
        low = watched[int(np.argmin(want[watched]))]
        assert rec["firing/min"] == pytest.approx(want[low], rel=1e-12) and rec["firing/min_name"] == names[low]
    assert [r["firing/silent"] for r in lines] == [1, 1, 1] and lines[-1]["firing/min_name"] == "a.lif1"
    warnings = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1 and "a.lif1" in warnings[0].message and "iteration 5" in warnings[0].message
    assert sum("Iter(train)" in r.message and "firing/mean" in r.message for r in caplog.records) == 3


def test_logger_hook_refuses_a_ring_shorter_than_the_interval(tmp_path):
    loop = make_loop(tmp_path, [[(1, 1)] * 5] * 6, interval=5, window=4)
    with pytest.raises(ValueError, match="FiringLog of 4 rows"):
        loop.run()


def test_validation_does_not_count_into_the_next_row(tmp_path):
    seen = []

    def validate():          # a validation forward must find no counters on the neurons ...
        seen.append([m.stats is None for m in loop.firing.nodes.values()])
        return {}
    loop = make_loop(tmp_path, [[(4, 2)] * 5] * 4, interval=2, val_interval=2, validate=validate)
    loop.run()
    assert seen == [[True] * 5] * 2 and loop.firing.attached          # ... and training goes on with the same ones
    assert all(m.stats.data_ptr() == loop.firing.counters[i].data_ptr() for i, m in enumerate(loop.firing.nodes.values()))
    assert loop.firing.read().sums[:, 0].tolist() == [[4, 2]] * 4
