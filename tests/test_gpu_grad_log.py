"""GPU: the gradient log -- s2f_grad_log_partials + s2f_grad_log_rows (csrc/gradlog.hip) through ops.grad_log_append on a synthetic
slot table against the numpy restatement tests/gradlog_ref.py (counts and the maximum exactly, the three sums of squares to the
rounding of an fp64 sum in another order), the ring, the streaks and both latches; then GradLog behind FlatAdamW.step() on the tiny
configuration C1_64, eager and inside GraphedHungarianStep (the rig of tests/step_rig.py, with a grad_log).

The scenario of the kernel tests -- five appends into a ring of three rows, patience 2 -- runs ONCE for the module; what every append
left on the device is kept on the host next to the restatement's state, and the tests read those records."""
import gc
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gradlog_ref as R  # noqa: E402
import step_rig as rig  # noqa: E402

pytestmark = pytest.mark.gpu

# one, two and five spans of 16 384, with and without a tail
SIZES = (1, 3, 4, 5, 255, 1023, 4097, 16384, 16385, 70001)
UNALIGNED, NO_GRAD, ZERO_A, ZERO_B, NEG_MAX, NAN_INF, INF_P, NAN_ONCE = 6, 4, 1, 5, 8, 9, 3, 7
WINDOW, PATIENCE, APPENDS = 3, 2, 5
EPS = 1e-8
GUARD = -0x5A5A5A5A5A5A5A5A


def rtol(numel):
    """every term is an exact fp64 product of fp32 values and none is negative: only the order of the additions differs"""
    return numel * 2.0 ** -53


class Table:
    """a synthetic optimizer: parameters behind a slot table, flat g / m / v of FlatGradAllReduce's layout, hyper and state"""

    def __init__(self, seed=0):
        rng = np.random.default_rng(seed)
        self.n = len(SIZES)
        self.offsets, off = [], 0
        for n in SIZES:
            self.offsets.append(off)
            off += (n + 3) // 4 * 4
        self.total = off
        # the parameters: one a view starting one element into its storage (4-byte aligned only), one holding an inf
        self.p_host = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
        self.p_host[INF_P][2] = np.inf
        self.params = []
        for i, a in enumerate(self.p_host):
            if i == UNALIGNED:
                store = torch.zeros(a.size + 1, device="cuda")
                store[1:].copy_(torch.from_numpy(a))
                self.params.append(store[1:])
            else:
                self.params.append(torch.from_numpy(a).cuda())
        assert self.params[UNALIGNED].data_ptr() % 16 == 4 and all(p.data_ptr() % 16 == 0 for i, p in enumerate(self.params) if i != UNALIGNED)
        self.m_host = self.flat_of([rng.standard_normal(n).astype(np.float32) * 1e-2 for n in SIZES])
        v = [np.square(rng.standard_normal(n).astype(np.float32)) * np.float32(1e-4) for n in SIZES]
        for a in v:
            a[rng.random(a.size) < 0.25] = 0.0          # exact zeros: denom = eps
            a[0] = 0.0
        self.v_host = self.flat_of(v)
        lr = np.full(self.n, 1e-3, np.float32) * (1 + np.arange(self.n, dtype=np.float32))
        lr[NO_GRAD] = -1.0
        self.hyper_host = np.stack([lr, np.full(self.n, 0.005, np.float32)], 1)
        self.bc1, self.bc2s = np.float32(1.0 - 0.9 ** 3), np.float32(np.sqrt(1.0 - 0.999 ** 3))
        self.state_host = np.array([0.5, 2.0, self.bc1, self.bc2s, 3.0, 0, 0, 0], np.float32)
        self.slots = torch.tensor([(p.data_ptr(), off, n) for p, off, n in zip(self.params, self.offsets, SIZES)], dtype=torch.int64).cuda()
        self.hyper, self.state = torch.from_numpy(self.hyper_host).cuda(), torch.from_numpy(self.state_host).cuda()
        self.m, self.v = torch.from_numpy(self.m_host).cuda(), torch.from_numpy(self.v_host).cuda()
        self.g = torch.zeros(self.total, device="cuda")

    def flat_of(self, parts):
        flat = np.zeros(self.total, np.float32)
        for a, off in zip(parts, self.offsets):
            flat[off:off + a.size] = a
        return flat

    def part(self, flat, i):
        return flat[self.offsets[i]:self.offsets[i] + SIZES[i]]

    def gradients(self, it):
        """iteration `it`'s g per parameter: see the scenario in `run`"""
        rng = np.random.default_rng(100 + it)
        g = [rng.standard_normal(n).astype(np.float32) * np.float32(10.0 ** (it - 2)) for n in SIZES]
        for a in g:
            a[rng.random(a.size) < 0.125] = 0.0
        if it != 3:
            g[ZERO_A][:] = 0.0          # all zero in rows 0, 1, 2 and 4
        g[ZERO_B][:] = 0.0              # all zero in every row
        g[NEG_MAX][-1] = -np.float32(1e6)          # its largest |g|, negative, in the one-element tail span
        g[NAN_INF][0], g[NAN_INF][-1] = np.nan, np.inf
        if it == 0:
            g[NAN_ONCE][100] = np.nan
        if it == 1:
            g[0][0] = -np.inf          # a lower index, but a later row than the latch
        return g

    def reference(self, g):
        return [R.row(g[i], self.p_host[i], self.part(self.m_host, i), self.part(self.v_host, i), self.hyper_host[i, 0], self.bc1,
                      self.bc2s, EPS) for i in range(self.n)]


def new_device_state(n, window):
    ring, streak, head = R.new_state(n, window)
    ring[:] = GUARD          # rows no launch has written yet must stay what they were
    return ring, streak, head


@pytest.fixture(scope="module")
def run():
    from spike2former_amd import ops
    t = Table()
    spans = ops.grad_log_table(t.slots)
    assert spans.shape[0] == 7 + 1 + 2 + 5
    partials = torch.zeros(spans.shape[0], 8, dtype=torch.int64, device="cuda")
    ring, streak, head = new_device_state(t.n, WINDOW)
    d_ring, d_streak, d_head = (torch.from_numpy(a.copy()).cuda() for a in (ring, streak, head))
    readonly = [t.m, t.v, t.hyper, t.state, t.slots] + [p if i != UNALIGNED else p._base for i, p in enumerate(t.params)]
    before = [x.clone() for x in readonly]
    records = []
    for it in range(APPENDS):
        g = t.gradients(it)
        g_flat = t.flat_of(g)
        t.g.copy_(torch.from_numpy(g_flat))
        ops.grad_log_append(t.slots, spans, t.hyper, t.state, t.g, t.m, t.v, partials, d_ring, d_streak, d_head, EPS, PATIENCE)
        torch.cuda.synchronize()
        rows = t.reference(g)
        R.append(rows, ring, streak, head, PATIENCE)
        records.append(types.SimpleNamespace(rows=rows, ring=ring.copy(), streak=streak.copy(), head=head.copy(),
                                             d_ring=d_ring.cpu().numpy(), d_streak=d_streak.cpu().numpy(), d_head=d_head.cpu().numpy(),
                                             g_same=bool(torch.equal(t.g.view(torch.int32), torch.from_numpy(g_flat).cuda().view(torch.int32)))))
    same = [bool(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b))
            for a, b in zip(readonly, before)]
    yield types.SimpleNamespace(table=t, spans=spans, records=records, inputs_unchanged=same)
    gc.collect()


def test_counts_and_maximum_are_exact(run):
    for it, rec in enumerate(run.records):
        got = rec.d_ring[it % WINDOW]
        for i, (floats, ints) in enumerate(rec.rows):
            assert got[i, 4:].tolist() == ints.tolist(), (it, i, SIZES[i])
            assert got[i, 3] == np.float64(floats[3]).view(np.int64), (it, i, SIZES[i])
    last = run.records[-1].rows
    assert last[NEG_MAX][0][3] == 1e6 and last[NAN_INF][1][1] == 2 and last[INF_P][1][2] >= 1 and last[ZERO_B][1][0] == SIZES[ZERO_B]
    assert last[NO_GRAD][0][2] == 0.0 and last[UNALIGNED][0][2] > 0.0          # lr < 0: u is 0


def test_sums_of_squares_agree_to_the_rounding_of_the_sum(run):
    worst = {}
    for it, rec in enumerate(run.records):
        got = np.ascontiguousarray(rec.d_ring[it % WINDOW][:, :3]).view(np.float64)
        for i, (floats, _) in enumerate(rec.rows):
            for c in range(3):
                err = abs(got[i, c] - floats[c]) / floats[c] if floats[c] else abs(got[i, c])
                worst[(SIZES[i], c)] = max(worst.get((SIZES[i], c), 0.0), err / rtol(SIZES[i]))
    print("worst error per (numel, column) in units of numel * 2^-53:", {k: round(v, 4) for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if v > 1.0}
    assert not bad, bad


def test_ring_wraps_and_head_counts(run):
    rec = run.records[-1]
    assert rec.d_head[0] == APPENDS and rec.d_head[2] == 0
    for r in (2, 3, 4):          # rows 2-4 survive in a ring of three
        exact = np.array_equal(rec.d_ring[r % WINDOW][:, 3:], rec.ring[r % WINDOW][:, 3:])
        assert exact and np.array_equal(rec.d_ring[r % WINDOW][:, 3:], run.records[r].ring[r % WINDOW][:, 3:]), r
        # the sums: the bits the launch of row r wrote are still there
        assert np.array_equal(rec.d_ring[r % WINDOW], run.records[r].d_ring[r % WINDOW]), r
    first = run.records[0]
    assert (first.d_ring[1:] == GUARD).all() and [int(x.d_head[0]) for x in run.records] == [1, 2, 3, 4, 5]


def test_streaks_and_the_stalled_latch(run):
    for it, rec in enumerate(run.records):
        assert np.array_equal(rec.d_streak, rec.streak), it
        assert rec.d_head[1] == rec.head[1] and rec.d_head[3] == rec.head[3], it
    assert R.event(run.records[0].d_head[1]) is None
    # ZERO_A and ZERO_B both reach the patience in row 1: the lower index holds the latch, and keeps it
    assert all(R.event(rec.d_head[1]) == (1, ZERO_A) for rec in run.records[1:])
    assert [int(rec.d_streak[ZERO_A, 0]) for rec in run.records] == [1, 2, 3, 0, 1]          # back to 0 when g is non-zero
    assert [int(rec.d_streak[ZERO_B, 0]) for rec in run.records] == [1, 2, 3, 4, 5]


def test_the_nonfinite_latch_holds_the_first_row_and_the_lowest_index(run):
    # row 0: NAN_ONCE (7) and NAN_INF (9); row 1: parameter 0 as well
    assert all(R.event(rec.d_head[3]) == (0, NAN_ONCE) for rec in run.records)
    assert [int(rec.d_streak[NAN_INF, 1]) for rec in run.records] == [1, 2, 3, 4, 5]
    assert [int(rec.d_streak[NAN_ONCE, 1]) for rec in run.records] == [1, 0, 0, 0, 0]
    assert [int(rec.d_streak[0, 1]) for rec in run.records] == [0, 1, 0, 0, 0]


def test_an_append_only_reads_its_inputs(run):
    assert all(run.inputs_unchanged) and all(rec.g_same for rec in run.records)


def test_two_appends_over_the_same_inputs_write_the_same_bits(run):
    from spike2former_amd import ops
    t = run.table
    partials = torch.zeros(run.spans.shape[0], 8, dtype=torch.int64, device="cuda")
    ring, streak, head = (torch.from_numpy(a).cuda() for a in new_device_state(t.n, 2))
    for _ in range(2):
        ops.grad_log_append(t.slots, run.spans, t.hyper, t.state, t.g, t.m, t.v, partials, ring, streak, head, EPS, PATIENCE)
    torch.cuda.synchronize()
    assert torch.equal(ring[0], ring[1]) and int(head[0]) == 2 and not bool((ring == GUARD).any())
    assert np.array_equal(ring[0].cpu().numpy(), run.records[-1].d_ring[(APPENDS - 1) % WINDOW])          # and those of the scenario's last row


# ---------------------------------------------------------------------------------------------------- the tiny model
def tiny(grad_log):
    import spike2former_amd as s2f
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.init_utils import seeded_init
    from spike2former_amd.train import FlatAdamW
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C1_64"))).cuda().train()
    red = FlatGradAllReduce(model.parameters(), 1)
    opt = FlatAdamW(model, red, lr=0.001, weight_decay=0.005, clip_grad=rig.CLIP, grad_log=grad_log, paramwise_cfg=rig.PARAMWISE)
    return model, red, opt


def test_eager_step_with_the_log_is_the_step_without_it():
    import spike2former_amd as s2f
    plain, logged = tiny(None), tiny(dict(window=4, patience=2))
    assert plain[2].grad_log is None and isinstance(logged[2].grad_log, s2f.GradLog)
    gen = torch.Generator(device="cuda").manual_seed(9)
    grads = [torch.randn(p.shape, device="cuda", generator=gen) * 1e-2 for p in plain[0].parameters()]
    for model, red, opt in (plain, logged):
        for p, g in zip(model.parameters(), grads):
            p.grad = g.clone()
        red.gather()
        opt.step()
    torch.cuda.synchronize()
    for (name, p), q in zip(plain[0].named_parameters(), logged[0].parameters()):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)), name
    assert torch.equal(plain[2].exp_avg.view(torch.int32), logged[2].exp_avg.view(torch.int32))
    assert torch.equal(plain[2].exp_avg_sq.view(torch.int32), logged[2].exp_avg_sq.view(torch.int32))
    assert torch.equal(plain[2].state, logged[2].state)
    model, red, opt = logged
    read = opt.grad_log.read()
    assert read.count == 1 and read.cols.shape == (1, len(opt.params), 8) and read.names == [g["name"] for g in opt.param_groups]
    assert read.first_nonfinite is None and read.first_stalled is None
    for i, (p, off) in enumerate(zip(opt.params, red.offsets)):
        n = p.numel()
        want = red.flat[off:off + n].double().pow(2).sum().item()
        assert abs(read.grad_sq[0, i] - want) <= rtol(n) * want, (read.names[i], n)
        assert read.numel[0, i] == n
        assert abs(read.weight_sq[0, i] - p.detach().double().pow(2).sum().item()) <= rtol(n) * read.weight_sq[0, i]
    norm = float(opt.grad_norm)
    print("total_grad_norm", read.total_grad_norm[0], "optimizer.grad_norm", norm)
    assert abs(read.total_grad_norm[0] - norm) <= 1e-5 * norm
    assert opt.grad_log.read().cols.shape[0] == 0          # the rows since the last read
    for m in (plain[0], logged[0]):
        for p in m.parameters():
            p.grad = None


def test_the_log_follows_a_rebuilt_optimizer():
    """FlatGradAllReduce.compact() moves a parameter behind the others and FlatAdamW.rebuild() re-lays its tables: the log's span table
    and names follow, and its rows start afresh"""
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.train import FlatAdamW
    torch.manual_seed(2)
    m = torch.nn.ModuleDict({"a": torch.nn.Linear(37, 19), "big": torch.nn.Linear(130, 127, bias=False), "c": torch.nn.Linear(5, 3)}).cuda()
    red = FlatGradAllReduce(m.parameters(), 1)
    opt = FlatAdamW(m, red, clip_grad=dict(max_norm=0.01), grad_log=True)
    log = opt.grad_log

    def one_step(skip=None):
        for name, p in m.named_parameters():
            p.grad = None if name == skip else torch.randn_like(p)
        red.gather()
        opt.step()
    one_step()
    first = log.read()
    assert first.count == 1 and first.names == [n for n, _ in m.named_parameters()] and log.spans.shape[0] == 6
    one_step(skip="big.weight")          # as if its gradient had arrived through a sink
    red.compact()
    opt.rebuild()
    assert log.names == [g["name"] for g in opt.param_groups] and log.names[-1] == "big.weight" and log.names != first.names
    assert log.read().count == 0 and log.spans[:, 0].tolist() == [0, 1, 2, 3, 4, 4]
    one_step()
    read = log.read()
    assert read.count == 1 and read.names == log.names
    for i, (p, off) in enumerate(zip(opt.params, red.offsets)):
        want = red.flat[off:off + p.numel()].double().pow(2).sum().item()
        assert abs(read.grad_sq[0, i] - want) <= rtol(p.numel()) * want and read.numel[0, i] == p.numel()
    for p in m.parameters():
        p.grad = None


def test_rows_of_the_captured_step_match_the_train_log():
    r = rig.build(grad_log=dict(window=8, patience=3))
    model, opt, log, step = r.model, r.opt, r.log, r.step
    assert step.grad_log is opt.grad_log and step.grad_log.read().count == 0          # the capture's passes are not row 0
    batches = rig.make_batches(r.K)
    for it in range(3):          # (nobody steps the schedule: the rate stays the warm-up's first)
        rig.feed(r, batches[it])
        step()
    step.check()
    read, rows = step.grad_log.read(), log.read()
    assert read.count == 3 and rows.count == 3 and read.cols.shape[0] == 3
    want = rows.rows[:, rows.names.index("grad_norm")].astype(np.float64)
    print("total_grad_norm", read.total_grad_norm.tolist(), "TrainLog grad_norm", want.tolist())
    assert np.isfinite(want).all() and (want > 0).all()
    assert (np.abs(read.total_grad_norm - want) <= 1e-5 * want).all()
    assert (read.numel[0] == np.array([p.numel() for p in opt.params])).all()
    for p in model.parameters():
        p.grad = None
    del step, r
    gc.collect()
