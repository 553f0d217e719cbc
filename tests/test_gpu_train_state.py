"""GPU, kernel level: s2f_state_copy and s2f_train_log_append (csrc/trainstate.hip) through ops.state_copy / ops.train_log_append
against plain indexing on host copies.  Bit equality everywhere."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD, GUARD2 = 0x5A5A5A5A, 0x3C3C3C3C
# (first word in the shared storage, words): 4-, 12-, 8-, 4- and 0-byte offsets from a 16-byte boundary, guard words between them
CARVED = ((1, 3), (7, 5), (18, 4095), (4117, 4097), (8216, 8193))
STORE = 16420


def bits(t):
    return t.detach().reshape(-1).view(torch.int32)


def table_tensors(fill=None, seed=0):
    """One table: lengths 1, 2, 3, 4, 5, 4095, 4096, 4097, 8193 words; fp32 and int64; five tensors carved out of one storage.
    Random BITS (NaN payloads, denormals, infinities among them), or the word `fill` everywhere.  -> (tensors, storage)"""
    g = torch.Generator().manual_seed(seed)

    def words(n):
        if fill is not None:
            return torch.full((n,), fill, dtype=torch.int32)
        return torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    store = words(STORE).cuda().view(torch.float32)
    assert store.data_ptr() % 16 == 0
    alone = {1: torch.float32, 2: torch.int64, 4: torch.int64, 4096: torch.int64}
    own = {n: words(n).cuda().view(dt) for n, dt in alone.items()}
    c = [store[a:a + n] for a, n in CARVED]
    tensors = [own[1], own[2], c[0], own[4], c[1], c[2], own[4096].view(64, 32), c[3], c[4]]
    assert [bits(t).numel() for t in tensors] == [1, 2, 3, 4, 5, 4095, 4096, 4097, 8193]
    assert [t.data_ptr() % 16 for t in c] == [4, 12, 8, 4, 0]
    if fill is None:          # the special values are there whatever the generator drew
        own[1].view(torch.int32)[0] = 0x7FC12345          # a NaN with a payload
        c[0].view(torch.int32)[:3] = torch.tensor([1, -(2 ** 31) + 5, 0x7F800000], dtype=torch.int32).cuda()          # denormals, +inf
    return tensors, store


def outside(store):
    keep = torch.ones(STORE, dtype=torch.bool)
    for a, n in CARVED:
        keep[a:a + n] = False
    return bits(store).cpu()[keep]


def test_state_copy_packs_and_unpacks_bits():
    from spike2former_amd import ops
    src, _ = table_tensors(seed=1)
    slots, chunks, words = ops.state_table(src)
    assert chunks.shape[0] == 7 + 2 + 3 and words % 4 == 0
    tail = 64
    flat = torch.full((words + tail,), GUARD, dtype=torch.int32, device="cuda")
    want = flat.cpu().clone()
    for t, (_, off, n) in zip(src, slots.tolist()):
        want[off:off + n] = bits(t).cpu()
    assert int((want == GUARD).sum()) >= tail + 3 + 2 + 1 + 3 + 1          # pads between the slots and the words behind the last
    ops.state_copy(src, slots, chunks, flat)
    assert torch.equal(flat.cpu(), want)          # slots = the cat of the bit views; every pad word still the guard
    # back, into guarded tensors of the same layout in ANOTHER storage
    dst, store = table_tensors(fill=GUARD2)
    dslots, dchunks, dwords = ops.state_table(dst)
    assert dwords == words and dslots[:, 1:].tolist() == slots[:, 1:].tolist()
    ops.state_copy(dst, dslots, dchunks, flat, to_params=True)
    for a, b in zip(dst, src):
        assert a.dtype == b.dtype and torch.equal(bits(a), bits(b))          # NaN payloads and denormals included: bits
    assert bool((outside(store) == GUARD2).all())          # the neighbours inside the shared storage
    assert torch.equal(flat.cpu(), want)


def test_state_copy_under_capture():
    from spike2former_amd import ops
    src, _ = table_tensors(seed=2)
    dst, store = table_tensors(fill=GUARD2)
    slots, chunks, words = ops.state_table(src)
    dslots, dchunks, _ = ops.state_table(dst)
    flat = torch.full((words,), GUARD, dtype=torch.int32, device="cuda")
    ops.state_copy(src, slots, chunks, flat)          # (the module is loaded before the capture)
    flat.fill_(GUARD)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.state_copy(src, slots, chunks, flat)
        ops.state_copy(dst, dslots, dchunks, flat, to_params=True)
    for replay in range(2):
        for t in src:
            bits(t).add_(replay + 1)          # other values for each replay
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(dst, src):
            assert torch.equal(bits(a), bits(b)), replay
        assert bool((outside(store) == GUARD2).all())


@pytest.mark.parametrize("n,window", list(itertools.product((1, 63, 64, 65, 256), (1, 2, 10))))
def test_train_log_append_wraps(n, window):
    from spike2former_amd import ops
    stride = n + 3
    vals = torch.zeros(n, device="cuda")
    srcs = [vals[i] for i in range(n)]
    table = ops.train_log_table(srcs)
    ring = torch.full((window, stride), -7.0, device="cuda")
    head = torch.tensor([0, -1], dtype=torch.int64, device="cuda")
    rows = []
    for it in range(window + 3):
        rows.append(torch.arange(n, dtype=torch.float32) * 0.5 + 1000.0 * it)
        vals.copy_(rows[-1])
        ops.train_log_append(srcs, ring, head, table=table)
    got, h = ring.cpu(), head.cpu().tolist()
    assert h == [window + 3, -1]
    for it in range(3, window + 3):          # the last `window` rows, each where its index says
        assert torch.equal(got[it % window, :n], rows[it])
    assert bool((got[:, n:] == -7.0).all())          # the slack of every row


@pytest.mark.parametrize("order", list(itertools.permutations((0, 64, 255))))
def test_train_log_append_latches_the_first_non_finite_row(order):
    from spike2former_amd import ops
    n, window = 256, 2
    vals = torch.zeros(n, device="cuda")
    srcs = [vals[i] for i in range(n)]
    table = ops.train_log_table(srcs)
    ring = torch.zeros(window, n, device="cuda")
    head = torch.tensor([0, -1], dtype=torch.int64, device="cuda")
    at = dict(zip((3, 5, 8), order))          # iteration -> the lane that holds a non-finite value in it (and only in it)
    seen = []
    for it in range(12):
        vals.fill_(float(it))
        if it in at:
            vals[at[it]] = float("inf") if it != 5 else float("nan")
        ops.train_log_append(srcs, ring, head, table=table)
        seen.append(head.cpu().tolist())
    assert seen == [[it + 1, -1 if it < 3 else 3] for it in range(12)]          # the FIRST, still there after five wraps


def test_train_log_append_under_capture():
    from spike2former_amd import ops
    n, window = 65, 10
    vals = torch.zeros(n, device="cuda")
    srcs = [vals[i] for i in range(n)]
    table = ops.train_log_table(srcs)
    ring = torch.zeros(window, n, device="cuda")
    head = torch.tensor([0, -1], dtype=torch.int64, device="cuda")
    ops.train_log_append(srcs, ring, head, table=table)          # row 0, eagerly
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.train_log_append(None, ring, head, table=table, n=n)
    rows = [torch.zeros(n)]
    for replay in range(5):
        rows.append(torch.arange(n, dtype=torch.float32) + 100.0 * (replay + 1))
        vals.copy_(rows[-1])
        graph.replay()
    got = ring.cpu()
    assert head.cpu().tolist() == [6, -1]
    for i, r in enumerate(rows):
        assert torch.equal(got[i], r)
    assert len({tuple(got[i].tolist()) for i in range(1, 6)}) == 5
