"""csrc/lsa.hip on the MI355X: `ops.lsa_tables` against the host route, `MaskFormerLoss.match_tables` (scipy's
linear_sum_assignment per decoder layer and image) -- the reference of every assertion here.

  validity    matched queries distinct, matched classes distinct and present, #matched = min(Q, n_present), the two tables agree,
              num_masks equal to the host's exactly;
  optimality  the total of the chosen entries (summed here in fp64) equals scipy's within the rounding of the solvers' fp64 dual
              updates, nr (nr + nc) 2^-52 max|cost| with nr <= nc the oriented sizes: computed from the matrix, no free constant;
  identity    all three tables equal the host's bit for bit.
Families with exact ties (integer costs; one offset per query, whose fp32 entries give exactly tied totals) have several optimal
assignments: validity and optimality are what is REQUIRED of them (test_tied_costs_give_an_equally_optimal_assignment); that the kernel
also resolves ties in scipy's scan order is checked separately (test_ties_are_resolved_in_scipys_scan_order)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L, B = 7, 2
SHAPES = [(10, 20, 3), (10, 20, 10), (10, 20, 16), (100, 150, 1), (100, 150, 10), (100, 150, 40), (100, 150, 100), (100, 150, 150)]
SEEDS = (0, 1, 2)


def _crit(Q, K):
    from spike2former_amd.loss import MaskFormerLoss
    return MaskFormerLoss(K, Q)


def _counts(rng, K, n, batch=B):
    """count_full [batch, 256]: n classes present per image (pixel counts 1 .. 999), plus ignored pixels"""
    count = np.zeros((batch, 256), np.float32)
    for b in range(batch):
        count[b, rng.choice(K, n, replace=False)] = rng.integers(1, 1000, n)
        count[b, 255] = 17
    return count


def _device(cost, count, K, out=None):
    from spike2former_amd import ops
    tgt, rows, num, status = ops.lsa_tables(torch.from_numpy(cost).cuda(), torch.from_numpy(count).cuda(), K, out=out)
    torch.cuda.synchronize()
    return tgt.cpu().numpy(), rows.cpu().numpy(), num.cpu().numpy(), int(status.item())


def _valid_and_optimal(cost, count, K, got, want, skip=()):
    """points 1 and 2 of the module docstring for every (l, b) not in `skip`; -> the largest |total - scipy's total| / bound"""
    tgt, rows, num = got
    wt, wr, wn = want
    nl, nb, Q = tgt.shape
    rows3, wr3 = rows.reshape(nb, nl, Q), wr.reshape(nb, nl, Q)
    worst = 0.0
    for b in range(nb):
        present = np.nonzero(count[b, :K])[0]
        for l in range(nl):
            if (l, b) in skip:
                continue
            r = rows3[b, l]
            matched = np.nonzero(r >= 0)[0]
            assert np.array_equal(np.where(r >= 0, r, K), tgt[l, b]), (l, b)
            assert len(matched) == min(Q, present.size), (l, b, len(matched))
            assert len(set(r[matched].tolist())) == len(matched) and set(r[matched].tolist()) <= set(present.tolist()), (l, b)
            wm = np.nonzero(wr3[b, l] >= 0)[0]
            total = cost[l, b, matched, r[matched]].astype(np.float64).sum()
            ref = cost[l, b, wm, wr3[b, l][wm]].astype(np.float64).sum()
            if present.size:
                nr, nc = sorted((Q, present.size))
                bound = nr * (nr + nc) * 2.0 ** -52 * float(np.abs(cost[l, b][:, present]).max())
                assert abs(total - ref) <= bound, (l, b, total - ref, bound)
                worst = max(worst, abs(total - ref) / bound if bound > 0 else 0.0)
    if not skip:
        assert np.array_equal(num, wn), (num, wn)
    return worst


def _uniform(rng, Q, K, count):
    return rng.random((L, B, Q, K), np.float32) * 22 - 1


def _queries_alike(rng, Q, K, count):
    """every query nearly alike (plausible early in training): the n (n + 1) / 2-scan worst case of the solver at n >= Q"""
    cost = _uniform(rng, Q, K, count)
    for b in range(B):
        present = np.nonzero(count[b, :K])[0]
        n = present.size
        for l in range(L):
            cost[l, b][:, present] = (5 * rng.random(n)[None, :] + 1e-4 * rng.random((Q, n))).astype(np.float32)
    return cost


@pytest.mark.parametrize("family", [_uniform, _queries_alike], ids=["uniform", "queries_alike"])
@pytest.mark.parametrize("Q,K,n", SHAPES)
def test_tables_are_scipys_on_tie_free_costs(Q, K, n, family):
    crit = _crit(Q, K)
    for seed in SEEDS:
        rng = np.random.default_rng(seed)
        count = _counts(rng, K, n)
        cost = family(rng, Q, K, count)
        want = crit.match_tables(cost, count)
        tgt, rows, num, status = _device(cost, count, K)
        assert status == 0
        worst = _valid_and_optimal(cost, count, K, (tgt, rows, num), want)
        print(f"Q {Q} K {K} n {n} seed {seed} {family.__name__}: |total - scipy| / bound = {worst:.3f}")
        assert np.array_equal(tgt, want[0]) and tgt.dtype == want[0].dtype, seed
        assert np.array_equal(rows, want[1]) and rows.dtype == want[1].dtype, seed
        assert np.array_equal(num, want[2]) and num.dtype == want[2].dtype, seed


@pytest.mark.parametrize("family", ["integers", "query_offsets"])
def test_tied_costs_give_an_equally_optimal_assignment(family):
    Q, K = 100, 150
    n = 100 if family == "integers" else 150
    crit = _crit(Q, K)
    for seed in SEEDS:
        rng = np.random.default_rng(seed)
        count = _counts(rng, K, n)
        cost = _uniform(rng, Q, K, count)
        for b in range(B):
            present = np.nonzero(count[b, :K])[0]
            for l in range(L):
                if family == "integers":
                    cost[l, b][:, present] = rng.integers(0, 4, (Q, n)).astype(np.float32)
                else:
                    cost[l, b][:, present] = (5 * rng.random(Q)[:, None] + 1e-4 * rng.random((Q, n))).astype(np.float32)
        want = crit.match_tables(cost, count)
        tgt, rows, num, status = _device(cost, count, K)
        assert status == 0
        _valid_and_optimal(cost, count, K, (tgt, rows, num), want)


def test_ties_are_resolved_in_scipys_scan_order():
    """fp32 costs tie exactly more often than one expects (the "queries alike" family above has tied optima in most problems); among
    equal minima the kernel takes the column scipy's list of unscanned columns yields.  Integer costs and constant matrices, both
    orientations."""
    for Q, K, n in ((100, 150, 100), (100, 150, 150), (100, 150, 40), (10, 20, 16), (10, 20, 3)):
        crit = _crit(Q, K)
        rng = np.random.default_rng(11)
        count = _counts(rng, K, n)
        cost = rng.integers(0, 4, (L, B, Q, K)).astype(np.float32)
        cost[0] = 0.0
        cost[1] = 2.5
        want = crit.match_tables(cost, count)
        tgt, rows, num, status = _device(cost, count, K)
        assert status == 0
        _valid_and_optimal(cost, count, K, (tgt, rows, num), want)
        assert np.array_equal(tgt, want[0]) and np.array_equal(rows, want[1]) and np.array_equal(num, want[2]), (Q, K, n)


def test_image_without_a_class_and_with_one_class():
    Q, K = 10, 20
    crit = _crit(Q, K)
    rng = np.random.default_rng(3)
    count = np.zeros((3, 256), np.float32)
    count[0, 255] = 4096                      # every pixel ignored: nothing to match, the image counts 1 in num_masks
    count[1, 7] = 5                           # one class
    count[2, [0, 19, 4]] = (1, 2, 3)
    cost = rng.random((L, 3, Q, K), np.float32) * 22 - 1
    want = crit.match_tables(cost, count)
    tgt, rows, num, status = _device(cost, count, K)
    assert status == 0
    assert np.array_equal(tgt, want[0]) and np.array_equal(rows, want[1]) and np.array_equal(num, want[2])
    assert (tgt[:, 0] == K).all() and (rows.reshape(3, L, Q)[0] == -1).all() and (num == 1 + 1 + 3).all()
    assert ((rows.reshape(3, L, Q)[1] == 7).sum(-1) == 1).all()


def test_label_outside_the_classes_sets_status_bit_0_and_nan_num_masks():
    Q, K = 10, 20
    rng = np.random.default_rng(4)
    count = _counts(rng, K, 5)
    cost = _uniform(rng, Q, K, count)
    with pytest.raises(ValueError, match="labels >= num_classes"):
        bad = count.copy(); bad[1, 200] = 3
        _crit(Q, K).match_tables(cost, bad)
    for k in (K, 200, 254):
        bad = count.copy(); bad[1, k] = 3
        tgt, rows, num, status = _device(cost, bad, K)
        assert status == 1 and np.isnan(num).all(), (k, status, num)
    assert _device(cost, count, K)[3] == 0          # the ignored label alone (count[:, 255] > 0) is no error


def test_non_finite_costs_set_status_bit_1_and_the_launch_returns():
    """Every loop of the solver is bounded by the problem's sizes and non-finite entries of a present column are found while the tile
    is loaded, before the solver runs (csrc/lsa.hip): the launch returns, the problem is left unmatched, the others are solved."""
    Q, K = 100, 150
    crit = _crit(Q, K)
    rng = np.random.default_rng(5)
    count = _counts(rng, K, 40)
    cost = _uniform(rng, Q, K, count)
    want = crit.match_tables(cost, count)
    # a NaN in an ABSENT column changes nothing
    absent = int(np.nonzero(count[0, :K] == 0)[0][0])
    dirty = cost.copy(); dirty[:, 0, 5, absent] = np.nan
    tgt, rows, num, status = _device(dirty, count, K)
    assert status == 0 and np.array_equal(tgt, want[0]) and np.array_equal(rows, want[1]) and np.array_equal(num, want[2])
    # a NaN and a +Inf in present columns of two problems
    p0, p1 = (int(k) for k in np.nonzero(count[1, :K])[0][:2])
    dirty = cost.copy(); dirty[2, 1, 3, p0] = np.nan; dirty[4, 1, 77, p1] = np.inf
    with pytest.raises(ValueError):
        crit.match_tables(dirty, count)
    tgt, rows, num, status = _device(dirty, count, K)
    assert status == 2
    assert np.isnan(num[[2, 4]]).all() and np.array_equal(num[[0, 1, 3, 5, 6]], want[2][[0, 1, 3, 5, 6]])
    rows3 = rows.reshape(B, L, Q)
    for l in (2, 4):
        assert (tgt[l, 1] == K).all() and (rows3[1, l] == -1).all()
    _valid_and_optimal(cost, count, K, (tgt, rows, num), want, skip={(2, 1), (4, 1)})
    keep = np.ones((L, B), bool); keep[2, 1] = keep[4, 1] = False
    assert np.array_equal(tgt[keep], want[0][keep])


def test_every_output_is_overwritten_and_replays_are_bit_identical():
    Q, K = 100, 150
    crit = _crit(Q, K)
    rng = np.random.default_rng(6)
    count = _counts(rng, K, 40)
    cost = _uniform(rng, Q, K, count)
    want = crit.match_tables(cost, count)
    runs = []
    for fill in (-77, 0x5a5a5a5a):
        out = (torch.full((L, B, Q), fill, dtype=torch.int64, device="cuda"), torch.full((B, L * Q), fill, dtype=torch.int32, device="cuda"),
               torch.full((L,), float("nan") if fill < 0 else 1e30, device="cuda"), torch.full((1,), fill, dtype=torch.int32, device="cuda"))
        runs.append(_device(cost, count, K, out=out))
    for tgt, rows, num, status in runs:
        assert status == 0 and np.array_equal(tgt, want[0]) and np.array_equal(rows, want[1]) and np.array_equal(num, want[2])
    # after a failed launch the same buffers hold a clean result again (the status word is written, not accumulated)
    dirty = cost.copy(); dirty[0, 0, 0, int(np.nonzero(count[0, :K])[0][0])] = -np.inf
    assert _device(dirty, count, K, out=out)[3] == 2
    tgt, rows, num, status = _device(cost, count, K, out=out)
    assert status == 0 and np.array_equal(tgt, want[0]) and np.array_equal(rows, want[1]) and np.array_equal(num, want[2])


def test_cost_tile_in_lds_and_from_l2_agree():
    """Q * n_present above the LDS tile's 15 000 fp64 elements: the same solver re-reads the fp32 costs from L2 (Q = 128, n = 150;
    and the other orientation, Q = 200, n = 100)."""
    for Q, K, n in ((128, 150, 150), (200, 150, 100), (256, 254, 254)):
        crit = _crit(Q, K)
        rng = np.random.default_rng(7)
        count = _counts(rng, K, n)
        cost = rng.random((2, B, Q, K), np.float32) * 22 - 1
        want = crit.match_tables(cost, count)
        tgt, rows, num, status = _device(cost, count, K)
        assert status == 0 and np.array_equal(tgt, want[0]) and np.array_equal(rows, want[1]) and np.array_equal(num, want[2])
