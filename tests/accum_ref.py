"""numpy restatement of gradient accumulation (csrc/optim.hip: s2f_grad_accumulate, s2f_grad_accum_stats; train.GradAccum.plan;
runner.noise_scale) -- the oracle of tests/test_grad_accum_host.py and tests/test_gpu_grad_accum.py.  Every float32 operation
below is ONE rounding (numpy does not contract), every sum runs in the kernels' fixed order, so the results are compared by bits."""
import numpy as np

RUN = 16384          # elements per workgroup of s2f_grad_sqnorm / s2f_grad_accumulate: 256 threads x 16 float4
THREADS = 256


def parts(n):
    return 0 if n <= 0 else (n + RUN - 1) // RUN


def accumulate(g, acc, scale):
    """out = fl(acc + fl(scale * g)), or fl(scale * g) with acc None: two fp32 roundings"""
    g = np.asarray(g, np.float32)
    with np.errstate(all="ignore"):
        r = np.float32(scale) * g
        return r if acc is None else np.asarray(acc, np.float32) + r


def _tree(red):
    """the 256-wide fp64 tree over the last axis: red[t] += red[t + s] for s = 128, 64 .. 1"""
    red = red.copy()
    s = THREADS // 2
    while s > 0:
        red[..., :s] = red[..., :s] + red[..., s:2 * s]
        s //= 2
    return red[..., 0]


def sq_partials(g):
    """what s2f_grad_sqnorm writes: per run of 16 384 elements, thread t adds the squares of its 16 groups of four (group i at
    element (i * 256 + t) * 4 of the run) into ONE fp32 accumulator in element order, then the fp64 tree.  Elements past the end
    contribute nothing (here: zeros, x + 0 = x for the non-negative or NaN accumulator)."""
    g = np.asarray(g, np.float32)
    nb = parts(g.size)
    pad = np.zeros(nb * RUN, np.float32)
    pad[:g.size] = g
    per_thread = pad.reshape(nb, 16, THREADS, 4).transpose(0, 2, 1, 3).reshape(nb, THREADS, 64)
    with np.errstate(all="ignore"):
        sq = per_thread * per_thread
        acc = np.zeros((nb, THREADS), np.float32)
        for j in range(64):
            acc = acc + sq[:, :, j]
        return _tree(acc.astype(np.float64))


def ordered_sum(p):
    """s2f_adamw_prepare's fixed order: thread t owns the contiguous run of ceil(n / 256) partials, then the 256-wide tree"""
    p = np.asarray(p, np.float64)
    per = (p.size + THREADS - 1) // THREADS
    pad = np.zeros(THREADS * per, np.float64)
    pad[:p.size] = p
    runs = pad.reshape(THREADS, per)
    a = np.zeros(THREADS, np.float64)
    with np.errstate(all="ignore"):
        for k in range(per):
            a = a + runs[:, k]
        return float(_tree(a))


def stats(micro, accum_parts):
    """s2f_grad_accum_stats: micro [rows][nparts] -> fp32 {sum of row sums / rows, sum of accum_parts, rows, 0}"""
    micro = np.asarray(micro, np.float64)
    m = 0.0
    for row in micro:
        m = m + ordered_sum(row)
    return np.array([m / float(len(micro)), ordered_sum(accum_parts), float(len(micro)), 0.0]).astype(np.float32)


def plan(i, counts, total=None):
    """mmengine's rule, stated by brute force: the iterations 0 .. total - 1 are cut into groups of `counts` from iteration 0, the
    last group is what is left; a group's micro-batch gradients are averaged (scale 1 / its length), it opens at its first and
    updates at its last iteration.  -> (scale, first, last)"""
    if total is None:
        group = list(range(i - i % counts, i - i % counts + counts))
    else:
        groups = [list(range(lo, min(lo + counts, total))) for lo in range(0, total, counts)]
        group = next(g for g in groups if i in g)
    return 1.0 / len(group), i == group[0], i == group[-1]


def noise_scale(m, M, small, big):
    """-> (S / G2 or None, G2, S); m, M: mean |g|^2 at the batch sizes small, big"""
    g2 = (big * M - small * m) / (big - small)
    s = (m - M) / (1.0 / small - 1.0 / big)
    return (s / g2 if g2 > 0 else None), g2, s
