"""numpy restatement of the gradient log (csrc/gradlog.hip, include/s2f.h "gradient log"): one parameter's row from its g, p, m, v, and
the ring / streak / head bookkeeping of one append.  u is formed in float32 with the kernel's expressions in their order (every numpy
float32 operation rounds once, as the kernel's under `fp contract(off)`); the three sums of squares are exact fp64 products of fp32
values added with math.fsum, i.e. rounded once."""
import math

import numpy as np

F = np.float32


def update(m, v, lr, bc1, bc2s, eps):
    """the Adam step without the decay term, float32 [numel]; zeros for lr < 0 (a parameter without a gradient)"""
    m, v = np.asarray(m, F), np.asarray(v, F)
    if F(lr) < 0:
        return np.zeros_like(m)
    with np.errstate(all="ignore"):
        step_size = F(lr) / F(bc1)
        denom = np.sqrt(v) / F(bc2s) + F(eps)
        return step_size * (m / denom)


def _sumsq(x):
    x = np.asarray(x, np.float64)
    return math.fsum((x * x).tolist())


def row(g, p, m, v, lr, bc1, bc2s, eps):
    """-> (float64 [4], int64 [4]): columns 0-3 and 4-7 of the parameter's row"""
    g, p = np.asarray(g, F).reshape(-1), np.asarray(p, F).reshape(-1)
    u = update(np.asarray(m).reshape(-1), np.asarray(v).reshape(-1), lr, bc1, bc2s, eps)
    gf, pf, uf = np.isfinite(g), np.isfinite(p), np.isfinite(u)
    floats = np.array([_sumsq(g[gf]), _sumsq(p[pf]), _sumsq(u[uf]), float(np.abs(g[gf]).max()) if gf.any() else 0.0], np.float64)
    ints = np.array([int((g[gf] == 0).sum()), int((~gf).sum()), int((~(pf & uf)).sum()), g.size], np.int64)
    return floats, ints


def new_state(n, window):
    """-> (ring int64 [window, n, 8], streak int32 [n, 2], head int64 [4]) as the caller initialises them"""
    return np.zeros((window, n, 8), np.int64), np.zeros((n, 2), np.int32), np.array([0, -1, 0, -1], np.int64)


def append(rows, ring, streak, head, patience):
    """one launch pair: `rows` = [(floats, ints)] per parameter -> the next row of the ring, the streaks, the two latches, head[0]"""
    count, window = int(head[0]), ring.shape[0]
    mask = (1 << 64) - 1

    def offer(k, event):
        if event & mask < int(head[k]) & mask:          # the minimum under unsigned comparison: -1 is the largest
            head[k] = event
    stalled, bad = [], []
    for i, (floats, ints) in enumerate(rows):
        ring[count % window, i, :4] = np.asarray(floats, np.float64).view(np.int64)
        ring[count % window, i, 4:] = ints
        streak[i, 0] = streak[i, 0] + 1 if ints[3] > 0 and ints[0] == ints[3] else 0
        streak[i, 1] = streak[i, 1] + 1 if ints[1] > 0 else 0
        if streak[i, 0] == patience:
            stalled.append(i)
        if streak[i, 1] == 1:
            bad.append(i)
    if stalled:
        offer(1, (count << 32) | min(stalled))
    if bad:
        offer(3, (count << 32) | min(bad))
    head[0] = count + 1


def event(word):
    word = int(word)
    return None if word < 0 else (word >> 32, word & 0xffffffff)
