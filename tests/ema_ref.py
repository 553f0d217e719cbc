"""The weight average (spike2former_amd/ema.py, csrc/ema.hip) restated in numpy -- the bit-exact specification the GPU tests compare
against: the momentum schedule (fp64, rounded to fp32 once), the started / copy / skip rule, the lerp of three separately rounded
fp32 operations, the swap, and the fp64 drift sums in chunk order.  Nothing here imports the package."""
import math

import numpy as np

QUIET_NAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]


def momentum(kind, base, gamma, c):
    """the momentum of started update c (mmengine's `steps` == c), as an fp32"""
    if kind == "ExponentialMovingAverage":
        return np.float32(base)
    assert kind == "ExpMomentumEMA"
    return np.float32((1.0 - base) * math.exp(-(1.0 + c) / gamma) + base)


def table(kind, base, gamma=2000):
    """entry c = momentum(c), up to and including the first entry that equals the fp32 limit `base` (one entry for a constant)"""
    out, c = [momentum(kind, base, gamma, 0)], 0
    while kind == "ExpMomentumEMA" and out[-1] != np.float32(base):
        c += 1
        out.append(momentum(kind, base, gamma, c))
    return np.array(out, dtype=np.float32)


def decide(t, begin_iter, interval):
    """update number t (the optimizer's count, from 1) -> ('copy' | 'skip' | 'lerp', c).  mmengine: iteration i = t - 1 has started
    when i + 1 >= begin_iter; `steps` counts the started updates before this one; steps == 0 copies, steps % interval != 0 skips."""
    started = t >= begin_iter
    if not started:
        return "copy", t - max(begin_iter, 1)
    steps = t - max(begin_iter, 1)
    if steps == 0:
        return "copy", 0
    return ("skip", steps) if steps % interval else ("lerp", steps)


def lerp(e, p, m):
    """e + m * (p - e): three fp32 operations, each rounded on its own; a NaN result is the one quiet NaN 0x7fc00000"""
    e, p, m = np.asarray(e, np.float32), np.asarray(p, np.float32), np.float32(m)
    with np.errstate(all="ignore"):
        d = (p - e).astype(np.float32)
        q = (m * d).astype(np.float32)
        r = (e + q).astype(np.float32)
    return np.where(np.isnan(r), QUIET_NAN, r).astype(np.float32)


def update(e, p, t, tab, begin_iter=0, interval=1):
    """one s2f_ema_update over one parameter -> (the new average, whether anything was written)"""
    action, c = decide(t, begin_iter, interval)
    if action == "copy":
        return np.array(p, dtype=np.float32, copy=True), True
    if action == "skip":
        return np.array(e, dtype=np.float32, copy=True), False
    return lerp(e, p, tab[min(c, len(tab) - 1)]), True


def swap(e, p):
    return np.array(p, copy=True), np.array(e, copy=True)


def drift_partials(params, emas, chunk):
    """fp64 [chunks, 2] = {sum (p - e)^2, sum e^2} per chunk of `chunk` elements of each parameter, parameters in table order"""
    rows = []
    for p, e in zip(params, emas):
        p, e = np.asarray(p, np.float64).reshape(-1), np.asarray(e, np.float64).reshape(-1)
        for s in range(0, len(p), chunk):
            with np.errstate(all="ignore"):          # (non-finite inputs give non-finite rows, silently)
                d = p[s:s + chunk] - e[s:s + chunk]
                rows.append((float(np.sum(d * d)), float(np.sum(e[s:s + chunk] * e[s:s + chunk]))))
    return np.array(rows, dtype=np.float64).reshape(-1, 2)


def drift(partials):
    """ema/drift: the partials summed on the host in chunk order"""
    d2 = e2 = 0.0
    for d, e in np.asarray(partials).tolist():
        d2 += d
        e2 += e
    return math.sqrt(d2 / e2)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)
