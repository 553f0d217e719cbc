"""The segmentation log's rule in numpy, fp64 (include/s2f.h "segmentation log"; csrc/seglog.hip): the score of MaskFormerHead.predict
at the mask resolution, the first-maximum arg-max with NaN largest, the three areas of intersect_and_union against seg[:, ::2, ::2],
and the ring / streak / latch rule of one appended row.  The tests' reference: nothing here is imported by the package."""
import numpy as np

IGNORE = 255


def softmax_table(cls_lb, K):
    """cls_lb [Q, K+1] -> P fp64 [Q, K]: softmax over all K+1 columns, the void column dropped"""
    c = np.asarray(cls_lb, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(c - c.max(axis=1, keepdims=True))
        return (e / e.sum(axis=1, keepdims=True))[:, :K]


def sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def scores(cls_lb, mask_lb, K):
    """cls_lb [Q, K+1], mask_lb [Q, h, w] -> score fp64 [K, h, w] = sum over q ASCENDING of P[q, k] * S[q, p] (the kernel's order)"""
    P, S = softmax_table(cls_lb, K), sigmoid(mask_lb)
    out = np.zeros((K,) + S.shape[1:], np.float64)
    with np.errstate(invalid="ignore"):
        for q in range(P.shape[0]):
            out += P[q][:, None, None] * S[q][None]
    return out


def argmax_first(score):
    """score [K, ...] -> int64 [...]: the first maximum over axis 0; NaN counts as larger than any number (the first NaN wins)"""
    score = np.asarray(score)
    nan = np.isnan(score)
    with np.errstate(invalid="ignore"):
        plain = np.argmax(np.where(nan, -np.inf, score), axis=0)
    return np.where(nan.any(axis=0), np.argmax(nan, axis=0), plain).astype(np.int64)


def count(pred, label, K):
    """pred, label: integer maps of one shape -> int64 [3, K] = {intersect, pred, label} over the pixels with label < K"""
    pred, label = np.asarray(pred).reshape(-1), np.asarray(label).reshape(-1).astype(np.int64)
    keep = label < K          # 255 (ignored) and any label >= K count nowhere
    pred, label = pred[keep], label[keep]
    return np.stack([np.bincount(label[pred == label], minlength=K), np.bincount(pred, minlength=K),
                     np.bincount(label, minlength=K)]).astype(np.int64)


def areas(cls, masks, seg, layers):
    """cls [L, B, Q, K+1], masks [L, B, Q, h, w], seg uint8 [B, 2h, 2w], layers: the scored ones -> one row, int64 [L', 3, K]"""
    cls, masks, seg = np.asarray(cls), np.asarray(masks), np.asarray(seg)
    K = cls.shape[-1] - 1
    small = seg[:, ::2, ::2]
    row = np.zeros((len(layers), 3, K), np.int64)
    for i, l in enumerate(layers):
        for b in range(cls.shape[1]):
            row[i] += count(argmax_first(scores(cls[l, b], masks[l, b], K)), small[b], K)
    return row


def near_ties(cls, masks, layers):
    """-> bool [B, h, w]: the pixels whose fp64 top-two score gap in ANY scored layer is below 4 * Q * 2^-24 * max(1, max score), the
    fp32 accumulation bound of Q products <= 1 -- there the kernel's fp32 arg-max may differ legitimately"""
    cls, masks = np.asarray(cls), np.asarray(masks)
    L, B, Q, K1 = cls.shape
    out = np.zeros((B,) + masks.shape[-2:], bool)
    if K1 - 1 < 2:
        return out
    for l in layers:
        for b in range(B):
            s = np.sort(scores(cls[l, b], masks[l, b], K1 - 1), axis=0)
            out[b] |= (s[-1] - s[-2]) < 4 * Q * 2.0 ** -24 * np.maximum(1.0, s[-1])
    return out


def mask_labels(seg, drop):
    """seg uint8 [B, 2h, 2w] with the pixels the mask-resolution map `drop` [B, h, w] names set to 255 (a copy)"""
    seg = np.array(seg, copy=True)
    sub = seg[:, ::2, ::2]
    sub[drop] = IGNORE
    return seg


# ---------------------------------------------------------------------------------------------------- the ring of one log
def new_state(K, nl, window):
    """-> (ring int64 [window, nl, 3, K], streak int32 [K], head int64 [4] = {rows, latch, ticket, reserved})"""
    return np.zeros((window, nl, 3, K), np.int64), np.zeros(K, np.int32), np.array([0, -1, 0, 0], np.int64)


def append(row, ring, streak, head, patience):
    """one launch pair: row int64 [nl, 3, K] OVERWRITES ring[head[0] % window]; the streaks follow the LAST scored layer: 0 where a
    class was hit, + 1 where it was labelled and not hit, unchanged where it is absent; the first class to REACH patience is offered
    to head[1] as row << 32 | class, which keeps the minimum under unsigned comparison; head[0] += 1"""
    n = int(head[0])
    ring[n % ring.shape[0]] = row
    hit, labelled = row[-1, 0] > 0, row[-1, 2] > 0
    missed = labelled & ~hit
    streak[hit] = 0
    streak[missed] += 1
    reached = np.flatnonzero(missed & (streak == patience))
    if reached.size:
        event, mask = (n << 32) | int(reached[0]), (1 << 64) - 1
        if event & mask < int(head[1]) & mask:
            head[1] = event
    head[0] = n + 1


def first_missed(head):
    word = int(head[1])
    return None if word < 0 else (word >> 32, word & 0xffffffff)
