"""The match log restated in plain numpy loops (include/s2f.h "match log"; csrc/matchlog.hip is the kernel): the six fields per decoder
layer, the usage of every query, the idle streaks and the latch.  The sums run in the prescribed order -- per (layer, image) one serial
fp64 sum with q ascending, then the images' sums with b ascending, both from +0.0 -- so the `cost` word is comparable by BITS.  The
arg-min and arg-max are loops with strict comparisons from index 0 on the fp32 values, nothing vectorised."""
import numpy as np

FIELDS = ("matched", "cost", "greedy", "moved", "cls_hit", "unmatched_obj")
MATCHED, COST, GREEDY, MOVED, CLS_HIT, UNMATCHED_OBJ = range(6)


def first_argmin(column):
    """best = column[0], then strict < with the index ascending, on the fp32 values (as python floats: the same order)"""
    column = np.asarray(column).tolist()
    at = 0
    for q in range(1, len(column)):
        if column[q] < column[at]:
            at = q
    return at


def first_argmax(row):
    """best = row[0], then strict > with the index ascending"""
    row = np.asarray(row).tolist()
    at = 0
    for k in range(1, len(row)):
        if row[k] > row[at]:
            at = k
    return at


def owners(classes, K):
    """{class: the lowest query matched to it} of one (layer, image): `classes` int [Q], anything outside 0 .. K-1 is unmatched"""
    out = {}
    for q, c in enumerate(classes):
        c = int(c)
        if 0 <= c < K and c not in out:
            out[c] = q
    return out


def row(cost, cls, row_class):
    """cost fp32 [L, B, Q, K], cls fp32 [L, B, Q, K+1], row_class int32 [B, L*Q] -> (fields int64 [L, 6] with the cost as the bits of
    its double, usage int32 [Q])"""
    L, B, Q, K = cost.shape
    assert cls.shape == (L, B, Q, K + 1) and row_class.shape == (B, L * Q) and cost.dtype == cls.dtype == np.float32
    table = row_class.reshape(B, L, Q)
    fields = np.zeros((L, 6), np.int64)
    usage = np.zeros(Q, np.int32)
    for l in range(L):
        layer_cost = np.float64(0.0)
        for b in range(B):
            now = owners(table[b, l], K)
            before = owners(table[b, l - 1], K) if l > 0 else {}
            cheapest = {c: first_argmin(cost[l, b, :, c]) for c in now}
            paid = np.float64(0.0)
            for q in range(Q):
                c = int(table[b, l, q])
                top = first_argmax(cls[l, b, q])
                if 0 <= c < K:
                    fields[l, MATCHED] += 1
                    paid = paid + np.float64(cost[l, b, q, c])
                    fields[l, GREEDY] += cheapest[c] == q
                    fields[l, MOVED] += l > 0 and before.get(c) != q
                    fields[l, CLS_HIT] += top == c
                    if l == L - 1:
                        usage[q] += 1
                else:
                    fields[l, UNMATCHED_OBJ] += top != K
            layer_cost = layer_cost + paid
        fields[l, COST] = np.float64(layer_cost).view(np.int64)
    return fields, usage


def costs(fields):
    """fields int64 [..., 6] -> the cost column as doubles"""
    return np.ascontiguousarray(fields[..., COST]).view(np.float64)


def row_words(L, Q):
    return 6 * L + (Q + 1) // 2


def new_state(L, Q, window):
    """-> (ring int64 [window, 6L + ceil(Q/2)], idle int32 [Q], head int64 [4]) as MatchLog.clear() leaves them"""
    return np.zeros((window, row_words(L, Q)), np.int64), np.zeros(Q, np.int32), np.array([0, -1, 0, 0], np.int64)


def pack(fields, usage):
    """-> the row's 8-byte words: the fields, then usage as int32 padded with a zero to whole words"""
    Q = len(usage)
    padded = np.zeros(2 * ((Q + 1) // 2), np.int32)
    padded[:Q] = usage
    return np.concatenate([fields.reshape(-1), padded.view(np.int64)])


def append(fields, usage, ring, idle, head, patience):
    """what s2f_match_log_rows does with one row's sums: ring, idle and head are updated in place"""
    count = int(head[0])
    ring[count % ring.shape[0]] = pack(fields, usage)
    for q in range(len(usage)):
        if usage[q] > 0:
            idle[q] = 0
        else:
            idle[q] += 1
            if idle[q] == patience:
                event = (count << 32) | q
                if head[1] < 0 or event < head[1]:          # the unsigned minimum: -1 is the largest value
                    head[1] = event
    head[0] = count + 1


def first_idle(head):
    return None if head[1] < 0 else (int(head[1]) >> 32, int(head[1]) & 0xffffffff)
