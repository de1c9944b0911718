"""numpy references of the candidate-ranking kernels (cffm_amd/csrc/rank.hip), written from the ORDER as include/cffm_hip.h
states it in prose - scores compare as IEEE floats with -0 == +0, NaN ranks below everything (-inf included), among equal
scores the smaller candidate position wins - with np.lexsort, not from the 64-bit key the kernels sort on.  key64() is that
key, kept here only so that tests/test_rank_ref.py can check the two against each other."""
import numpy as np

NAN_BITS = 0x7fc00000          # val_out of a padded slot


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def full_order(scores):
    """Positions of ALL candidates of ONE row, best first (no skipping)."""
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    pos = np.arange(s.size)
    nan = np.isnan(s)
    # lexsort: the LAST key is the primary one.  NaN last; then score descending (-0.0 == 0.0 compares equal, NaN slots get a
    # constant so that they tie and fall through to the position); then position ascending.
    val = np.where(nan, np.float32(0), s).astype(np.float64)
    return np.lexsort((pos, -val, nan))


def orders_of(scores):
    """full_order of every row of scores [C,N]: the expensive part, to be computed once and handed to topk_ref / rank_ref."""
    return [full_order(row) for row in np.asarray(scores, dtype=np.float32)]


def order_ref(scores, skip=None, order=None):
    """Positions of the non-skipped candidates of ONE row, best first: skipping removes candidates, it does not reorder them."""
    order = full_order(scores) if order is None else order
    if skip is not None:
        order = order[np.asarray(skip).reshape(-1)[order] == 0]
    return order


def expand_ref(ctx, field, cand, first, rows):
    """ids of global rows [first, first + rows) of the flattened [C * N] (context, candidate) range: int32 [rows, F]."""
    ctx, cand = np.asarray(ctx, dtype=np.int32), np.asarray(cand, dtype=np.int32).reshape(-1)
    N = cand.size
    g = first + np.arange(rows, dtype=np.int64)
    out = ctx[g // N].copy()
    out[:, field] = cand[g % N]
    return out


def topk_ref(scores, k, skip=None, orders=None):
    """(idx int32 [C,k], val bits uint32 [C,k], count int32 [C]) of scores [C,N].  orders: orders_of(scores), if already there."""
    scores = np.asarray(scores, dtype=np.float32)
    C = scores.shape[0]
    idx = np.full((C, k), -1, dtype=np.int32)
    val = np.full((C, k), NAN_BITS, dtype=np.uint32)
    count = np.zeros(C, dtype=np.int32)
    for c in range(C):
        o = order_ref(scores[c], None if skip is None else skip[c], None if orders is None else orders[c])[:k]
        idx[c, :o.size] = o
        val[c, :o.size] = bits(scores[c])[o]
        count[c] = o.size
    return idx, val, count


def rank_ref(scores, target, skip=None, orders=None):
    """0-based rank of candidate target[c] among the non-skipped candidates of row c (its own skip flag ignored); -1 for a target
    outside [0, N)."""
    scores = np.asarray(scores, dtype=np.float32)
    C, N = scores.shape
    out = np.full(C, -1, dtype=np.int32)
    for c in range(C):
        t = int(target[c])
        if not 0 <= t < N:
            continue
        sk = None
        if skip is not None:
            sk = np.array(skip[c]).reshape(-1).copy()
            sk[t] = 0
        out[c] = int(np.nonzero(order_ref(scores[c], sk, None if orders is None else orders[c]) == t)[0][0])
    return out


def key64(scores, skip=None):
    """The kernels' sort key of ONE row (larger = better, 0 = skipped), as include/cffm_hip.h defines it."""
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    u = bits(s + np.float32(0.0)).astype(np.uint64)
    u = np.where(u == 0x80000000, np.uint64(0), u)                 # -0 + 0 is +0 in IEEE arithmetic; spelled out for the reader
    k32 = np.where(np.isnan(s), np.uint64(0), np.where(u >> np.uint64(31) != 0, ~u & np.uint64(0xffffffff), u | np.uint64(0x80000000)))
    key = (k32 << np.uint64(32)) | (np.uint64(0xffffffff) - np.arange(s.size, dtype=np.uint64))
    if skip is not None:
        key = np.where(np.asarray(skip).reshape(-1) != 0, np.uint64(0), key)
    return key


def metrics_ref(ranks, k):
    """HR@k and NDCG@k written out row by row."""
    hr = nd = 0.0
    for r in ranks:
        if 0 <= r < k:
            hr += 1.0
            nd += 1.0 / np.log2(r + 2.0)
    return hr / len(ranks), nd / len(ranks)
