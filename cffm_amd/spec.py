"""Shapes, hyper-parameters and parameter initialisation of the CFFM hot path.

Mirrors the constructor arguments of the reference class (CFFM.py:98-147) and the variable set it
creates (CFFM.py:239-293, :323, :375-377, :339, :409-410, :441).  Pure Python/numpy: importable
without a GPU and without the HIP library.
"""
import math
from dataclasses import dataclass

import numpy as np

ACTIVATIONS = ('relu', 'prelu', 'elu', 'selu', 'gelu')   # CFFM.py:132-141, enum order of cffm_hip.h
ADAGRAD_INIT_ACC = 1e-8                                  # CFFM.py:524


@dataclass
class CFFMConfig:
    M: int                      # features_M
    F: int                      # num_field
    K: int = 32                 # inner_dims
    D: int = 32                 # outer_dims
    activation: str = 'relu'
    lamda_att: float = 1.0
    beta_outer: float = 1.0
    linear_att: int = 1
    inner_conv: int = 1
    outer_conv: int = 1
    loss_type: str = 'square_loss'
    lamda_bilinear: float = 0.0
    optimizer: str = 'AdagradOptimizer'
    lr: float = 0.05

    def __post_init__(self):
        if self.activation not in ACTIVATIONS:
            raise ValueError('activation must be one of %s' % (ACTIVATIONS,))
        if self.F < 2:
            raise ValueError('num_field must be >= 2')
        if self.D < 4 or (self.D & (self.D - 1)):
            raise ValueError('outer_dims must be a power of two >= 4 (stride-2 VALID conv chain)')
        if self.K < 2 or self.K % 2:
            raise ValueError('inner_dims must be even (1x2 stride-2 window)')

    @property
    def P(self):                # CFFM.py:130
        return int(self.F * (self.F - 1) / 2)

    @property
    def Lc(self):               # CFFM.py:373
        return int(math.log(self.D, 2))

    @property
    def live_layers(self):      # layer Lc-1 never reaches t1 (CFFM.py:394-396)
        return self.Lc - 1

    @property
    def t1_width(self):
        return 2 * self.D - 2

    @property
    def act_id(self):
        return ACTIVATIONS.index(self.activation)


def pair_lists(F):
    """(i, j) of pair p in the reference's row-major i<j order (CFFM.py:304-305)."""
    ii = [i for i in range(F) for _ in range(i + 1, F)]
    jj = [j for i in range(F) for j in range(i + 1, F)]
    return ii, jj


def param_shapes(cfg):
    P, Lc, F, K, D, M = cfg.P, cfg.Lc, cfg.F, cfg.K, cfg.D, cfg.M
    s = {
        'inner_embeddings': (M, K), 'outer_embeddings': (M, D), 'feature_bias': (M, 1),
        'outer_W': (P, 1), 'outer_b': (1,),
        'bias_W': (F, F), 'bias_b': (F,), 'bias': (),
        'inner_layer_conv_weight_0': (1, 2, 1, 2), 'inner_layer_conv_bias_0': (2,),
        'dense_kernel': (P * K, 1), 'dense_bias': (1,),
        'dense_1_kernel': (2 * D - 2, 32), 'dense_1_bias': (32,),
        'dense_2_kernel': (32, 1), 'dense_2_bias': (1,),
        'dense_3_kernel': (F, 1), 'dense_3_bias': (1,),
    }
    for l in range(Lc):
        s['outer_layer_conv_weight_%d' % l] = (2, 2, P, P)
        s['outer_layer_conv_bias_%d' % l] = (P,)
    return s


TABLES = ('inner_embeddings', 'outer_embeddings', 'feature_bias')
UNTRAINED = ('outer_W', 'outer_b')   # created, counted, never used (CFFM.py:271-272, :412)


def logged_param_count(cfg):
    """The number ``calculate_parameters`` logs (CFFM.py:543-553): members of self.weights only."""
    n = 0
    for name, shp in param_shapes(cfg).items():
        if name.startswith('dense'):
            continue
        n += int(np.prod(shp)) if shp else 1
    return n


def _trunc_normal(rng, shape, std=1.0):
    x = rng.standard_normal(shape)
    bad = np.abs(x) > 2.0
    while bad.any():                     # tf.truncated_normal: re-draw beyond two sigma (CFFM.py:460)
        x[bad] = rng.standard_normal(int(bad.sum()))
        bad = np.abs(x) > 2.0
    return x * std


def _glorot_uniform(rng, shape):
    lim = math.sqrt(6.0 / (shape[0] + shape[1]))
    return rng.uniform(-lim, lim, size=shape)


def init_params(cfg, seed=2021, dtype=np.float32, tables=True):
    """Parameter dict with the reference's initial distributions.  The reference seeds
    nothing; a seed is taken here so that runs and tests are repeatable.  tables=False leaves the three
    embedding tables out (HipEngine(params='device') draws them on the GPU)."""
    rng = np.random.default_rng(seed)
    p = {}
    for name, shp in param_shapes(cfg).items():
        if not tables and name in TABLES:
            continue
        if name == 'inner_embeddings':
            v = rng.standard_normal(shp) * 0.1
        elif name == 'outer_embeddings':
            v = rng.standard_normal(shp) * 0.01
        elif name == 'feature_bias':
            v = np.zeros(shp)                          # random_normal(stddev=0) -> exactly 0
        elif name == 'bias':
            v = np.zeros(shp)
        elif name.endswith('conv_bias_0') or 'conv_bias_' in name:
            v = np.full(shp, 0.01)                     # bias_variable (CFFM.py:466)
        elif name.startswith('dense') and name.endswith('kernel'):
            v = _glorot_uniform(rng, shp)              # tf.layers.dense default
        elif name.startswith('dense'):
            v = np.zeros(shp)
        else:                                          # weight_variable: trunc-N(0,1)
            v = _trunc_normal(rng, shp)
        p[name] = np.ascontiguousarray(v, dtype=dtype)
    return p


# ---- tables drawn by GLOBAL row: the numpy twin (and the specification) of cffm_init_table_rows, include/cffm_hip.h -------------
PHILOX_M = (0xD2511F53, 0xCD9E8D57)
PHILOX_W = (0x9E3779B9, 0xBB67AE85)
TABLE_STD = {'inner_embeddings': 0.1, 'outer_embeddings': 0.01}      # CFFM.py:257, :264


def philox4x32_10(counter, key):
    """Philox4x32-10 on arrays: counter = four, key = two arrays (or scalars) of 32-bit words, broadcast against each other.
    Returns the four output words as uint32 arrays.  The words are carried in uint64 so that the 32 x 32 -> 64 bit products
    are exact."""
    mask = np.uint64(0xffffffff)
    c0, c1, c2, c3 = (np.asarray(c).astype(np.uint64) & mask for c in counter)
    k0, k1 = (np.asarray(k).astype(np.uint64) & mask for k in key)
    m0, m1 = np.uint64(PHILOX_M[0]), np.uint64(PHILOX_M[1])
    w0, w1 = np.uint64(PHILOX_W[0]), np.uint64(PHILOX_W[1])
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = c0 * m0, c2 * m1
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & mask, (p0 >> sh) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + w0) & mask, (k1 + w1) & mask
    return tuple(np.asarray(c).astype(np.uint32) for c in (c0, c1, c2, c3))


def table_words(seed, rows, table, width):
    """The integer half of the draw: Philox words of global ``rows`` for the ceil(width / 4) column groups of ``table``
    (0 inner, 1 outer), four uint32 arrays [n, groups].  Exact, so one call serves every floating-point evaluation."""
    seed = int(seed) & 0xffffffffffffffff
    g = np.asarray(rows).astype(np.uint64).reshape(-1, 1)
    q = np.arange((int(width) + 3) // 4, dtype=np.uint64).reshape(1, -1)
    return philox4x32_10((g & np.uint64(0xffffffff), g >> np.uint64(32), q, np.uint64(table)), (seed & 0xffffffff, seed >> 32))


def unit_normals(words, width, dtype=np.float64):
    """Box-Muller of table_words() in ``dtype``: [n, width] unit normals (the 24-bit uniforms are exact in float32, so only
    log, sqrt and sin / cos are evaluated in ``dtype``)."""
    dt = np.dtype(dtype).type
    x0, x1, x2, x3 = words
    out = np.empty(x0.shape + (4,), dtype=dtype)
    for a, b, c in ((x0, x1, 0), (x2, x3, 2)):
        u1 = ((a >> np.uint32(8)).astype(dtype) + dt(1)) * dt(2.0 ** -24)
        u2 = (b >> np.uint32(8)).astype(dtype) * dt(2.0 ** -24)
        r = np.sqrt(dt(-2) * np.log(u1))
        ang = dt(2 * math.pi) * u2
        out[..., c] = r * np.cos(ang)
        out[..., c + 1] = r * np.sin(ang)
    return out.reshape(x0.shape[0], -1)[:, :int(width)]


def table_rows(cfg, seed, rows, dtype=np.float64):
    """The three tables at an arbitrary array of GLOBAL rows, as cffm_init_table_rows draws them: a value depends on
    (seed, global row, table, column) alone, so table_rows(rows)[i] is row rows[i] of the one model that ``seed`` names, for
    every sharding.  N(0, 0.1) / N(0, 0.01) / exact zeros (CFFM.py:257-277); the table of a disabled branch stays zero."""
    rows = np.asarray(rows).reshape(-1)
    dt = np.dtype(dtype).type
    out = {}
    for t, (name, width, on) in enumerate((('inner_embeddings', cfg.K, cfg.inner_conv), ('outer_embeddings', cfg.D, cfg.outer_conv))):
        if on:
            out[name] = np.ascontiguousarray(unit_normals(table_words(seed, rows, t, width), width, dtype) * dt(TABLE_STD[name]))
        else:
            out[name] = np.zeros((rows.shape[0], width), dtype=dtype)
    out['feature_bias'] = np.zeros((rows.shape[0], 1), dtype=dtype)
    return out


# ---- ranked lists drawn BY LIST ID: the numpy twin (and the specification) of cffm_draw_lists, include/cffm_hip.h ----------------
DRAW_TAG = 2                 # fourth counter word of the list draw; the table draw uses 0 (inner) and 1 (outer) there
DRAW_MAX_M = 1023            # lists of at most 1024, the bound cffm_topk has


def draw_words(seed, ids, n_words):
    """Words 0 .. n_words - 1 of the lists ``ids`` (64-bit list ids), uint64 [G, n_words]: word i is output word i & 3 of
    philox4x32_10(counter = (id lo, id hi, i >> 2, DRAW_TAG), key = (seed lo, seed hi))."""
    seed = int(seed) & 0xffffffffffffffff
    g = np.asarray(ids).astype(np.uint64).reshape(-1, 1)
    q = np.arange((int(n_words) + 3) // 4, dtype=np.uint64).reshape(1, -1)
    x = philox4x32_10((g & np.uint64(0xffffffff), g >> np.uint64(32), q, np.uint64(DRAW_TAG)), (seed & 0xffffffff, seed >> 32))
    return np.stack(x, axis=2).reshape(g.shape[0], -1)[:, :int(n_words)].astype(np.uint64)


def draw_lists(seed, list0, at, U, m):
    """G = len(at) ranked lists over a set of U distinct tuples: list g (id list0 + g) holds its positive at[g] and m distinct
    other indices of [0, U), the positive at a drawn place.  Returns (lists int64 [G, m + 1], place int64 [G]).  A list is a
    function of (seed, id) alone.  Integer arithmetic only: the negatives are the length-m prefix of a Fisher-Yates shuffle of
    0 .. U - 2 carried as a sparse map (position -> value, absent = identity), step i swapping position i with
    t = i + ((w_i * (U - 1 - i)) >> 32); a value >= at[g] is moved up by one (the set without the target); the place is
    (w_m * (m + 1)) >> 32.  The map is two arrays filled in step order, as the kernel holds it."""
    at = np.asarray(at).astype(np.int64).reshape(-1)
    U, m, G = int(U), int(m), int(at.shape[0])
    if U < 2 or not 1 <= m <= U - 1:
        raise ValueError('draw_lists: needs U >= 2 and 1 <= m <= U - 1')
    n = U - 1
    w = draw_words(seed, np.uint64(int(list0)) + np.arange(G, dtype=np.uint64), m + 1)
    sh = np.uint64(32)
    keys = np.full((G, m), -1, dtype=np.int64)
    vals = np.zeros((G, m), dtype=np.int64)
    cnt = np.zeros(G, dtype=np.int64)
    chosen = np.empty((G, m), dtype=np.int64)
    rows = np.arange(G)

    def find(k, i):
        hit = keys[:, :max(i, 1)] == k[:, None]             # unfilled entries hold -1
        return hit.any(axis=1), hit.argmax(axis=1)

    for i in range(m):
        t = i + ((w[:, i] * np.uint64(n - i)) >> sh).astype(np.int64)
        has_t, pos_t = find(t, i)
        has_i, pos_i = find(np.full(G, i, dtype=np.int64), i)
        vt = np.where(has_t, vals[rows, pos_t], t)
        vi = np.where(has_i, vals[rows, pos_i], i)
        chosen[:, i] = vt
        slot = np.where(has_t, pos_t, cnt)                  # map[t] = vi: the entry of t, or a new one
        keys[rows, slot] = t
        vals[rows, slot] = vi
        cnt += ~has_t
    neg = chosen + (chosen >= at[:, None])
    place = ((w[:, m] * np.uint64(m + 1)) >> sh).astype(np.int64)
    p = np.arange(m + 1)[None, :]
    src = np.clip(p - (p > place[:, None]), 0, m - 1)
    lists = np.where(p == place[:, None], at[:, None], np.take_along_axis(neg, src, axis=1))
    return lists, place


# ---- weighted ranked lists drawn BY LIST ID: the numpy twin (and the specification) of cffm_draw_lists_weighted -------------------
DRAW_W_TAG = 3               # fourth counter word of the weighted list draw (the table draw: 0 and 1, the uniform list draw: 2)
DRAW_W_PLACE = 0xffffffff    # third counter word of the block whose word 0 draws the place


def draw_weighted_cap(m):
    """The most words a list of m negatives consumes before it counts as incomplete: 8 rounds of 64 per 64 slots, and 8 more."""
    return 64 * (8 * ((int(m) + 1 + 63) // 64) + 8)


def weight_cdf(weights):
    """uint32 [U] for cffm_draw_lists_weighted: the running sum of q_j = floor(w_j * scale) + (w_j > 0) with
    scale = (2^32 - 1 - U) / sum(w), so that the total is at most 2^32 - 1, every positive weight holds at least one of the T values
    and a zero weight holds none (cdf[j] == cdf[j - 1]: never drawn).  weights: non-negative, finite, one positive at least."""
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim != 1 or w.shape[0] < 1 or not np.isfinite(w).all() or (w < 0).any() or not (w > 0).any():
        raise ValueError('weight_cdf: weights must be a vector of non-negative finite numbers with at least one positive')
    U = int(w.shape[0])
    if U > 2 ** 31 - 1:
        raise ValueError('weight_cdf: at most 2^31 - 1 weights')
    total = float(w.sum())
    if not np.isfinite(total):
        raise ValueError('weight_cdf: the sum of the weights is not finite')
    scale = float(2 ** 32 - 1 - U) / total
    q = np.floor(w * scale).astype(np.uint64) + (w > 0).astype(np.uint64)
    cdf = np.cumsum(q, dtype=np.uint64)
    if int(cdf[-1]) > 2 ** 32 - 1:                          # only rounding in sum(w) could do this; never seen
        raise ValueError('weight_cdf: the quantised weights sum to more than 2^32 - 1')
    return cdf.astype(np.uint32)


def draw_words_weighted(seed, ids, n_words):
    """Words 0 .. n_words - 1 of the weighted lists ``ids``, uint64 [G, n_words] (n_words a multiple of 4): word i is output word
    i & 3 of philox4x32_10(counter = (id lo, id hi, i >> 2, DRAW_W_TAG), key = (seed lo, seed hi))."""
    seed = int(seed) & 0xffffffffffffffff
    g = np.asarray(ids).astype(np.uint64).reshape(-1, 1)
    q = np.arange((int(n_words) + 3) // 4, dtype=np.uint64).reshape(1, -1)
    x = philox4x32_10((g & np.uint64(0xffffffff), g >> np.uint64(32), q, np.uint64(DRAW_W_TAG)), (seed & 0xffffffff, seed >> 32))
    return np.stack(x, axis=2).reshape(g.shape[0], -1)[:, :int(n_words)].astype(np.uint64)


def _accept_first(cand, at, m):
    """Sequential acceptance over the candidate words of every row at once: candidate i is accepted iff it is not the row's target
    and did not occur earlier in the row.  Returns (neg int64 [G, m], the first m accepted in order, -1 where there are fewer;
    full bool [G])."""
    G, n = cand.shape
    order = np.argsort(cand, axis=1, kind='stable')
    srt = np.take_along_axis(cand, order, axis=1)
    first_sorted = np.ones((G, n), dtype=bool)
    first_sorted[:, 1:] = srt[:, 1:] != srt[:, :-1]          # stable: the earliest occurrence leads its run
    first = np.zeros((G, n), dtype=bool)
    np.put_along_axis(first, order, first_sorted, axis=1)
    ok = first & (cand != at[:, None])
    rank = np.cumsum(ok, axis=1)
    neg = np.full((G, m + 1), -1, dtype=np.int64)            # column m takes everything past the m-th
    rows, cols = np.nonzero(ok)
    neg[rows, np.minimum(rank[rows, cols] - 1, m)] = cand[rows, cols]
    return neg[:, :m], rank[:, -1] >= m


def draw_lists_weighted(seed, list0, at, cdf, m):
    """G = len(at) ranked lists over U = len(cdf) distinct tuples with the negatives drawn in proportion to the weights behind
    ``cdf`` (weight_cdf): list g (id list0 + g) holds its positive at[g] and m distinct other indices, the positive at a drawn
    place.  Returns (lists int64 [G, m + 1], place int64 [G]).  A list is a function of (seed, id) alone; integer arithmetic only.
    With T = cdf[U - 1]: word w gives r = (w * T) >> 32 and the candidate j = #{cdf <= r}, clamped to U - 1; candidates are taken
    in word order, one is accepted iff it is not at[g] and was not accepted before, and the negatives are the first m accepted in
    that order - successive sampling without replacement, proportional to the weights, over the set without the target.  A list
    that has not accepted m after draw_weighted_cap(m) words is incomplete: its row and its place are -1, as they are for an at[g]
    outside [0, U) and for T == 0.  The place is (w_place * (m + 1)) >> 32, w_place word 0 of the counter
    (id lo, id hi, DRAW_W_PLACE, DRAW_W_TAG)."""
    at = np.asarray(at).astype(np.int64).reshape(-1)
    cdf = np.asarray(cdf)
    if cdf.ndim != 1 or cdf.shape[0] < 1:
        raise ValueError('draw_lists_weighted: cdf must be a vector of U >= 1 words')
    cdf = (cdf.astype(np.int64) & 0xffffffff).astype(np.uint64)                  # int32 storage is reinterpreted
    U, m, G = int(cdf.shape[0]), int(m), int(at.shape[0])
    if not 1 <= m <= U - 1:
        raise ValueError('draw_lists_weighted: needs 1 <= m <= U - 1')
    T = cdf[U - 1]
    sh = np.uint64(32)
    ids = np.uint64(int(list0)) + np.arange(G, dtype=np.uint64)
    lists = np.full((G, m + 1), -1, dtype=np.int64)
    place = np.full(G, -1, dtype=np.int64)
    live = np.nonzero((at >= 0) & (at < U))[0] if int(T) > 0 else np.zeros(0, dtype=np.int64)
    cap = draw_weighted_cap(m)
    chunk = max(1, (1 << 21) // cap)
    for c0 in range(0, live.shape[0], chunk):
        todo = live[c0:c0 + chunk]
        n = min(cap, 64 * (2 * ((m + 1 + 63) // 64)))
        while todo.shape[0]:                                 # a prefix of the words decides a list that completes inside it
            w = draw_words_weighted(seed, ids[todo], n)
            cand = np.minimum(np.searchsorted(cdf, (w * T) >> sh, side='right'), U - 1).astype(np.int64)
            neg, full = _accept_first(cand, at[todo], m)
            done = todo[full]
            if done.shape[0]:
                idd = ids[done].reshape(-1, 1)
                wp = philox4x32_10((idd & np.uint64(0xffffffff), idd >> sh, np.uint64(DRAW_W_PLACE), np.uint64(DRAW_W_TAG)),
                                   (int(seed) & 0xffffffff, (int(seed) & 0xffffffffffffffff) >> 32))[0].astype(np.uint64).reshape(-1)
                pl = ((wp * np.uint64(m + 1)) >> sh).astype(np.int64)
                p = np.arange(m + 1)[None, :]
                src = np.clip(p - (p > pl[:, None]), 0, m - 1)
                lists[done] = np.where(p == pl[:, None], at[done][:, None], np.take_along_axis(neg[full], src, axis=1))
                place[done] = pl
            if n == cap:
                break
            todo, n = todo[~full], min(cap, 2 * n)
    return lists, place


# ---- hard negatives picked from a scored pool BY LIST ID: the numpy twin (and the specification) of cffm_pick_hard ----------------
HARD_TAG = 4                 # fourth counter word of the pick's place (the table draw: 0 and 1, the list draws: 2 and 3)
HARD_MAX_LP = 1024           # pools of at most 1024 positions, the positive among them


def pick_hard(seed, list0, scores, target_pool, m):
    """The select step of dynamic negative sampling over G scored pools of Lp positions: scores float32 [G, Lp], target_pool [G] the
    pool position of each list's positive (list g has the id list0 + g).  Returns (sel int64 [G, m + 1], place int64 [G]): sel holds
    pool positions - the positive at place[g], around it the m best-scored of the Lp - 1 other positions, hardest first, the
    negative of rank r at slot r + (r >= place) - and a list whose target lies outside [0, Lp) has a row of -1 and place -1.
    The order is that of include/cffm_hip.h in prose: score descending as IEEE floats with -0 == +0, NaN below everything (-inf
    included), equal scores (NaN among themselves too) to the smaller position.  Integer work on the float bits and one lexsort,
    not the 64-bit key the kernel compares.  place = (w * (m + 1)) >> 32, w output word 0 of philox4x32_10(counter = (id lo, id hi,
    0, HARD_TAG), key = (seed lo, seed hi)): a function of (seed, id, m) alone."""
    s = np.asarray(scores)
    if s.ndim != 2 or s.dtype != np.float32:
        raise ValueError('pick_hard: scores must be float32 [G, Lp]')
    t = np.asarray(target_pool).astype(np.int64).reshape(-1)
    G, Lp, m = int(s.shape[0]), int(s.shape[1]), int(m)
    if not 2 <= Lp <= HARD_MAX_LP or not 1 <= m <= Lp - 1 or t.shape[0] != G:
        raise ValueError('pick_hard: needs 2 <= Lp <= %d, 1 <= m <= Lp - 1 and one target per list' % HARD_MAX_LP)
    seed = int(seed) & 0xffffffffffffffff
    sel = np.full((G, m + 1), -1, dtype=np.int64)
    place = np.full(G, -1, dtype=np.int64)
    live = np.nonzero((t >= 0) & (t < Lp))[0]
    if live.shape[0] == 0:
        return sel, place
    b = s[live].view(np.uint32)
    nan = (b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    neg = (b >> np.uint32(31)).astype(np.int64)
    mag = (b & np.uint32(0x7fffffff)).astype(np.int64)
    val = np.where(nan, 0, np.where(neg == 1, -mag, mag))        # the floats' own order on their bits; -0 and +0 both give 0
    pos = np.broadcast_to(np.arange(Lp, dtype=np.int64), val.shape)
    own = pos == t[live][:, None]
    # lexsort: the LAST key is the primary one.  The positive last of all; then NaN last; then score descending; then position
    order = np.lexsort((pos, -val, nan, own), axis=-1)
    ids = (np.uint64(int(list0)) + live.astype(np.uint64)).reshape(-1)
    w = philox4x32_10((ids & np.uint64(0xffffffff), ids >> np.uint64(32), np.uint64(0), np.uint64(HARD_TAG)),
                      (seed & 0xffffffff, seed >> 32))[0].astype(np.uint64)
    pl = ((w * np.uint64(m + 1)) >> np.uint64(32)).astype(np.int64)
    slot = np.arange(m + 1, dtype=np.int64)[None, :]
    src = np.clip(slot - (slot > pl[:, None]), 0, m - 1)         # the rank held by a slot other than the place
    sel[live] = np.where(slot == pl[:, None], t[live][:, None], np.take_along_axis(order[:, :m], src, axis=1))
    place[live] = pl
    return sel, place


# ---- logQ-corrected sampled softmax: the table and the float64 twin (and the specification) of cffm_list_loss_logq ----------------
def logq_table(cdf, m, U=None):
    """float32 [U, 2] for cffm_list_loss_logq: column 0 is log(m q_j), column 1 is log(1 - q_j), q the proposal the m negatives of a
    list were drawn from.  cdf: the words of weight_cdf (int32 storage is reinterpreted), q_j = (cdf[j] - cdf[j - 1]) / T with
    T = cdf[U - 1]; an index that is never drawn (q_j = 0) gets -inf in column 0, and column 1 is log1p(-q_j).  cdf=None with U is the
    uniform proposal q = 1 / U.  Computed in float64 and rounded once."""
    m = int(m)
    if m < 1:
        raise ValueError('logq_table: needs m >= 1 negatives')
    if cdf is None:
        if U is None or int(U) < 1:
            raise ValueError('logq_table: the uniform table needs U >= 1')
        q = np.full(int(U), 1.0 / int(U), dtype=np.float64)
    else:
        cdf = np.asarray(cdf)
        if cdf.ndim != 1 or cdf.shape[0] < 1:
            raise ValueError('logq_table: cdf must be a vector of U >= 1 words')
        if U is not None and int(U) != cdf.shape[0]:
            raise ValueError('logq_table: U = %d is not the length of the cdf (%d)' % (int(U), cdf.shape[0]))
        words = cdf.astype(np.int64) & 0xffffffff
        T = int(words[-1])
        if T == 0:
            raise ValueError('logq_table: the cdf has total T == 0: nothing can be drawn from it')
        q = np.diff(words, prepend=0).astype(np.float64) / float(T)
    with np.errstate(divide='ignore'):
        return np.stack([np.log(m * q), np.log1p(-q)], axis=1).astype(np.float32)


def list_loss_logq(scores, target, lists, corr):
    """The logQ-corrected sampled softmax in float64: scores [G, Lg], target [G] the positives' places, lists [G, Lg] the candidates'
    indices i_n into U distinct tuples, corr [U, 2] (logq_table).  With t = target[g]: c_n = corr[i_n, 0] - corr[i_t, 1] for n != t,
    c_t = 0, z = s - c, terms[g] = logsumexp(z) - z_t, dout[g, n] = (softmax(z)_n - [n = t]) / G, loss = mean of the terms.  A target
    outside [0, Lg), and any index outside [0, U) in a list with a valid target, gives a zero row and a zero term; a non-finite z
    does what the arithmetic does (NaN term and row).  Returns (loss float, dout float64 [G, Lg], terms float64 [G])."""
    s = np.asarray(scores, dtype=np.float64)
    ix = np.asarray(lists).astype(np.int64)
    c = np.asarray(corr, dtype=np.float64)
    t = np.asarray(target).astype(np.int64).reshape(-1)
    if s.ndim != 2 or ix.shape != s.shape or t.shape[0] != s.shape[0] or c.ndim != 2 or c.shape[1] != 2:
        raise ValueError('list_loss_logq: scores and lists [G, Lg], target [G], corr [U, 2]')
    G, Lg = s.shape
    U = c.shape[0]
    dout, terms = np.zeros((G, Lg)), np.zeros(G)
    for g in range(G):
        tg = int(t[g])
        if tg < 0 or tg >= Lg or (ix[g] < 0).any() or (ix[g] >= U).any():
            continue
        with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
            corr_g = c[ix[g], 0] - c[ix[g, tg], 1]
            corr_g[tg] = 0.0
            z = s[g] - corr_g
            mx = np.max(z) if not np.isnan(z).any() else np.nan
            e = np.exp(z - mx)
            den = e.sum()
            terms[g] = np.log(den) + mx - z[tg]
            p = e / den
            p[tg] -= 1.0
            dout[g] = p / G
            if np.isnan(terms[g]):
                dout[g] = np.nan
    return (float(terms.sum() / G) if G else 0.0), dout, terms


# ---- the skip mask of a ranking call from a sparse "seen" relation: the build and the numpy twin (and the specification) of
# cffm_seen_mask ------------------------------------------------------------------------------------------------
def seen_index(owner, cand_pos):
    """The CSR of a seen relation from parallel arrays: pair i says that owner[i] has seen the candidate at position cand_pos[i].
    Returns (keys int64 [R] the sorted distinct owners, off int32 [R + 1], pos int32 [nnz]): row r, pos[off[r]:off[r + 1]], holds the
    positions of owner keys[r], ascending and distinct (a repeated pair counts once).  A context finds its row by looking its owner
    up in keys; an owner that is not there has seen nothing."""
    owner = np.asarray(owner).astype(np.int64).reshape(-1)
    p = np.asarray(cand_pos).astype(np.int64).reshape(-1)
    if owner.shape != p.shape:
        raise ValueError('seen_index: one candidate position per owner')
    if p.size and (p.min() < 0 or p.max() >= 2 ** 31):
        raise ValueError('seen_index: candidate positions must lie in [0, 2^31)')
    pairs = np.unique(np.stack([owner, p], axis=1), axis=0) if p.size else np.zeros((0, 2), dtype=np.int64)
    if pairs.shape[0] >= 2 ** 31:
        raise ValueError('seen_index: the relation must hold fewer than 2^31 pairs')
    keys = np.unique(pairs[:, 0])
    off = np.append(np.searchsorted(pairs[:, 0], keys, side='left'), pairs.shape[0])       # np.unique sorted the pairs by owner first
    return keys, off.astype(np.int32), pairs[:, 1].astype(np.int32)


def seen_mask(off, pos, row, N, skip_in=None, nnz=None):
    """uint8 [C, N], the mask cffm_seen_mask writes: byte (c, n) is 1 where skip_in[c, n] != 0 or where n is an entry pos[j],
    lo <= j < hi, of context c's CSR row r = row[c] - lo and hi being off[r] and off[r + 1] clamped into [0, nnz] - and 0 otherwise.
    Malformed input as the kernel takes it: a row[c] outside [0, R) and a decreasing pair of offsets give no entries, entries of pos
    outside [0, N) are ignored, entries may repeat and come in any order.  nnz: the number of entries of pos that belong to the
    relation (default: all of pos); nothing at or beyond it is looked at."""
    off = np.asarray(off).astype(np.int64).reshape(-1)
    pos = np.asarray(pos).astype(np.int64).reshape(-1)
    row = np.asarray(row).astype(np.int64).reshape(-1)
    N, R = int(N), off.shape[0] - 1
    nnz = pos.shape[0] if nnz is None else int(nnz)
    if R < 0 or N < 1 or not 0 <= nnz <= pos.shape[0]:
        raise ValueError('seen_mask: needs off [R + 1], N >= 1 and 0 <= nnz <= len(pos)')
    C = row.shape[0]
    if skip_in is None:
        mask = np.zeros((C, N), dtype=np.uint8)
    else:
        skip_in = np.asarray(skip_in)
        if skip_in.shape != (C, N):
            raise ValueError('seen_mask: skip_in must be [%d, %d]' % (C, N))
        mask = (skip_in != 0).astype(np.uint8)
    for c in range(C):
        r = int(row[c])
        if not 0 <= r < R:
            continue
        lo, hi = (min(max(int(v), 0), nnz) for v in (off[r], off[r + 1]))
        p = pos[lo:hi] if hi > lo else pos[:0]
        mask[c, p[(p >= 0) & (p < N)]] = 1
    return mask
