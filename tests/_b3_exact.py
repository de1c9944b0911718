"""Exact-arithmetic cases for the three bf16x3 conv kernels (gemm_tile_b3 forward / input gradient, wgrad3_kernel; conv.hip).

Every operand value is  m * (1 | 1 + 2^-9 | 1 + 2^-9 + 2^-18)  with a small integer m: the round-to-nearest split of split_bf16x3
returns exactly the pieces m, m 2^-9, m 2^-18 (one, two or three populated pieces), every cross term is a small integer times a
power of two, and the operands are so sparse that the sum of |kept terms| of every output stays below 2^24 of its lowest bit.  Then
every partial sum in ANY order and under ANY rounding of the accumulate is exact, and a correct kernel returns the integer reference
bit for bit - the bf16x3 loop and the fp32 loop alike.  tests/test_b3_exact_cpu.py proves those three properties for every case
with a float32 replay of the split; tests/test_gpu_b3_exact.py runs the cases.

Layer 1 of a (F, D, B) shape: rows m = (b, y, x) of C[1] [B, So, So, Pp], reduction index of the forward kv = tap * P + p over the
2 x 2 patch of C[0] (tap = 2 dy + dx).  The three contractions of one case:
  fwd     z[m, q]      = sum_kv A[m, kv] W[kv, q]          A = im2col(act(C[0])) 2 nonzeros per row, W dense
  dgrad   dA[m, kv]    = sum_q  G[m, q] W[kv, q]           G = dC[1] 2 nonzeros per row
  wgrad   gW[kv, q]    = sum_m  A[m, kv] G'[m, q]          both sparse; gb[q] = sum_m G'[m, q]
A class (na, nb) gives the first operand na populated pieces and the second nb: C[0] x W, dC[1] x W, C[0] x dC[1].  Which piece
products occur:
  a1b1 (1,1)   a2b1 (2,1): + a2 b1   a1b2 (1,2): + a1 b2   a2b2 (2,2): + a2 b2   a3b1 (3,1): + a3 b1   a1b3 (1,3): + a1 b3
  six: the reduction indices take the types (3,1), (1,3), (2,2) in turn, so all six kept products occur in every long enough sum and
       the dropped bracket a2 b3 + a3 b2 + a3 b3 is identically zero.
(A third piece cannot be populated without the second - the split puts the whole remainder of the first piece into the second -, so
"a1 b1 + a3 b1 alone" does not exist; a3b1 / a1b3 are the classes in which a3 b1 / a1 b3 is the one product the previous class lacks.)

The layout walks: the nonzeros of row m sit at kv = m mod 4P and half a period further, so every (k-step, lane group, k within the
record) slot of the filter image and of the A operand - the channels next to the pad and every tap among them - carries a product for
68 rows spread over the row tiles, the first and the last included; the multipliers are hashed small integers (signs and zeros in
the filter), so a record read from the wrong slot, a skipped or a repeated term changes the integer result.

The bias gradient is a plain fp32 sum of dC[1] over all rows, so a column of a dC[1] with three populated pieces (19 significant
bits) can hold some twenty nonzeros only: the weight-gradient data of the classes a1b3 and six populate LIMITED_ROWS rows, spread
evenly over the row range (both ends and every position of a 32-row step included).  Those two classes have a second weight-gradient
data set (build(full=True)) with every row populated, so that the third piece of dC[1] reaches every (slab, step) of wgrad3; only
the weight gradient of that run is exact and checked."""
import numpy as np

E = (0.0, 1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -9 + 2.0 ** -18)
CLASSES = {'a1b1': (1, 1), 'a2b1': (2, 1), 'a1b2': (1, 2), 'a2b2': (2, 2), 'a3b1': (3, 1), 'a1b3': (1, 3), 'six': None}
SIX_TYPES = ((3, 1), (1, 3), (2, 2))
TERMS6 = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))
DROPPED = ((1, 2), (2, 1), (2, 2))
LIMITED_ROWS = 2400
LIMITED_CLASSES = ('a1b3', 'six')

# the cases of tests/test_b3_exact_cpu.py and tests/test_gpu_b3_exact.py: (shape, class, activation).  F = 16 is the smallest shape whose
# three layer-1 roles run bf16x3 (32768 rows); F = 22 (Pp = 240) is the nearest one with an odd number of 16-deep halves in the input
# gradient's reduction that still does
GEOS = {'f16-d32-b512': (16, 32, 512), 'f22-d32-b512': (22, 32, 512)}
CASES = [('f16-d32-b512', c, 'relu') for c in ('a1b1', 'a2b1', 'a1b2', 'a2b2', 'a3b1', 'a1b3', 'six')] + [
    ('f16-d32-b512', 'selu-one', 'selu'), ('f22-d32-b512', 'six', 'relu')]
SELU_SCALE32 = np.float32(1.0507009873554804934193349852946)


class Geo(object):
    def __init__(self, F, D, B):
        self.F, self.D, self.B = F, D, B
        self.P = F * (F - 1) // 2
        self.Pp = (self.P + 15) // 16 * 16
        self.Sin, self.So = D >> 1, D >> 2
        self.rows = B * self.So * self.So
        self.KV = 4 * self.P


def _h(*xs):
    """A 64-bit mix of integer arrays (broadcast)."""
    h = np.full(np.broadcast(*xs).shape, 0x9E3779B97F4A7C15, dtype=np.uint64)
    for i, x in enumerate(xs):
        h = (h ^ (np.asarray(x).astype(np.uint64) + np.uint64(i + 1))) * np.uint64(0xBF58476D1CE4E5B9)
        h = h ^ (h >> np.uint64(29))
    return h


def _types(cls, idx):
    """(na, nb) per reduction index."""
    idx = np.asarray(idx)
    if CLASSES[cls] is not None:
        na, nb = CLASSES[cls]
        return np.full(idx.shape, na), np.full(idx.shape, nb)
    t = np.array(SIX_TYPES)[idx % 3]
    return t[..., 0], t[..., 1]


_E = np.array(E)


def filter_w(g, cls, red):
    """W [KV, P] float32: hashed multipliers 1 .. 6, a fifth of them negative, one in eleven zero.  red: 'kv' (forward: the pieces of
    row kv follow the type of kv) or 'q' (input gradient: of column q)."""
    kv, q = np.arange(g.KV)[:, None], np.arange(g.P)[None, :]
    h = _h(kv, q)
    mag = 1 + (h % np.uint64(6)).astype(np.int64)
    sgn = np.where((h >> np.uint64(8)) % np.uint64(5) == 0, -1, 1)
    keep = (h >> np.uint64(16)) % np.uint64(11) != 0
    nb = np.broadcast_to(_types(cls, kv if red == 'kv' else q)[1], h.shape)
    return (mag * sgn * keep * _E[nb]).astype(np.float32), nb


def rows_a(g, cls, red='kv', mmax=3):
    """The A operand (im2col of C[0]) as (idx [rows, 2], val [rows, 2] float32): nonzeros at kv = m mod KV and half a period on.
    red: 'kv' (the pieces follow the type of kv) or 'm' (weight gradient: of the row)."""
    m = np.arange(g.rows)
    idx = np.stack([m % g.KV, (m + g.KV // 2 + m // g.KV) % g.KV], axis=1)
    mult = 1 + (_h(m[:, None], idx) % np.uint64(mmax)).astype(np.int64)
    na = np.broadcast_to(_types(cls, idx if red == 'kv' else m[:, None])[0], idx.shape)
    return idx, (mult * _E[na]).astype(np.float32), na


def rows_g(g, cls, role, red, limited=False, mmax=3):
    """dC[1] as (idx [rows, 2], val [rows, 2]): nonzeros at q = (m div KV + 2 (m mod KV)) mod P and 51 further, signs hashed.  role: 0 = it is the
    first operand (input gradient), 1 = the second (weight gradient).  red: 'q' or 'm'.  limited: only LIMITED_ROWS rows are
    populated, one nonzero each, q = (rank of the row) mod P."""
    m = np.arange(g.rows)
    if limited:
        live = np.unique(np.floor(np.arange(LIMITED_ROWS) * ((g.rows - 1) / (LIMITED_ROWS - 1.0))).astype(np.int64))
        rank = np.full(g.rows, -1)
        rank[live] = np.arange(live.size)
        idx = np.stack([np.maximum(rank, 0) % g.P, np.zeros(g.rows, dtype=np.int64)], axis=1)
        on = np.stack([rank >= 0, np.zeros(g.rows, dtype=bool)], axis=1)
    else:
        q1 = (m // g.KV + 2 * (m % g.KV)) % g.P                # with rows_a: at most four rows meet in one (kv, q) of the weight gradient
        idx = np.stack([q1, (q1 + 51) % g.P], axis=1)
        on = np.ones(idx.shape, dtype=bool)
    h = _h(m[:, None], idx, 7)
    mult = (1 + (h % np.uint64(mmax)).astype(np.int64)) * np.where((h >> np.uint64(8)) % np.uint64(4) == 0, -1, 1)
    n = np.broadcast_to(_types(cls, idx if red == 'q' else m[:, None])[role], idx.shape)
    return idx, (mult * on * _E[n]).astype(np.float32), n


def gate(g):
    """C[0] of the input-gradient run as im2col rows [rows, KV]: 1.0, one element in eight 0.0 (the gate must close there)."""
    m, kv = np.arange(g.rows)[:, None], np.arange(g.KV)[None, :]
    return (_h(m, kv, 3) % np.uint64(8) != 0).astype(np.float32)


def dt1_rows(g, unit):
    """dt1 columns of pool 1, [B, Sin]: 0 .. 3 units (the broadcast pool gradient the input gradient adds before the gate)."""
    b, h = np.arange(g.B)[:, None], np.arange(g.Sin)[None, :]
    return ((b + 2 * h) % 4).astype(np.float32) * np.float32(unit)


# ---- one case: operands, the integer reference, and what the CPU test needs to prove it exact --------------------------------------
def build(g, cls, kind, act='relu', full=False):
    """kind 'fwd' | 'dgrad' | 'wgrad'.  Returns a dict with the sparse operands ('a' = (idx, val) of the first, 'b' of the second where
    it is sparse, 'W' [KV, P] where it is the filter) - the values BEFORE the activation; 'a_act' the first operand as the kernel
    multiplies it (after act_pos4 in fp32)."""
    if act == 'selu':
        return _build_selu(g, kind)
    out = {'kind': kind, 'cls': cls, 'act': act}
    if kind == 'fwd':
        ai, av, out['a_n'] = rows_a(g, cls)
        out['W'], out['b_n'] = filter_w(g, cls, 'kv')
    elif kind == 'dgrad':
        ai, av, out['a_n'] = rows_g(g, cls, 0, 'q')
        out['W'], out['b_n'] = filter_w(g, cls, 'q')
        out['gate'] = gate(g)
        out['dt1'] = dt1_rows(g, 2.0 ** -18)
    else:
        limited = cls in LIMITED_CLASSES and not full       # full: every row populated; the bias gradient of that run is not exact
        ai, av, out['a_n'] = rows_a(g, cls, 'm', mmax=2 if limited else 3)
        bi, bv, out['b_n'] = rows_g(g, cls, 1, 'm', limited=limited, mmax=2 if limited else 3)
        out['b'] = (bi, bv)
    out['a'] = (ai, av)
    out['a_act'] = av
    return out


def _build_selu(g, kind):
    """selu: act_pos4 multiplies the A operand by the fp32 scale, which leaves a full 24-bit significand - exact sums then exist only
    for ONE term per output with the other factor a power of two.  A: one nonzero per row, 1 + j / 1024 (j < 512: below 1.6 after the scale, so that sum |pieces| stays below 2^24 lowest bits); W and dC[1]: +-2^e."""
    m = np.arange(g.rows)
    out = {'kind': kind, 'cls': 'selu-one', 'act': 'selu'}
    kv, q = np.arange(g.KV)[:, None], np.arange(g.P)[None, :]
    h = _h(kv, q, 11)
    W = (np.where((h >> np.uint64(8)) % np.uint64(3) == 0, -1.0, 1.0) * 2.0 ** ((h % np.uint64(4)).astype(np.int64) - 1)).astype(np.float32)
    idx = np.stack([m % g.KV, np.zeros(g.rows, dtype=np.int64)], axis=1)
    val = np.stack([1.0 + (_h(m, 5) % np.uint64(512)).astype(np.float64) / 1024, np.zeros(g.rows)], axis=1).astype(np.float32)
    gi = np.stack([(m // g.KV + 2 * (m % g.KV)) % g.P, np.zeros(g.rows, dtype=np.int64)], axis=1)
    hg = _h(m, 13)
    gv = np.stack([np.where((hg >> np.uint64(8)) % np.uint64(3) == 0, -1.0, 1.0) * 2.0 ** ((hg % np.uint64(4)).astype(np.int64) - 1),
                   np.zeros(g.rows)], axis=1).astype(np.float32)
    if kind == 'fwd':
        out['a'], out['W'] = (idx, val), W
        out['a_act'] = (val * SELU_SCALE32).astype(np.float32)
    elif kind == 'dgrad':                    # the A operand of the input gradient is dC[1] (no activation); the gate scales by selu'
        out['a'], out['W'] = (gi, gv), W
        out['a_act'] = gv
        out['gate'] = gate(g)
        out['dt1'] = dt1_rows(g, 0.5)
    else:
        out['a'], out['b'] = (idx, val), (gi, gv)
        out['a_act'] = (val * SELU_SCALE32).astype(np.float32)
    return out


def dense(g, sp, width):
    """(idx, val) -> [rows, width] float64."""
    idx, val = sp
    out = np.zeros((g.rows, width))
    np.add.at(out, (np.arange(g.rows)[:, None], idx), val.astype(np.float64))
    return out


def contract(g, kind, av, aidx, second):
    """The contraction of a case on given float64 values of its operands (the full values, or one piece each): av [rows, 2] with
    indices aidx; second = W [KV, P] (fwd, dgrad) or (idx, val) of dC[1] (wgrad).  Exact in float64 for the cases of this file."""
    if kind == 'fwd':
        return (av[:, :, None] * second[aidx]).sum(axis=1)                                  # [rows, P]
    if kind == 'dgrad':
        return (av[:, :, None] * second.T[aidx]).sum(axis=1)                                # [rows, KV]
    bidx, bv = second
    out = np.zeros((g.KV, g.P))
    for ta in range(aidx.shape[1]):
        for tb in range(bidx.shape[1]):
            np.add.at(out, (aidx[:, ta], bidx[:, tb]), av[:, ta] * bv[:, tb])
    return out


def expected(g, case):
    """The integer reference of a case as float64: 'z' [rows, P] (fwd, before relu), 'dA' [rows, KV] (dgrad, gated, selu' applied
    in fp32), 'gW' [KV, P] and 'gb' [P] (wgrad)."""
    kind = case['kind']
    aidx = case['a'][0]
    av = case['a_act'].astype(np.float64)
    if kind == 'fwd':
        return {'z': contract(g, kind, av, aidx, case['W'].astype(np.float64))}
    if kind == 'dgrad':
        acc = contract(g, kind, av, aidx, case['W'].astype(np.float64))
        b = np.arange(g.rows) // (g.So * g.So)
        y = (np.arange(g.rows) // g.So) % g.So
        dh = (np.arange(g.KV) // g.P) >> 1
        pre = acc + case['dt1'].astype(np.float64)[b[:, None], 2 * y[:, None] + dh[None, :]]
        pre32 = pre.astype(np.float32)
        assert np.array_equal(pre32.astype(np.float64), pre)
        gsc = SELU_SCALE32 if case['act'] == 'selu' else np.float32(1.0)
        return {'dA': ((pre32 * gsc).astype(np.float32) * case['gate']).astype(np.float64)}
    bidx, bv = case['b']
    gb = np.zeros(g.P)
    np.add.at(gb, bidx, bv.astype(np.float64))
    return {'gW': contract(g, kind, av, aidx, (bidx, bv.astype(np.float64))), 'gb': gb,
            'gb_abs': np.bincount(bidx.ravel(), weights=np.abs(bv).ravel().astype(np.float64), minlength=g.P)}


# ---- device layouts ---------------------------------------------------------------------------------------------------------------
def to_c0(g, rows_kv):
    """im2col rows [rows, KV] -> C[0] [B, Sin, Sin, Pp] float32 (pad channels zero)."""
    a = np.zeros((g.B, g.So, g.So, 2, 2, g.Pp), dtype=np.float32)
    a[..., :g.P] = rows_kv.reshape(g.B, g.So, g.So, 2, 2, g.P)
    return np.ascontiguousarray(a.transpose(0, 1, 3, 2, 4, 5)).reshape(g.B, g.Sin, g.Sin, g.Pp)


def from_c0(g, c0):
    """C[0]-shaped [B, Sin, Sin, Pp] -> im2col rows [rows, KV]."""
    a = np.asarray(c0).reshape(g.B, g.So, 2, g.So, 2, g.Pp).transpose(0, 1, 3, 2, 4, 5)
    return np.ascontiguousarray(a[..., :g.P]).reshape(g.rows, g.KV)


def to_c1(g, rows_p):
    """[rows, P] -> C[1]-shaped [B, So, So, Pp] float32."""
    a = np.zeros((g.rows, g.Pp), dtype=np.float32)
    a[:, :g.P] = rows_p
    return a.reshape(g.B, g.So, g.So, g.Pp)


def to_theta_w(g, W):
    """W [KV, P] -> the filter as theta holds it, [4][Pp][Pp] float32."""
    t = np.zeros((4, g.Pp, g.Pp), dtype=np.float32)
    t[:, :g.P, :g.P] = W.reshape(4, g.P, g.P)
    return t


# ---- the proof obligations (CPU) --------------------------------------------------------------------------------------------------
def lowbit(x):
    """The value of the lowest set bit of each float64 element (inf for zeros)."""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)
    mi = np.abs(np.ldexp(m, 53)).astype(np.int64)
    lb = (mi & -mi).astype(np.float64)
    return np.where(x != 0, np.ldexp(lb, e - 53), np.inf)


def exactness(g, case, split):
    """split(x) -> the three float64 pieces of fp32 x (the float32 replay of split_bf16x3).  Returns (kept, dropped, ratio): the sum
    of the six kept piece products, the sum of the three dropped ones, and per output sum |kept terms| / (the smallest lowest set bit
    any of its piece products can have) - the order-independent exactness condition wants ratio < 2^24."""
    kind = case['kind']
    aidx = case['a'][0]
    pa = split(case['a_act'])
    if kind == 'wgrad':
        pb = split(case['b'][1])
        sec = lambda j, f=(lambda v: v): (case['b'][0], f(pb[j]))
    else:
        pb = split(case['W'])
        sec = lambda j, f=(lambda v: v): f(pb[j])
    live = lambda terms: [(i, j) for i, j in terms if pa[i].any() and pb[j].any()]          # an unpopulated piece contributes 0
    shape = (g.KV, g.P) if kind == 'wgrad' else (g.rows, g.P if kind == 'fwd' else g.KV)
    kept = sum((contract(g, kind, pa[i], aidx, sec(j)) for i, j in live(TERMS6)), np.zeros(shape))
    dropped = sum((contract(g, kind, pa[i], aidx, sec(j)) for i, j in live(DROPPED)), np.zeros(shape))
    mag = sum((contract(g, kind, np.abs(pa[i]), aidx, sec(j, np.abs)) for i, j in live(TERMS6)), np.zeros(shape))
    # the lowest bit a piece product at reduction index k can have: (min over the pieces of a at k) x (min over the pieces of b at k)
    la = np.minimum.reduce([lowbit(p) for p in pa])
    lb = np.minimum.reduce([lowbit(p) for p in pb])
    inv_a, inv_b = np.where(np.isinf(la), 0.0, 1.0 / la), np.where(np.isinf(lb), 0.0, 1.0 / lb)
    # max over the terms of an output of 1 / (la lb), as a (max, x) contraction: replace sum by max
    if kind == 'fwd':
        inv = (inv_a[:, :, None] * inv_b[aidx]).max(axis=1)
    elif kind == 'dgrad':
        inv = (inv_a[:, :, None] * inv_b.T[aidx]).max(axis=1)
    else:
        inv = np.zeros((g.KV, g.P))
        bidx = case['b'][0]
        for ta in range(aidx.shape[1]):
            for tb in range(bidx.shape[1]):
                np.maximum.at(inv, (aidx[:, ta], bidx[:, tb]), inv_a[:, ta] * inv_b[:, tb])
    return kept, dropped, mag * inv
