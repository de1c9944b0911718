"""Helpers of the logQ tests (cffm_list_loss_logq, cffm_amd.spec.list_loss_logq): the exact enumeration of successive sampling without
replacement that the consistency check runs on, the full-softmax gradient it is measured against, and the inputs the device tests
share.  No test lives here."""
import itertools

import numpy as np

from cffm_amd import spec


# ---- exact enumeration ------------------------------------------------------------------------------------------------------------
def ordered_draws(w, t, m):
    """Every ordered draw of m distinct negatives from the set without t, each with its probability under successive sampling in
    proportion to w: [(negatives tuple, probability)]."""
    w = np.asarray(w, dtype=np.float64)
    others = [j for j in range(w.shape[0]) if j != t]
    rest = float(w[others].sum())
    out = []
    for neg in itertools.permutations(others, m):
        p, left = 1.0, rest
        for j in neg:
            p *= w[j] / left
            left -= w[j]
        out.append((neg, p))
    return out


def full_softmax_grad(scores, t):
    """d/ds of -log softmax(s)_t over the whole catalogue, float64 [U]."""
    s = np.asarray(scores, dtype=np.float64)
    e = np.exp(s - s.max())
    g = e / e.sum()
    g[t] -= 1.0
    return g


def expected_sampled_grad(scores, t, w, m, corr):
    """(E[gradient of the sampled loss with respect to all U scores], the sum of the draws' probabilities): every ordered draw of
    ordered_draws(w, t, m) as the list (t, negatives) through spec.list_loss_logq with the table corr, its dout scattered to the
    catalogue and weighted by the draw's probability."""
    s = np.asarray(scores, dtype=np.float64)
    draws = ordered_draws(w, t, m)
    lists = np.array([(t,) + neg for neg, _ in draws], dtype=np.int64)
    prob = np.array([p for _, p in draws])
    G = lists.shape[0]
    _, dout, _ = spec.list_loss_logq(s[lists], np.zeros(G, dtype=np.int64), lists, corr)
    grad = np.zeros(s.shape[0])
    np.add.at(grad, lists.reshape(-1), (dout * G * prob[:, None]).reshape(-1))          # dout carries the 1 / G of the mean
    return grad, float(prob.sum())


# ---- the inputs of the device tests -----------------------------------------------------------------------------------------------
def table(U, seed, span=19.0):
    """fp32 [U, 2]: column 0 over [-span, span] (both signs), column 1 over [-1, 0] as log(1 - q) is: |c| up to span + 1."""
    rng = np.random.default_rng(seed)
    c = np.empty((U, 2), dtype=np.float32)
    c[:, 0] = rng.uniform(-span, span, size=U)
    c[:, 1] = -rng.uniform(0.0, 1.0, size=U)
    if U >= 2:
        c[0, 0], c[1, 0] = span, -span
    return c


def make_inputs(G, Lg, U, seed=0):
    """(scores fp32 [G, Lg], target int32 [G], lists int32 [G, Lg], corr fp32 [U, 2]).  Targets first, last, middle; indices drawn
    with repetition (at U = 2 nothing else is possible beyond Lg = 2); list 1, where there is one, holds one index Lg times; list 3
    has the two extreme corrections at its two ends.  The scores carry their own correction, s = N(0, 1) + c, so that z = s - c is
    a list of N(0, 1) while c spans +-20: a correction dropped, doubled or of the wrong sign moves z by up to 40, and no list is
    saturated.  A saturated list has p_t = 1 - 1e-6 or so, and the float32 p_t - 1 of the header's formula - the arithmetic
    cffm_list_loss is bound to, bit for bit - then holds dout[t] to 6e-8 / G absolutely, not to 1e-5 of itself.  The criterion of
    tests/test_gpu_list_loss.py cannot hold such a row: its row sum wants 1 - p_t >= 3e-3, which at Lg = 2 is |z_0 - z_1| < 5.8 -
    four standard deviations of the difference of two N(0, 1), and not three of two N(0, 2)."""
    rng = np.random.default_rng(seed + 1000 * G + 10 * Lg + U)
    noise = rng.standard_normal((G, Lg))
    t = np.array([(0, Lg - 1, Lg // 2)[g % 3] for g in range(G)], dtype=np.int32)
    lists = rng.integers(0, U, size=(G, Lg)).astype(np.int32)
    if G >= 2:
        lists[1, :] = lists[1, 0]
    if G >= 4:
        lists[3, 0], lists[3, Lg - 1] = 0, min(1, U - 1)              # the extreme corrections, at both ends of a list
    corr = table(U, seed + U)
    c = corr[lists, 0].astype(np.float64) - corr[lists[np.arange(G), t], 1].astype(np.float64)[:, None]
    c[np.arange(G), t] = 0.0
    return (noise + c).astype(np.float32), t, lists, corr
