"""cffm_amd.spec.weight_cdf and draw_lists_weighted, the numpy twin and specification of cffm_draw_lists_weighted: the structure of
every list, zero weights, invariance under a split of the list range, the incomplete row, the quantisation, the twin against a naive
per-list loop, and the distribution as fixed-seed chi-squares (deterministic; each bound is the 99.9 % quantile of its
distribution, as in tests/test_draw_lists_ref.py)."""
import itertools

import numpy as np
import pytest

from cffm_amd.spec import DRAW_TAG, DRAW_W_TAG, draw_lists_weighted, draw_weighted_cap, draw_words_weighted, philox4x32_10, weight_cdf


def _negatives(lists, place):
    """The m negatives of every list in list order."""
    G, Lg = lists.shape
    return lists[np.arange(Lg)[None, :] != place[:, None]].reshape(G, Lg - 1)


def _rank_weights(U):
    return np.arange(1, U + 1, dtype=np.float64) ** -0.75


def _chi2(counts, expect):
    return float(((counts - expect) ** 2 / expect).sum())


def test_constants():
    assert DRAW_W_TAG == 3 and DRAW_W_TAG != DRAW_TAG
    assert [draw_weighted_cap(m) for m in (1, 8, 62, 63, 64, 99, 129, 1023)] == [1024, 1024, 1024, 1024, 1536, 1536, 2048, 8704]


def test_weight_cdf_quantisation():
    rng = np.random.RandomState(1)
    for w in (np.ones(1), np.ones(66), _rank_weights(4096), np.array([0.0, 5.0, 0.0, 1e-300, 1e300]), rng.rand(1000) * (rng.rand(1000) > 0.3),
              np.array([1e4] + [1.0] * 63), np.full(2 ** 20, 1e-9)):
        cdf = weight_cdf(w)
        assert cdf.dtype == np.uint32 and cdf.shape == w.shape
        q = np.diff(np.concatenate([[0], cdf.astype(np.int64)]))
        assert (q >= 0).all() and int(cdf[-1]) <= 2 ** 32 - 1
        assert np.array_equal(q >= 1, w > 0)
        scale = (2 ** 32 - 1 - w.shape[0]) / w.sum()
        assert np.array_equal(q, np.floor(w * scale).astype(np.int64) + (w > 0))
    for bad in ([], [0.0, 0.0], [1.0, -1.0], [1.0, np.nan], [np.inf, 1.0], [[1.0, 2.0]]):
        with pytest.raises(ValueError, match='weight_cdf'):
            weight_cdf(bad)


@pytest.mark.parametrize('U,m,G,kind', [(2, 1, 50, 'ones'), (66, 65, 200, 'ones'), (130, 129, 60, 'ones'), (4082, 99, 300, 'rank'),
                                        (300, 100, 40, 'rank'), (40, 19, 200, 'even0')])
def test_every_list_holds_its_target_once_and_distinct_others(U, m, G, kind):
    w = {'ones': np.ones(U), 'rank': _rank_weights(U), 'even0': np.arange(U) % 2 * 1.0}[kind]
    rng = np.random.RandomState(U % 1000 + m)
    at = rng.randint(0, U, size=G)
    at[0], at[-1] = 0, U - 1
    seed, list0 = int(rng.randint(0, 2 ** 31)) << 20, int(rng.randint(0, 2 ** 31)) << 7
    lists, place = draw_lists_weighted(seed, list0, at, weight_cdf(w), m)
    assert lists.dtype == np.int64 and place.dtype == np.int64 and lists.shape == (G, m + 1) and place.shape == (G,)
    assert (place >= 0).all()                                                   # none of these is skewed enough for the cap
    assert ((lists >= 0) & (lists < U)).all() and (place <= m).all()
    assert (lists[np.arange(G), place] == at).all() and ((lists == at[:, None]).sum(axis=1) == 1).all()
    srt = np.sort(lists, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()
    if kind == 'even0':
        assert (_negatives(lists, place) % 2 == 1).all()                        # a zero weight is never drawn


def test_split_invariance():
    U, m, G, G1, list0 = 50, 6, 257, 100, 2 ** 32 - 130                     # the id's low word wraps inside the first part
    cdf = weight_cdf(_rank_weights(U))
    at = (np.arange(G) * 11) % U
    whole = draw_lists_weighted(77, list0, at, cdf, m)
    a, b = draw_lists_weighted(77, list0, at[:G1], cdf, m), draw_lists_weighted(77, list0 + G1, at[G1:], cdf, m)
    assert np.array_equal(whole[0], np.concatenate([a[0], b[0]])) and np.array_equal(whole[1], np.concatenate([a[1], b[1]]))
    for g in (0, 99, 100, 256):                                                 # and a list alone is the list of the whole call
        one = draw_lists_weighted(77, list0 + g, at[g:g + 1], cdf, m)
        assert np.array_equal(one[0][0], whole[0][g]) and one[1][0] == whole[1][g]
    other = draw_lists_weighted(78, list0, at, cdf, m)
    assert not np.array_equal(whole[0], other[0])
    assert np.array_equal(draw_lists_weighted(77, list0, at, cdf.view(np.int32), m)[0], whole[0])     # int32 storage is reinterpreted


def test_incomplete_and_targetless_lists_are_minus_one():
    U, m, G = 64, 8, 400
    w = np.ones(U)
    w[5] = 1e4
    cdf = weight_cdf(w)
    at = (np.arange(G) * 7) % U
    at[[3, 10, 11]] = (-1, U, 2 ** 31 - 1)
    lists, place = draw_lists_weighted(7, 0, at, cdf, m)
    short = place < 0
    assert 0.1 < short.mean() < 0.9 and short[[3, 10, 11]].all()
    assert (lists[short] == -1).all() and (lists[~short] >= 0).all()
    assert (lists[~short][np.arange((~short).sum()), place[~short]] == at[~short]).all()
    lists, place = draw_lists_weighted(7, 0, at, np.zeros(U, dtype=np.uint32), m)                 # T == 0
    assert (lists == -1).all() and (place == -1).all()
    for bad_m in (0, U):
        with pytest.raises(ValueError, match='draw_lists_weighted'):
            draw_lists_weighted(7, 0, at, cdf, bad_m)


def _naive(seed, list0, at, cdf, m):
    """One list at a time, one word at a time: the specification read aloud."""
    cdf = [int(c) for c in np.asarray(cdf).astype(np.uint64)]
    U, T, cap = len(cdf), cdf[-1], draw_weighted_cap(m)
    key = (seed & 0xffffffff, seed >> 32)
    lists, place = [], []
    for g, a in enumerate(int(v) for v in at):
        lid = list0 + g
        acc = []
        if 0 <= a < U and T > 0:
            for i in range(cap):
                w = int(philox4x32_10((lid & 0xffffffff, lid >> 32, i >> 2, 3), key)[i & 3])
                r = (w * T) >> 32
                j = min(sum(1 for c in cdf if c <= r), U - 1)
                if j != a and j not in acc:
                    acc.append(j)
                    if len(acc) == m:
                        break
        if len(acc) < m:
            lists.append([-1] * (m + 1))
            place.append(-1)
            continue
        p = (int(philox4x32_10((lid & 0xffffffff, lid >> 32, 0xffffffff, 3), key)[0]) * (m + 1)) >> 32
        lists.append(acc[:p] + [a] + acc[p:])
        place.append(p)
    return np.array(lists), np.array(place)


@pytest.mark.parametrize('U,m,G,kind', [(12, 11, 60, 'ones'), (30, 4, 120, 'rank'), (16, 5, 120, 'spike')])
def test_the_twin_is_the_naive_loop(U, m, G, kind):
    w = {'ones': np.ones(U), 'rank': _rank_weights(U), 'spike': np.where(np.arange(U) == 2, 3e3, 1.0)}[kind]
    cdf = weight_cdf(w)
    at = (np.arange(G) * 5 + 1) % (U + 1) - (np.arange(G) % 17 == 0)           # some -1 and some U among them
    seed, list0 = 0xfeedface12345678, 2 ** 32 - 40
    got = draw_lists_weighted(seed, list0, at, cdf, m)
    want = _naive(seed, list0, at, cdf, m)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if kind == 'spike':
        assert 0 < (got[1] < 0).sum() < G
    words = draw_words_weighted(seed, [list0 + 3], 8)[0]
    assert int(words[5]) == int(philox4x32_10(((list0 + 3) & 0xffffffff, (list0 + 3) >> 32, 1, 3), (seed & 0xffffffff, seed >> 32))[1])


def test_the_first_negative_is_drawn_in_proportion_to_the_weights():
    """60,000 lists at U = 8, weights 1 .. 8, m = 1: for each of the 8 targets the first negative against w_j / (W - w_at); the eight
    chi-squares of 6 dof each add up to one of 48 dof (99.9 %: 84.0).  Measured 47.79 on 48 dof; the place 1.60 on 1 dof."""
    G, U = 60000, 8
    w = np.arange(1.0, 9.0)
    at = np.arange(G) % U
    lists, place = draw_lists_weighted(1, 0, at, weight_cdf(w), 1)
    assert (place >= 0).all()
    neg = _negatives(lists, place)[:, 0]
    total = 0.0
    for a in range(U):
        counts = np.bincount(neg[at == a], minlength=U).astype(np.float64)
        assert counts[a] == 0
        keep = np.arange(U) != a
        total += _chi2(counts[keep], (at == a).sum() * w[keep] / w[keep].sum())
    assert total < 84.0
    assert _chi2(np.bincount(place, minlength=2), G / 2.0) < 10.83             # the place, 1 dof


def test_ordered_pairs_follow_successive_sampling():
    """120,000 lists at U = 6, weights 1 .. 6, target 0, m = 2: the 5 * 4 = 20 ordered pairs (j1, j2) against
    w_j1 / W' * w_j2 / (W' - w_j1), W' the weight without the target: 19 dof (99.9 %: 43.8); the 3 places: 2 dof (13.8).  Measured 13.95 and 0.13."""
    G, U = 120000, 6
    w = np.arange(1.0, 7.0)
    at = np.zeros(G, dtype=np.int64)
    lists, place = draw_lists_weighted(2, 2 ** 33, at, weight_cdf(w), 2)
    assert (place >= 0).all()
    neg = _negatives(lists, place)
    counts = np.bincount(neg[:, 0] * U + neg[:, 1], minlength=U * U).astype(np.float64)
    rest = w[1:].sum()
    expect = np.zeros(U * U)
    for j1, j2 in itertools.permutations(range(1, U), 2):
        expect[j1 * U + j2] = G * w[j1] / rest * w[j2] / (rest - w[j1])
    assert (counts[expect == 0] == 0).all()
    assert _chi2(counts[expect > 0], expect[expect > 0]) < 43.8
    assert _chi2(np.bincount(place, minlength=3), G / 3.0) < 13.8
