"""cffm_amd.spec.pick_hard, the numpy twin and specification of cffm_pick_hard: the twin against a per-list Python loop over
tests/_rank_ref.py full_order (the order written from its prose), the structure of every list, invariance under a split of the list
range, the invalid row, what the place depends on, the place's distribution as fixed-seed chi-squares (deterministic; each bound is
the 99.9 % quantile of its distribution, as in tests/test_draw_lists_ref.py), and dominance: the picked list's loss term is at least
that of the pool's first m negatives."""
import numpy as np
import pytest

from cffm_amd.spec import DRAW_TAG, DRAW_W_TAG, HARD_MAX_LP, HARD_TAG, philox4x32_10, pick_hard
from tests import _rank_ref as R

SEED = 0x9e3779b97f4a7c15
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, -1.5, 1e-45, -1e-45], dtype=np.float32)


def scores_of(kind, G, Lp, seed=0):
    rng = np.random.default_rng(seed)
    if kind == 'normal':
        return rng.standard_normal((G, Lp)).astype(np.float32)
    if kind == 'three':                                                           # quantised to 3 values: ties everywhere
        return rng.integers(-1, 2, size=(G, Lp)).astype(np.float32)
    if kind == 'special':                                                         # +-0, +-inf, NaN, denormals among ordinary values
        s = rng.standard_normal((G, Lp)).astype(np.float32)
        hit = rng.random((G, Lp)) < 0.6
        return np.where(hit, SPECIAL[rng.integers(0, SPECIAL.size, size=(G, Lp))], s)
    if kind == 'mostly_nan':                                                      # fewer than m non-NaN negatives in most lists
        s = np.full((G, Lp), np.nan, dtype=np.float32)
        keep = rng.random((G, Lp)) < 0.15
        return np.where(keep, rng.integers(-1, 2, size=(G, Lp)).astype(np.float32), s)
    if kind == 'equal':
        return np.full((G, Lp), 0.25, dtype=np.float32)
    raise KeyError(kind)


def place_of(seed, ident, m):
    w = int(philox4x32_10((ident & 0xffffffff, ident >> 32, 0, HARD_TAG), (seed & 0xffffffff, seed >> 32))[0])
    return (w * (m + 1)) >> 32


def naive(seed, list0, scores, target, m):
    G, Lp = scores.shape
    sel = np.full((G, m + 1), -1, dtype=np.int64)
    place = np.full(G, -1, dtype=np.int64)
    for g in range(G):
        t = int(target[g])
        if not 0 <= t < Lp:
            continue
        best = [int(p) for p in R.full_order(scores[g]) if p != t][:m]            # removing the positive does not reorder the rest
        pl = place_of(seed, list0 + g, m)
        for r, p in enumerate(best):
            sel[g, r + (r >= pl)] = p
        sel[g, pl] = t
        place[g] = pl
    return sel, place


def test_constants():
    assert HARD_TAG == 4 and HARD_TAG not in (0, 1, DRAW_TAG, DRAW_W_TAG) and HARD_MAX_LP == 1024


@pytest.mark.parametrize('kind', ['normal', 'three', 'special', 'mostly_nan', 'equal'])
@pytest.mark.parametrize('Lp,m', [(2, 1), (9, 3), (9, 8), (65, 63), (66, 7)])
def test_the_twin_against_a_per_list_loop(kind, Lp, m):
    G, list0 = 41, 2 ** 32 - 17
    s = scores_of(kind, G, Lp, seed=Lp + m)
    t = np.random.default_rng(5).integers(0, Lp, size=G)
    t[:2] = (0, Lp - 1)
    got = pick_hard(SEED, list0, s, t, m)
    want = naive(SEED, list0, s, t, m)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if kind == 'mostly_nan' and Lp >= 9:
        nan_free = (~np.isnan(s)).sum(axis=1) - ~np.isnan(s[np.arange(G), t])
        assert (nan_free < m).any()                                               # NaN negatives do get picked, smallest position first
    sel, place = got
    # every list holds its positive exactly once, at place, and m distinct negatives
    assert ((place >= 0) & (place <= m)).all() and np.array_equal(sel[np.arange(G), place], t)
    for g in range(G):
        assert len(set(sel[g].tolist())) == m + 1 and sel[g].min() >= 0 and sel[g].max() < Lp


def test_the_order_on_a_known_row():
    s = np.array([[-0.0, np.nan, 2.0, np.inf, 0.0, -np.inf, 2.0, np.nan, 7.0]], dtype=np.float32)
    sel, place = pick_hard(1, 0, s, [8], 8)                                       # the positive (7.0, position 8) is no negative
    neg = [int(p) for p in np.delete(sel[0], place[0])]
    assert neg == [3, 2, 6, 0, 4, 5, 1, 7]                                        # inf; 2.0 twice by position; -0 == +0; -inf; the NaNs last
    sel3, place3 = pick_hard(1, 0, s, [3], 3)                                     # the best-scored position as the positive
    assert [int(p) for p in np.delete(sel3[0], place3[0])] == [8, 2, 6] and sel3[0, place3[0]] == 3


def test_the_same_lists_under_a_split_and_other_lists_for_another_seed():
    G, Lp, m, list0 = 67, 17, 4, 2 ** 32 - 30
    s = scores_of('three', G, Lp)
    t = np.arange(G) % Lp
    whole = pick_hard(77, list0, s, t, m)
    a, b = pick_hard(77, list0, s[:26], t[:26], m), pick_hard(77, list0 + 26, s[26:], t[26:], m)
    assert all(np.array_equal(w, np.concatenate([x, y])) for w, x, y in zip(whole, a, b))
    for g in (0, 26, 66):
        one = pick_hard(77, list0 + g, s[g:g + 1], t[g:g + 1], m)
        assert np.array_equal(one[0][0], whole[0][g]) and one[1][0] == whole[1][g]
    other = pick_hard(78, list0, s, t, m)
    assert not np.array_equal(other[1], whole[1])
    assert np.array_equal(np.sort(other[0], axis=1), np.sort(whole[0], axis=1))   # the same members: only the place is drawn


def test_the_invalid_row():
    G, Lp, m = 9, 12, 5
    s = scores_of('normal', G, Lp)
    t = np.arange(G) % Lp
    good = pick_hard(3, 40, s, t, m)
    bad = t.copy()
    bad[[1, 4, 8]] = (-1, Lp, -(2 ** 31))
    sel, place = pick_hard(3, 40, s, bad, m)
    for g in range(G):
        if g in (1, 4, 8):
            assert place[g] == -1 and (sel[g] == -1).all()
        else:
            assert place[g] == good[1][g] and np.array_equal(sel[g], good[0][g])
    assert sel.dtype == place.dtype == np.int64 and sel.shape == (G, m + 1) and place.shape == (G,)
    none = pick_hard(3, 40, s, np.full(G, Lp), m)
    assert (none[0] == -1).all() and (none[1] == -1).all()
    for kw in (dict(m=0), dict(m=Lp), dict(scores=s[:, :1], m=1), dict(scores=s.astype(np.float64)), dict(scores=s[0]),
               dict(target_pool=t[:-1]), dict(scores=np.zeros((2, 1025), dtype=np.float32), target_pool=[0, 0])):
        with pytest.raises(ValueError, match='pick_hard'):
            pick_hard(**dict(dict(seed=3, list0=0, scores=s, target_pool=t, m=m), **kw))


def test_the_place_depends_on_seed_id_and_m_alone():
    G, m = 50, 4
    t = np.arange(G) % 6
    base = pick_hard(11, 1000, scores_of('normal', G, 6), t, m)[1]
    assert np.array_equal(base, pick_hard(11, 1000, scores_of('three', G, 6, seed=9), t, m)[1])          # not on the scores
    assert np.array_equal(base, pick_hard(11, 1000, scores_of('special', G, 40), (t * 5) % 40, m)[1])     # nor on Lp or the target
    assert np.array_equal(base, [place_of(11, 1000 + g, m) for g in range(G)])
    assert not np.array_equal(base, pick_hard(11, 1000, scores_of('normal', G, 6), t, 5)[1])              # on m
    assert not np.array_equal(base, pick_hard(12, 1000, scores_of('normal', G, 6), t, m)[1])              # on the seed
    assert not np.array_equal(base, pick_hard(11, 1001, scores_of('normal', G, 6), t, m)[1])              # on the id
    assert np.array_equal(base[1:], pick_hard(11, 1001, scores_of('normal', G, 6), t, m)[1][:-1])
    hi = pick_hard(11, 2 ** 40 + 7, scores_of('normal', 3, 6), [0, 1, 2], m)[1]                           # the id's high word counts
    assert np.array_equal(hi, [place_of(11, 2 ** 40 + 7 + g, m) for g in range(3)])
    assert not np.array_equal(hi, pick_hard(11, 7, scores_of('normal', 3, 6), [0, 1, 2], m)[1])


@pytest.mark.parametrize('m,bound', [(1, 10.83), (3, 16.27)])
def test_the_place_is_uniform(m, bound):
    """60,000 lists of seed 1 from id 2^33: the m + 1 places against G / (m + 1), m dof (99.9 %: 10.83 at 1 dof, 16.27 at 3).
    Measured 0.09 on 1 dof (m = 1) and 5.32 on 3 dof (m = 3)."""
    G, Lp = 60000, 5
    s = np.zeros((G, Lp), dtype=np.float32)
    place = pick_hard(1, 2 ** 33, s, np.arange(G) % Lp, m)[1]
    counts = np.bincount(place, minlength=m + 1).astype(np.float64)
    assert counts.shape == (m + 1,)
    chi2 = float(((counts - G / (m + 1.0)) ** 2 / (G / (m + 1.0))).sum())
    print('place chi-square m=%d: %.2f on %d dof' % (m, chi2, m))
    assert chi2 < bound


def _terms(scores, t, negs):
    """(BPR, softmax) term of every list in float64: mean softplus(s_n - s_t), and logsumexp over the list minus s_t."""
    s = scores.astype(np.float64)
    G = s.shape[0]
    st = s[np.arange(G), t][:, None]
    sn = np.take_along_axis(s, negs, axis=1)
    bpr = np.logaddexp(0.0, sn - st).mean(axis=1)
    soft = np.logaddexp.reduce(np.concatenate([st, sn], axis=1), axis=1) - st[:, 0]
    return bpr, soft


@pytest.mark.parametrize('kind', ['normal', 'three'])
def test_the_picked_list_dominates_the_pools_first_negatives(kind):
    """Both terms are monotone in every negative's score and the picked negatives are, rank by rank, at least the pool's first m, so
    the picked list's term is at least theirs; 1e-12 relative covers the order of the float64 summation."""
    G, Lp, m = 200, 17, 4
    s = scores_of(kind, G, Lp, seed=3) * np.float32(3)
    t = np.arange(G) % Lp
    sel, place = pick_hard(5, 0, s, t, m)
    picked = sel[np.arange(m + 1)[None, :] != place[:, None]].reshape(G, m)
    others = np.stack([np.delete(np.arange(Lp), tg) for tg in t])
    first = others[:, :m]
    hard, drawn = _terms(s, t, picked), _terms(s, t, first)
    for h, d in zip(hard, drawn):
        assert (h >= d - 1e-12 * np.abs(d)).all()
    if kind == 'normal':
        assert (hard[0] > drawn[0]).mean() > 0.9 and (hard[1] > drawn[1]).mean() > 0.9      # and it is harder, not merely no easier
    # rank by rank: the r-th picked score is at least the r-th best of ANY m negatives
    sp = np.take_along_axis(s, picked, axis=1)
    assert (np.diff(sp, axis=1) <= 0).all() and (sp >= np.sort(np.take_along_axis(s, first, axis=1), axis=1)[:, ::-1]).all()
