"""cffm_amd.spec.draw_lists, the numpy twin and specification of cffm_draw_lists: the known answer that pins the reading of the
specification, the structure of every list, coverage at m = U - 1, invariance under a split of the list range, and uniformity as
fixed-seed chi-squares (deterministic; each bound is the 99.9 % quantile of its distribution)."""
import numpy as np
import pytest

from cffm_amd.spec import draw_lists


def _negatives(lists, place, at):
    """The m negatives of every list in list order, mapped back to 0 .. U - 2 (the set without the target)."""
    G, Lg = lists.shape
    neg = lists[np.arange(Lg)[None, :] != place[:, None]].reshape(G, Lg - 1)
    return neg - (neg > at[:, None])


def test_known_answer():
    lists, place = draw_lists(3, 0, [0, 4, 2], 5, 4)
    assert lists.dtype == np.int64 and place.dtype == np.int64
    assert lists.tolist() == [[2, 3, 1, 4, 0], [0, 1, 2, 4, 3], [3, 2, 1, 0, 4]]
    assert place.tolist() == [4, 3, 1]


@pytest.mark.parametrize('U,m,G', [(2, 1, 50), (5, 4, 200), (9, 3, 300), (4082, 4, 500), (300, 100, 40), (2 ** 31 - 1, 7, 100)])
def test_every_list_holds_its_target_once_and_distinct_others(U, m, G):
    rng = np.random.RandomState(U % 1000 + m)
    at = rng.randint(0, U, size=G)
    at[0], at[-1] = 0, U - 1
    seed, list0 = int(rng.randint(0, 2 ** 31)) << 20, int(rng.randint(0, 2 ** 31)) << 7
    lists, place = draw_lists(seed, list0, at, U, m)
    assert lists.shape == (G, m + 1) and place.shape == (G,)
    assert ((lists >= 0) & (lists < U)).all() and ((place >= 0) & (place <= m)).all()
    assert (lists[np.arange(G), place] == at).all() and ((lists == at[:, None]).sum(axis=1) == 1).all()
    srt = np.sort(lists, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()


@pytest.mark.parametrize('U', [5, 1024])
def test_coverage_when_every_other_index_is_drawn(U):
    G = 64
    at = (np.arange(G) * 37) % U
    lists, _ = draw_lists(9, 12345, at, U, U - 1)
    assert (np.sort(lists, axis=1) == np.arange(U)[None, :]).all()


def test_split_invariance():
    U, m, G, G1, list0 = 50, 6, 257, 100, 2 ** 32 - 130                     # the id's low word wraps inside the first part
    at = (np.arange(G) * 11) % U
    whole = draw_lists(77, list0, at, U, m)
    a, b = draw_lists(77, list0, at[:G1], U, m), draw_lists(77, list0 + G1, at[G1:], U, m)
    assert np.array_equal(whole[0], np.concatenate([a[0], b[0]])) and np.array_equal(whole[1], np.concatenate([a[1], b[1]]))
    other = draw_lists(78, list0, at, U, m)
    assert not np.array_equal(whole[0], other[0])


def _chi2(counts, expect):
    return float(((counts - expect) ** 2 / expect).sum())


def test_ordered_triples_and_place_are_uniform():
    """210,000 lists at U = 8, m = 3: the 7 * 6 * 5 = 210 ordered triples of negatives (a subset draw would pass a set test and
    fail this one) and the 4 places.  Measured 226.45 on 209 dof and 1.00 on 3 dof."""
    G = 210000
    at = np.arange(G) % 8
    lists, place = draw_lists(1, 0, at, 8, 3)
    neg = _negatives(lists, place, at)
    counts = np.bincount(neg[:, 0] * 49 + neg[:, 1] * 7 + neg[:, 2], minlength=343)
    seen = counts[counts > 0]
    assert seen.size == 210
    assert _chi2(seen, G / 210.0) < 276
    assert _chi2(np.bincount(place, minlength=4), G / 4.0) < 16.3


def test_marginal_is_uniform_at_the_frappe_item_count():
    """81,640 lists of 4 negatives at U = 4082, ids across 2^32: the marginal over the 4081 values.  Measured 3857.3 on 4080 dof."""
    G, U = 81640, 4082
    at = (7 * np.arange(G)) % U
    lists, place = draw_lists(0x1234567890abcdef, 2 ** 32 - 5, at, U, 4)
    counts = np.bincount(_negatives(lists, place, at).ravel(), minlength=U - 1)
    assert counts.size == U - 1
    assert _chi2(counts, G * 4 / float(U - 1)) < 4360
