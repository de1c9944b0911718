"""cffm_draw_lists_weighted on the GPU, exact against its numpy twin (cffm_amd.spec.draw_lists_weighted).  Every output sits in a
guarded buffer (tests/test_gpu_rows.py Guard): canary bytes in front of and behind a poisoned payload, so a write outside the
G * (m + 1) [* nf] elements of the contract shows.  The cases: both sides of the 64-word round and of the four-entry read of the
accepted set (m = 1, 63, 64, 65), every other index drawn (m = U - 1), the longest list (m = 1023), weights so skewed that the word
cap leaves lists incomplete, zero weights, the deepest search (U = 2^20), a full and an empty cdf, targets out of range, ids across
2^32, every output mode; G runs over a ragged last workgroup of the four-list workgroups."""
import functools

import numpy as np
import pytest
import torch

from cffm_amd.spec import draw_lists_weighted, draw_weighted_cap, weight_cdf
from tests.test_gpu_draw_lists import table, targets
from tests.test_gpu_rows import Guard, dev_of, stream

pytestmark = pytest.mark.gpu

SEED = 0x9e3779b97f4a7c15                       # a non-zero high word
GS = (1, 4, 5, 67)
LIST0S = (0, 2 ** 40 + 3, 2 ** 32 - 2, 12345)


@functools.lru_cache(maxsize=None)
def lib():
    from cffm_amd import hip
    hip.load()
    return hip.fast()


@functools.lru_cache(maxsize=None)
def cdf_of(kind, U):
    r = np.arange(1, U + 1, dtype=np.float64)
    w = {'rank': r ** -0.75, 'uniform': np.ones(U), 'spike': np.where(r == 3, 1e4, 1.0), 'even0': (r - 1) % 2}[kind]
    return weight_cdf(w)


def run(seed, list0, at, cdf, m, nf=0, want_lists=True):
    """One call into guarded buffers: (lists or None, tuples or None, target) on the host, canaries and padding checked."""
    G, U = int(at.shape[0]), int(cdf.shape[0])
    d_at = dev_of(np.asarray(at, dtype=np.int32))
    d_cdf = dev_of(np.asarray(cdf, dtype=np.uint32).view(np.int32))
    d_cand = dev_of(table(U, nf)) if nf else None
    g_lists = Guard(G * (m + 1) * 4) if want_lists else None
    g_tuples = Guard(G * (m + 1) * nf * 4) if nf else None
    g_target = Guard(G * 4)
    rc = lib().cffm_draw_lists_weighted(seed, list0, G, d_at.data_ptr(), U, m, d_cdf.data_ptr(), d_cand.data_ptr() if nf else 0, nf,
                                        g_lists.ptr if want_lists else 0, g_tuples.ptr if nf else 0, g_target.ptr, stream())
    assert rc == 0, rc
    lists = g_lists.read('lists_out', np.int32).reshape(G, m + 1).copy() if want_lists else None
    tuples = g_tuples.read('tuples_out', np.int32).reshape(G, m + 1, nf).copy() if nf else None
    return lists, tuples, g_target.read('target_out', np.int32).copy()


def gathered(U, nf, want):
    """table[want] with the zero row of a list without a target."""
    return np.where((want >= 0)[:, :, None], table(U, nf)[np.maximum(want, 0)], 0)


def check(seed, list0, at, cdf, m, nf=0, want_lists=True, ref=None):
    want, place = ref if ref is not None else draw_lists_weighted(seed, list0, at, cdf, m)
    lists, tuples, target = run(seed, list0, at, cdf, m, nf, want_lists)
    assert np.array_equal(target, place)
    if want_lists:
        assert np.array_equal(lists, want)
    if nf:
        assert np.array_equal(tuples, gathered(int(cdf.shape[0]), nf, want))
    return want, place


@pytest.mark.parametrize('m', [1, 63, 64, 65])
def test_popularity_weights_match_the_twin(m):
    U, cdf = 4096, cdf_of('rank', 4096)
    for j, G in enumerate(GS):
        at = targets(U, G)
        ref = check(SEED, LIST0S[j], at, cdf, m)                                 # the indices alone
        assert (ref[1] >= 0).all()
        check(SEED, LIST0S[j], at, cdf, m, nf=1 + j % 3, ref=ref)


def test_every_other_index_drawn():
    U, m, cdf = 66, 65, cdf_of('uniform', 66)
    for j, G in enumerate(GS):
        want, place = check(SEED, LIST0S[j], targets(U, G), cdf, m, nf=2)
        assert (place >= 0).all() and (np.sort(want, axis=1) == np.arange(U)[None, :]).all()     # the twin completes every list


def test_the_longest_list():
    U, m, cdf = 4096, 1023, cdf_of('rank', 4096)
    for j, G in enumerate((5, 67)):
        _, place = check(SEED, LIST0S[j], targets(U, G), cdf, m, nf=1)
        assert (place >= 0).all()


def test_skewed_weights_leave_the_same_lists_incomplete():
    U, m, G, cdf = 64, 8, 67, cdf_of('spike', 64)
    at = targets(U, G)
    want, place = draw_lists_weighted(SEED, 5, at, cdf, m)
    share = float((place < 0).mean())
    assert 0.1 < share < 0.9, share                                             # on the twin: the cap does bite, and not always
    assert (want[place < 0] == -1).all()
    lists, tuples, target = run(SEED, 5, at, cdf, m, nf=3)
    assert np.array_equal(target < 0, place < 0)
    assert np.array_equal(target, place) and np.array_equal(lists, want) and np.array_equal(tuples, gathered(U, 3, want))
    assert (tuples[place < 0] == 0).all()


def test_zero_weights_are_never_drawn():
    U, m, cdf = 40, 19, cdf_of('even0', 40)
    at = targets(U, 67)
    want, place = check(SEED, 9, at, cdf, m, nf=1)
    assert (place >= 0).all()
    neg = want[np.arange(m + 1)[None, :] != place[:, None]]
    assert (neg % 2 == 1).all()


def test_a_single_tuple_is_refused():
    d = dev_of(np.zeros(4, dtype=np.int32))
    for m in (1, 0):
        assert lib().cffm_draw_lists_weighted(1, 0, 1, d.data_ptr(), 1, m, d.data_ptr(), 0, 0, d.data_ptr(), 0, d.data_ptr(), stream()) == 10001


def test_the_deepest_search():
    U, cdf = 2 ** 20, cdf_of('rank', 2 ** 20)
    for j, (G, m) in enumerate(((5, 4), (67, 65))):
        want, place = check(SEED, LIST0S[j], targets(U, G), cdf, m, nf=2)
        assert (place >= 0).all() and want.max() > 2 ** 16                       # the draw does reach into the set


def test_a_full_and_an_empty_cdf():
    full = np.array([2 ** 30, 2 ** 31, 2 ** 31, 3 * 2 ** 30, 2 ** 32 - 1, 2 ** 32 - 1], dtype=np.uint32)   # T = 2^32 - 1; 2 and 5 hold nothing
    at = np.array([0, 1, 2, 3, 4, 5, 0, 3, 5], dtype=np.int32)
    for m in (1, 2, 3):
        want, place = check(SEED, 3, at, full, m, nf=1)
        assert (place >= 0).any()
        assert not np.isin(np.where(want == at[:, None], -1, want), (2, 5)).any()
    empty = np.zeros(9, dtype=np.uint32)
    want, place = check(SEED, 3, at, empty, 3, nf=2)
    assert (place == -1).all() and (want == -1).all()


def test_a_target_out_of_range_gives_the_empty_row_and_leaves_its_neighbours():
    U, m, nf, G, cdf = 4096, 65, 2, 9, cdf_of('rank', 4096)
    at = targets(U, G)
    good = run(SEED, 40, at, cdf, m, nf=nf)
    bad = at.copy()
    bad[[1, 4, 8]] = (-1, U, np.iinfo(np.int32).min)
    want, place = check(SEED, 40, bad, cdf, m, nf=nf)
    lists, tuples, target = run(SEED, 40, bad, cdf, m, nf=nf)
    for g in range(G):
        if g in (1, 4, 8):
            assert target[g] == -1 and (lists[g] == -1).all() and (tuples[g] == 0).all()
        else:
            assert target[g] == good[2][g] and np.array_equal(lists[g], good[0][g]) and np.array_equal(tuples[g], good[1][g])
    bad[8] = np.iinfo(np.int32).max
    _, tuples, target = run(SEED, 40, bad, cdf, m, nf=nf, want_lists=False)
    assert (target[[1, 4, 8]] == -1).all() and (tuples[[1, 4, 8]] == 0).all() and np.array_equal(tuples[0], good[1][0])


def test_the_counter_low_word_wraps_inside_one_call():
    for U, m in ((4096, 4), (4096, 65)):
        check(SEED, 2 ** 32 - 2, targets(U, 5), cdf_of('rank', U), m)
        check(3, 2 ** 32 - 2, targets(U, 5, salt=1), cdf_of('rank', U), m)
    check(SEED, 2 ** 62, targets(66, 5), cdf_of('uniform', 66), 7)


def test_every_output_mode():
    U, m, cdf = 300, 5, cdf_of('rank', 300)
    at = targets(U, 5)
    ref = draw_lists_weighted(SEED, 7, at, cdf, m)
    check(SEED, 7, at, cdf, m, nf=0, ref=ref)
    for nf in (1, 3):
        check(SEED, 7, at, cdf, m, nf=nf, ref=ref)
        only = run(SEED, 7, at, cdf, m, nf=nf, want_lists=False)                # the same tuples without the index output
        assert only[0] is None and np.array_equal(only[1], gathered(U, nf, ref[0])) and np.array_equal(only[2], ref[1])


def test_two_calls_give_equal_bits_and_a_split_call_the_same_lists():
    for U, m, nf, kind in ((4096, 4, 2, 'rank'), (64, 8, 1, 'spike')):
        G, list0, cdf = 67, 2 ** 32 - 30, cdf_of(kind, U)
        at = targets(U, G)
        one = run(SEED, list0, at, cdf, m, nf=nf)
        two = run(SEED, list0, at, cdf, m, nf=nf)
        assert all(np.array_equal(a, b) for a, b in zip(one, two))
        a, b = run(SEED, list0, at[:26], cdf, m, nf=nf), run(SEED, list0 + 26, at[26:], cdf, m, nf=nf)
        assert all(np.array_equal(w, np.concatenate([x, y])) for w, x, y in zip(one, a, b))
        other = run(SEED + 1, list0, at, cdf, m, nf=nf)
        assert not np.array_equal(other[0], one[0])


def test_engine_draw_lists_weighted():
    """HipEngine.draw_lists_weighted: device tensors of the documented shapes, equal to the twin, and the empty call."""
    from cffm_amd.engine import HipEngine
    from cffm_amd.spec import CFFMConfig, init_params
    cfg = CFFMConfig(M=50, F=4, K=8, D=8)
    eng = HipEngine(cfg, init_params(cfg, seed=1))
    U, m, G = 300, 5, 33
    cdf = cdf_of('rank', U)
    at = targets(U, G)
    want, place = draw_lists_weighted(SEED, 99, at, cdf, m)
    cand, d_cdf = dev_of(table(U, 2)), dev_of(cdf.view(np.int32))
    tuples, lists, target = eng.draw_lists_weighted(SEED, 99, dev_of(at), d_cdf, m, cand)
    assert tuples.dtype == lists.dtype == target.dtype == torch.int32 and tuples.shape == (G, m + 1, 2) and tuples.is_contiguous()
    assert np.array_equal(lists.cpu().numpy(), want) and np.array_equal(target.cpu().numpy(), place)
    assert np.array_equal(tuples.cpu().numpy(), table(U, 2)[want])
    none, lists2, target2 = eng.draw_lists_weighted(SEED, 99, dev_of(at).long(), d_cdf.view(torch.uint32), m)
    assert none is None and torch.equal(lists2, lists) and torch.equal(target2, target)
    t0, l0, p0 = eng.draw_lists_weighted(SEED, 0, dev_of(at[:0]), d_cdf, m, cand)
    assert t0.shape == (0, m + 1, 2) and l0.shape == (0, m + 1) and p0.shape == (0,)
    for bad_m in (0, U, 1024):
        with pytest.raises(ValueError, match='draw_lists_weighted'):
            eng.draw_lists_weighted(SEED, 0, dev_of(at), d_cdf, bad_m)
    with pytest.raises(ValueError, match='cdf'):
        eng.draw_lists_weighted(SEED, 0, dev_of(at), d_cdf.float(), m)
    assert draw_weighted_cap(m) == 1024
