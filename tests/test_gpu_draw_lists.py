"""cffm_draw_lists on the GPU, exact against its numpy twin (cffm_amd.spec.draw_lists) in both modes - the indices alone, and the
tuples gathered from a table of nf = 1, 2, 3 columns.  Every output sits in a guarded buffer (tests/test_gpu_rows.py Guard): canary
bytes in front of and behind a poisoned payload, so a write outside the G * (m + 1) [* nf] elements of the contract shows.  The
(U, m) cases are the smallest and the largest lists, the frappe item count, both sides of the 64-lane stride of a map lookup,
m = U - 1 (every other index drawn), and the largest U; G runs over a ragged last workgroup of the four-list workgroups."""
import functools

import numpy as np
import pytest
import torch

from cffm_amd.spec import draw_lists
from tests.test_gpu_rows import Guard, dev_of, stream

pytestmark = pytest.mark.gpu

SEED = 0x9e3779b97f4a7c15                       # a non-zero high word
CASES = [(2, 1), (5, 4), (4082, 4), (4082, 63), (4082, 64), (4082, 65), (4082, 100), (1100, 1023), (1024, 1023)]
GS = (1, 3, 4, 5, 257)
LIST0S = (0, 2 ** 40 + 3, 2 ** 32 - 2, 12345, 2 ** 62)


@functools.lru_cache(maxsize=None)
def lib():
    from cffm_amd import hip
    hip.load()
    return hip.fast()


@functools.lru_cache(maxsize=None)
def table(U, nf):
    """int32 [U, nf]: a different value in every cell, so that a wrong row or column shows."""
    u = np.arange(U, dtype=np.int64)[:, None]
    a = np.arange(nf, dtype=np.int64)[None, :]
    return ((u * 7 + a * 1000003 + 5) % (2 ** 31 - 1)).astype(np.int32)


def targets(U, G, salt=0):
    """at [G]: both ends of the skip (0 and U - 1) and values in between."""
    at = np.random.RandomState(U % 9973 + G + salt).randint(0, U, size=G).astype(np.int32)
    at[0] = 0 if G > 1 else U - 1
    at[-1] = U - 1
    return at


def run(seed, list0, at, U, m, nf=0, want_lists=True):
    """One call into guarded buffers: (lists or None, tuples or None, target) on the host, canaries and padding checked."""
    G = int(at.shape[0])
    d_at = dev_of(np.asarray(at, dtype=np.int32))
    d_cand = dev_of(table(U, nf)) if nf else None
    g_lists = Guard(G * (m + 1) * 4) if want_lists else None
    g_tuples = Guard(G * (m + 1) * nf * 4) if nf else None
    g_target = Guard(G * 4)
    rc = lib().cffm_draw_lists(seed, list0, G, d_at.data_ptr(), U, m, d_cand.data_ptr() if nf else 0, nf,
                               g_lists.ptr if want_lists else 0, g_tuples.ptr if nf else 0, g_target.ptr, stream())
    assert rc == 0, rc
    lists = g_lists.read('lists_out', np.int32).reshape(G, m + 1).copy() if want_lists else None
    tuples = g_tuples.read('tuples_out', np.int32).reshape(G, m + 1, nf).copy() if nf else None
    return lists, tuples, g_target.read('target_out', np.int32).copy()


@functools.lru_cache(maxsize=8)
def twin(seed, list0, at_bytes, U, m):
    """The reference of one (seed, list0, at, U, m), computed once for the modes that share it."""
    return draw_lists(seed, list0, np.frombuffer(at_bytes, dtype=np.int32), U, m)


def check(seed, list0, at, U, m, nf=0, want_lists=True):
    want, place = twin(seed, list0, np.asarray(at, dtype=np.int32).tobytes(), U, m)
    lists, tuples, target = run(seed, list0, at, U, m, nf, want_lists)
    assert np.array_equal(target, place)
    if want_lists:
        assert np.array_equal(lists, want)
    if nf:
        assert np.array_equal(tuples, table(U, nf)[want])
    return lists, tuples, target


@pytest.mark.parametrize('U,m', CASES, ids=['U%d-m%d' % c for c in CASES])
def test_indices_and_tuples_match_the_twin(U, m):
    for j, G in enumerate(GS):
        at = targets(U, G)
        check(SEED, LIST0S[j], at, U, m)                                        # the indices alone
        lists, tuples, _ = check(SEED, LIST0S[j], at, U, m, nf=1 + j % 3)      # nf = 1, 2, 3, 1, 2
        assert np.array_equal(tuples, table(U, 1 + j % 3)[lists])
    lists, tuples, _ = check(SEED, 7, targets(U, 5), U, m, nf=3)
    only = run(SEED, 7, targets(U, 5), U, m, nf=3, want_lists=False)            # the same tuples without the index output
    assert only[0] is None and np.array_equal(only[1], tuples)


def test_the_largest_set_indices_only():
    U, m = 2 ** 31 - 1, 7
    for j, G in enumerate(GS):
        lists, _, _ = check(SEED, LIST0S[j], targets(U, G), U, m)
        assert lists.max() > 2 ** 24                                            # the draw does reach into the set


def test_the_counter_low_word_wraps_inside_one_call():
    for U, m in ((4082, 4), (4082, 65), (2 ** 31 - 1, 7)):
        check(SEED, 2 ** 32 - 2, targets(U, 5), U, m)
        check(3, 2 ** 32 - 2, targets(U, 5, salt=1), U, m)


def test_a_target_out_of_range_gives_the_empty_row_and_leaves_its_neighbours():
    U, m, nf, G = 4082, 65, 2, 9
    at = targets(U, G)
    good = check(SEED, 40, at, U, m, nf=nf)
    bad = at.copy()
    bad[[1, 4, 8]] = (-1, U, np.iinfo(np.int32).min)
    lists, tuples, target = run(SEED, 40, bad, U, m, nf=nf)
    for g in range(G):
        if g in (1, 4, 8):
            assert target[g] == -1 and (lists[g] == -1).all() and (tuples[g] == 0).all()
        else:
            assert target[g] == good[2][g] and np.array_equal(lists[g], good[0][g]) and np.array_equal(tuples[g], good[1][g])
    bad[8] = np.iinfo(np.int32).max
    _, tuples, target = run(SEED, 40, bad, U, m, nf=nf, want_lists=False)
    assert (target[[1, 4, 8]] == -1).all() and (tuples[[1, 4, 8]] == 0).all() and np.array_equal(tuples[0], good[1][0])


def test_two_calls_give_equal_bits_and_a_split_call_the_same_lists():
    for U, m, nf in ((4082, 4, 2), (1100, 100, 1)):
        G, list0 = 257, 2 ** 32 - 130
        at = targets(U, G)
        one = run(SEED, list0, at, U, m, nf=nf)
        two = run(SEED, list0, at, U, m, nf=nf)
        assert all(np.array_equal(a, b) for a, b in zip(one, two))
        a, b = run(SEED, list0, at[:100], U, m, nf=nf), run(SEED, list0 + 100, at[100:], U, m, nf=nf)
        assert all(np.array_equal(w, np.concatenate([x, y])) for w, x, y in zip(one, a, b))
        other = run(SEED + 1, list0, at, U, m, nf=nf)
        assert not np.array_equal(other[0], one[0])


def test_engine_draw_lists():
    """HipEngine.draw_lists: device tensors of the documented shapes, equal to the twin, and the empty call."""
    from cffm_amd.engine import HipEngine
    from cffm_amd.spec import CFFMConfig, init_params
    cfg = CFFMConfig(M=50, F=4, K=8, D=8)
    eng = HipEngine(cfg, init_params(cfg, seed=1))
    U, m, G = 300, 5, 33
    at = targets(U, G)
    want, place = draw_lists(SEED, 99, at, U, m)
    cand = dev_of(table(U, 2))
    tuples, lists, target = eng.draw_lists(SEED, 99, dev_of(at), U, m, cand)
    assert tuples.dtype == lists.dtype == target.dtype == torch.int32 and tuples.shape == (G, m + 1, 2) and tuples.is_contiguous()
    assert np.array_equal(lists.cpu().numpy(), want) and np.array_equal(target.cpu().numpy(), place)
    assert np.array_equal(tuples.cpu().numpy(), table(U, 2)[want])
    none, lists2, target2 = eng.draw_lists(SEED, 99, dev_of(at).long(), U, m)
    assert none is None and torch.equal(lists2, lists) and torch.equal(target2, target)
    t0, l0, p0 = eng.draw_lists(SEED, 0, dev_of(at[:0]), U, m, cand)
    assert t0.shape == (0, m + 1, 2) and l0.shape == (0, m + 1) and p0.shape == (0,)
    for kw in (dict(m=0), dict(m=U), dict(m=1024, U=5000)):
        with pytest.raises(ValueError, match='draw_lists'):
            eng.draw_lists(SEED, 0, dev_of(at), kw.get('U', U), kw['m'])
