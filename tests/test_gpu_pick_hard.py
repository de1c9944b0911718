"""cffm_pick_hard on the GPU, exact against its numpy twin (cffm_amd.spec.pick_hard).  Every output sits in a guarded buffer
(tests/test_gpu_rows.py Guard): canary bytes in front of and behind a poisoned payload, so a write outside the G * (m + 1) [* nf]
elements of the contract shows.  The cases: both sides of the 64-lane stride, the smallest and the largest pool (Lp = 2, 63, 64, 65,
66, 1024), m = 1, Lp - 2 and Lp - 1, G over a ragged last workgroup of the four-list workgroups, scores that are all equal, quantised
to three values, full of +-0 / +-inf / NaN, and all NaN, a row stride beyond Lp with NaN poison behind every row, the positive at the
first and the last pool position and out of range, ids across 2^32, every output mode, equal bits on two calls and under a split."""
import functools

import numpy as np
import pytest
import torch

from cffm_amd.spec import pick_hard
from tests.test_gpu_rows import Guard, dev_of, stream
from tests.test_pick_hard_ref import scores_of

pytestmark = pytest.mark.gpu

SEED = 0x9e3779b97f4a7c15                       # a non-zero high word
GS = (1, 4, 5, 67)
LIST0S = (0, 2 ** 40 + 3, 2 ** 32 - 2, 12345)
KINDS = ('equal', 'three', 'special', 'all_nan')


@functools.lru_cache(maxsize=None)
def lib():
    from cffm_amd import hip
    hip.load()
    return hip.fast()


def scores(kind, G, Lp, seed=0):
    if kind == 'all_nan':
        return np.full((G, Lp), np.nan, dtype=np.float32)
    return scores_of(kind, G, Lp, seed)


def pool(G, Lp, nf):
    """(pool_lists int32 [G, Lp], pool_tuples int32 [G, Lp, max(nf, 1)]): every entry tells its (list, position, column)."""
    g, p = np.arange(G, dtype=np.int64)[:, None], np.arange(Lp, dtype=np.int64)[None, :]
    lists = ((g * 1031 + p * 7 + 11) % (2 ** 31 - 1)).astype(np.int32)
    tuples = (lists.astype(np.int64)[:, :, None] * 5 + np.arange(max(nf, 1))[None, None, :] + 1).astype(np.int32)
    return lists, tuples


def targets(G, Lp, salt=0):
    t = ((np.arange(G) * 37 + salt) % Lp).astype(np.int32)
    t[0] = 0
    if G > 1:
        t[-1] = Lp - 1
    return t


def run(seed, list0, s, t, m, nf=0, want_lists=True, pad=0):
    """One call into guarded buffers: (lists or None, tuples or None, target) on the host, canaries and padding checked.  pad > 0:
    the scores lie in rows of Lp + pad, NaN behind every row."""
    G, Lp = s.shape
    padded = np.full((G, Lp + pad), np.nan, dtype=np.float32)
    padded[:, :Lp] = s
    d_s, d_t = dev_of(padded), dev_of(np.asarray(t, dtype=np.int32))
    pl, pt = pool(G, Lp, nf)
    d_pl = dev_of(pl) if want_lists else None
    d_pt = dev_of(pt) if nf else None
    g_lists = Guard(G * (m + 1) * 4) if want_lists else None
    g_tuples = Guard(G * (m + 1) * nf * 4) if nf else None
    g_target = Guard(G * 4)
    rc = lib().cffm_pick_hard(seed, list0, G, d_s.data_ptr(), Lp + pad, Lp, d_t.data_ptr(), m, d_pl.data_ptr() if want_lists else 0,
                              d_pt.data_ptr() if nf else 0, nf, g_lists.ptr if want_lists else 0, g_tuples.ptr if nf else 0,
                              g_target.ptr, stream())
    assert rc == 0, rc
    lists = g_lists.read('lists_out', np.int32).reshape(G, m + 1).copy() if want_lists else None
    tuples = g_tuples.read('tuples_out', np.int32).reshape(G, m + 1, nf).copy() if nf else None
    return lists, tuples, g_target.read('target_out', np.int32).copy()


def expected(sel, G, Lp, nf):
    """(lists, tuples) the selection gathers from pool(): -1 / zeros for the row of a list without a target."""
    pl, pt = pool(G, Lp, nf)
    ok = sel >= 0
    at = np.maximum(sel, 0)
    lists = np.where(ok, np.take_along_axis(pl, at, axis=1), -1)
    tuples = np.where(ok[:, :, None], np.take_along_axis(pt, at[:, :, None], axis=1), 0)
    return lists, tuples


def check(seed, list0, s, t, m, nf=0, want_lists=True, pad=0, ref=None):
    G, Lp = s.shape
    sel, place = ref if ref is not None else pick_hard(seed, list0, s, t, m)
    lists, tuples, target = run(seed, list0, s, t, m, nf, want_lists, pad)
    want_l, want_t = expected(sel, G, Lp, nf)
    assert np.array_equal(target, place)
    if want_lists:
        assert np.array_equal(lists, want_l)
    if nf:
        assert np.array_equal(tuples, want_t)
    return sel, place


def ms_of(Lp):
    return sorted({1, max(1, Lp - 2), Lp - 1})


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('Lp', [2, 63, 64, 65, 66])
def test_the_pick_matches_the_twin(kind, Lp):
    for j, G in enumerate(GS):
        s, t = scores(kind, G, Lp, seed=j), targets(G, Lp, salt=j)
        for i, m in enumerate(ms_of(Lp)):
            ref = check(SEED, LIST0S[j], s, t, m, pad=(0, 3)[i % 2])                 # the indices alone
            assert (ref[1] >= 0).all()
            check(SEED, LIST0S[j], s, t, m, nf=(1, 2, 4)[(i + j) % 3], pad=(5, 0)[i % 2], ref=ref)


@pytest.mark.parametrize('kind', KINDS)
def test_the_largest_pool(kind):
    Lp = 1024
    for j, G in ((1, 5), (3, 67)):
        s, t = scores(kind, G, Lp, seed=j), targets(G, Lp, salt=j)
        for m in ((1, Lp - 1) if G == 5 else (Lp - 2,)):
            check(SEED, LIST0S[j], s, t, m, nf=(1, 2, 4)[m % 3], pad=m % 2)


def test_a_target_out_of_range_gives_the_empty_row_and_leaves_its_neighbours():
    G, Lp, m, nf = 9, 65, 7, 2
    s, t = scores('three', G, Lp), targets(G, Lp)
    good = run(SEED, 40, s, t, m, nf=nf, pad=2)
    bad = t.copy()
    bad[[1, 4, 8]] = (-1, Lp, np.iinfo(np.int32).min)
    check(SEED, 40, s, bad, m, nf=nf, pad=2)
    lists, tuples, target = run(SEED, 40, s, bad, m, nf=nf, pad=2)
    for g in range(G):
        if g in (1, 4, 8):
            assert target[g] == -1 and (lists[g] == -1).all() and (tuples[g] == 0).all()
        else:
            assert target[g] == good[2][g] and np.array_equal(lists[g], good[0][g]) and np.array_equal(tuples[g], good[1][g])
    bad[8] = np.iinfo(np.int32).max
    _, tuples, target = run(SEED, 40, s, bad, m, nf=nf, want_lists=False)
    assert (target[[1, 4, 8]] == -1).all() and (tuples[[1, 4, 8]] == 0).all() and np.array_equal(tuples[0], good[1][0])
    every = check(SEED, 40, s, np.full(G, Lp, dtype=np.int32), m, nf=nf)            # a call of invalid lists only
    assert (every[1] == -1).all()


def test_the_counter_low_word_wraps_inside_one_call():
    for Lp, m in ((17, 4), (65, 16)):
        s = scores('three', 5, Lp)
        check(SEED, 2 ** 32 - 2, s, targets(5, Lp), m)
        check(3, 2 ** 32 - 2, s, targets(5, Lp, salt=1), m)
    check(SEED, 2 ** 62, scores('special', 5, 66), targets(5, 66), 7, nf=1)


def test_every_output_mode():
    G, Lp, m = 5, 17, 4
    s, t = scores('special', G, Lp), targets(G, Lp)
    ref = pick_hard(SEED, 7, s, t, m)
    check(SEED, 7, s, t, m, nf=0, ref=ref)
    for nf in (1, 2, 4):
        check(SEED, 7, s, t, m, nf=nf, ref=ref)
        only = run(SEED, 7, s, t, m, nf=nf, want_lists=False)                       # the same tuples without the index output
        assert only[0] is None and np.array_equal(only[1], expected(ref[0], G, Lp, nf)[1]) and np.array_equal(only[2], ref[1])


def test_two_calls_give_equal_bits_and_a_split_call_the_same_lists():
    for Lp, m, nf, kind in ((17, 4, 2, 'three'), (130, 64, 1, 'special')):
        G, list0 = 67, 2 ** 32 - 30
        s, t = scores(kind, G, Lp), targets(G, Lp)
        one = run(SEED, list0, s, t, m, nf=nf)
        two = run(SEED, list0, s, t, m, nf=nf)
        assert all(np.array_equal(a, b) for a, b in zip(one, two))
        # a split call sees its own lists as 0 ..: pool() numbers by the row of the call, so compare the chosen positions
        sel = pick_hard(SEED, list0, s, t, m)
        a, b = pick_hard(SEED, list0, s[:26], t[:26], m), pick_hard(SEED, list0 + 26, s[26:], t[26:], m)
        assert all(np.array_equal(w, np.concatenate([x, y])) for w, x, y in zip(sel, a, b))
        check(SEED, list0, s[:26], t[:26], m, nf=nf, ref=a)
        check(SEED, list0 + 26, s[26:], t[26:], m, nf=nf, ref=b)
        other = run(SEED + 1, list0, s, t, m, nf=nf)
        assert not np.array_equal(other[2], one[2])


def test_engine_pick_hard():
    """HipEngine.pick_hard: device tensors of the documented shapes, the row stride passed through, equal to the twin, the empty
    call, and ValueErrors that name the method."""
    from cffm_amd.engine import HipEngine
    from cffm_amd.spec import CFFMConfig, init_params
    cfg = CFFMConfig(M=50, F=4, K=8, D=8)
    eng = HipEngine(cfg, init_params(cfg, seed=1))
    G, Lp, m = 33, 17, 4
    s, t = scores('special', G, Lp), targets(G, Lp)
    sel, place = pick_hard(SEED, 99, s, t, m)
    pl, pt = pool(G, Lp, 2)
    want_l, want_t = expected(sel, G, Lp, 2)
    wide = torch.full((G, Lp + 7), float('nan'), device='cuda')
    wide[:, :Lp] = dev_of(s)
    view = wide[:, :Lp]                                                             # row stride Lp + 7, NaN behind every row
    assert view.stride(0) == Lp + 7
    tuples, lists, target = eng.pick_hard(SEED, 99, view, dev_of(t), m, lists=dev_of(pl), tuples=dev_of(pt))
    assert tuples.dtype == lists.dtype == target.dtype == torch.int32 and tuples.shape == (G, m + 1, 2) and tuples.is_contiguous()
    assert np.array_equal(lists.cpu().numpy(), want_l) and np.array_equal(target.cpu().numpy(), place)
    assert np.array_equal(tuples.cpu().numpy(), want_t)
    none, lists2, target2 = eng.pick_hard(SEED, 99, dev_of(s), dev_of(t).long(), m, lists=dev_of(pl).long())
    assert none is None and torch.equal(lists2, lists) and torch.equal(target2, target)
    tuples3, none, target3 = eng.pick_hard(SEED, 99, dev_of(s), dev_of(t), m, tuples=dev_of(pt))
    assert none is None and torch.equal(tuples3, tuples) and torch.equal(target3, target)
    t0, l0, p0 = eng.pick_hard(SEED, 0, dev_of(s[:0]), dev_of(t[:0]), m, lists=dev_of(pl[:0]), tuples=dev_of(pt[:0]))
    assert t0.shape == (0, m + 1, 2) and l0.shape == (0, m + 1) and p0.shape == (0,)
    d_s, d_t, d_pl, d_pt = dev_of(s), dev_of(t), dev_of(pl), dev_of(pt)
    for kw in (dict(m=0), dict(m=Lp), dict(scores=d_s.double()), dict(scores=d_s[0]), dict(scores=d_s.t()), dict(target_pool=d_t[:-1]),
               dict(lists=None), dict(lists=d_pl[:, :-1]), dict(lists=None, tuples=d_pt[:, :, 0]), dict(lists=None, tuples=d_pt[:-1]),
               dict(scores=d_s[:1].expand(G, Lp)), dict(scores=d_s[:, :1], m=1)):
        with pytest.raises(ValueError, match='pick_hard'):
            eng.pick_hard(**dict(dict(seed=SEED, list0=0, scores=d_s, target_pool=d_t, m=m, lists=d_pl), **kw))
