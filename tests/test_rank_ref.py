"""The numpy references of the ranking kernels (tests/_rank_ref.py) against answers written out by hand, the 64-bit sort key of
include/cffm_hip.h against the lexsort order on random vectors over the special values, and CFFM.ranking_metrics against
hand-computed HR / NDCG.  No GPU."""
import math

import numpy as np
import pytest

from cffm_amd.CFFM import ranking_metrics
from tests import _rank_ref as R

NAN, INF = float('nan'), float('inf')
NB = R.NAN_BITS


def f32(*v):
    return np.array(v, dtype=np.float32)


def test_expand_by_hand():
    ctx = np.array([[10, 11, 12], [20, 21, 22]], dtype=np.int32)
    cand = np.array([7, 8, 9], dtype=np.int32)
    assert R.expand_ref(ctx, 1, cand, 0, 6).tolist() == [[10, 7, 12], [10, 8, 12], [10, 9, 12], [20, 7, 22], [20, 8, 22], [20, 9, 22]]
    assert R.expand_ref(ctx, 0, cand, 2, 2).tolist() == [[9, 11, 12], [7, 21, 22]]          # a cut across two contexts
    assert R.expand_ref(ctx, 2, cand, 5, 1).tolist() == [[20, 21, 9]]


def test_ties_go_to_the_smaller_position():
    s = f32(1, 3, 3, 2, 3)[None]
    idx, val, count = R.topk_ref(s, 4)
    assert idx.tolist() == [[1, 2, 4, 3]] and count.tolist() == [4]
    assert val.tolist() == [R.bits(f32(3, 3, 3, 2)).tolist()]
    assert R.rank_ref(s, [4]).tolist() == [2] and R.rank_ref(s, [0]).tolist() == [4]


def test_signed_zeros_are_equal_and_keep_their_bits():
    s = f32(-0.0, 0.0, -1, 0.0, -0.0)[None]
    idx, val, count = R.topk_ref(s, 5)
    assert idx.tolist() == [[0, 1, 3, 4, 2]]
    assert val.tolist() == [[0x80000000, 0, 0, 0x80000000, 0xbf800000]]                      # the score's own bits come back
    assert R.rank_ref(s, [3]).tolist() == [2]


def test_infinities_and_nan_last_but_still_a_candidate():
    s = f32(NAN, -INF, 5, INF, NAN, -3)[None]
    idx, val, count = R.topk_ref(s, 6)
    assert idx.tolist() == [[3, 2, 5, 1, 0, 4]] and count.tolist() == [6]                    # NaN below -inf, NaNs by position
    assert val[0, 4] == R.bits(s)[0, 0] and np.isnan(val[0, 4:].view(np.float32)).all()
    assert R.rank_ref(s, [0]).tolist() == [4] and R.rank_ref(s, [4]).tolist() == [5] and R.rank_ref(s, [1]).tolist() == [3]


def test_all_equal_is_the_identity_order():
    s = np.full((2, 7), 0.25, dtype=np.float32)
    idx, _, count = R.topk_ref(s, 3)
    assert idx.tolist() == [[0, 1, 2], [0, 1, 2]] and count.tolist() == [3, 3]
    assert R.rank_ref(s, [6, 0]).tolist() == [6, 0]


def test_k_beyond_the_candidates_left_pads():
    s = f32(4, 9, 1, 7)[None]
    skip = np.array([[0, 1, 0, 1]], dtype=np.uint8)
    idx, val, count = R.topk_ref(s, 5, skip)
    assert idx.tolist() == [[0, 2, -1, -1, -1]] and count.tolist() == [2]
    assert val.tolist() == [[0x40800000, 0x3f800000, NB, NB, NB]]
    idx, val, count = R.topk_ref(s, 2, np.ones((1, 4), dtype=np.uint8))                      # everything skipped
    assert idx.tolist() == [[-1, -1]] and val.tolist() == [[NB, NB]] and count.tolist() == [0]


def test_skipped_target_and_target_out_of_range():
    s = f32(4, 9, 1, 3)[None]
    skip = np.array([[0, 1, 0, 1]], dtype=np.uint8)
    assert R.rank_ref(s, [3], skip).tolist() == [1]        # its own flag is ignored: only 4 (position 0) is ahead, 9 is skipped
    assert R.rank_ref(s, [1], skip).tolist() == [0]
    assert R.rank_ref(s, [2], skip).tolist() == [1]
    assert R.rank_ref(s, [-1], skip).tolist() == [-1] and R.rank_ref(s, [4]).tolist() == [-1]


def test_key64_sorted_descending_is_the_lexsort_order():
    rng = np.random.default_rng(5)
    special = np.array([0.0, -0.0, 1.5, -1.5, INF, -INF, NAN, 1e-45, -1e-45, 3.0], dtype=np.float32)
    for trial in range(2000):
        n = int(rng.integers(1, 40))
        s = special[rng.integers(0, special.size, size=n)]
        skip = (rng.random(n) < 0.3).astype(np.uint8) if trial % 2 else None
        key = R.key64(s, skip)
        live = np.nonzero(key)[0]
        assert live.size == (n if skip is None else int((skip == 0).sum()))                   # only a skipped candidate has key 0
        assert np.unique(key[live]).size == live.size
        by_key = live[np.argsort(key[live])[::-1]]
        assert by_key.tolist() == R.order_ref(s, skip).tolist(), (s, skip)


def test_ranking_metrics_by_hand():
    hr, ndcg = ranking_metrics([0, 1, 9, 10, 50], 10)
    assert hr == pytest.approx(3 / 5, abs=1e-15)
    assert ndcg == pytest.approx((1.0 + 1.0 / math.log2(3.0) + 1.0 / math.log2(11.0)) / 5, abs=1e-15)
    assert ranking_metrics([3], 3) == (0.0, 0.0) and ranking_metrics([2], 3) == (1.0, 0.5)
    assert ranking_metrics([-1, 0], 1) == (0.5, 0.5)                                          # a target that was no candidate
    got = ranking_metrics(np.array([5, 0, 2, 7], dtype=np.int32), 6)
    assert got == pytest.approx(R.metrics_ref([5, 0, 2, 7], 6), abs=1e-15)
    with pytest.raises(ValueError):
        ranking_metrics([], 5)
