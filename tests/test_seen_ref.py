"""cffm_amd.spec.seen_mask and seen_index (no GPU): the numpy twin of cffm_seen_mask against a brute-force double loop written from
the contract in include/cffm_hip.h, every rule about malformed input on its own, and the CSR build round trip."""
import numpy as np
import pytest

from cffm_amd import spec

I32_MAX = 2 ** 31 - 1


def brute(off, pos, row, N, skip_in=None, nnz=None):
    """Byte by byte, as the contract reads."""
    nnz = len(pos) if nnz is None else nnz
    R, C = len(off) - 1, len(row)
    out = np.zeros((C, N), dtype=np.uint8)
    for c in range(C):
        for n in range(N):
            if skip_in is not None and skip_in[c][n] != 0:
                out[c, n] = 1
                continue
            r = int(row[c])
            if r < 0 or r >= R:
                continue
            lo, hi = min(max(int(off[r]), 0), nnz), min(max(int(off[r + 1]), 0), nnz)
            for j in range(lo, hi):
                if int(pos[j]) == n:
                    out[c, n] = 1
    return out


def random_relation(rng, R, N, most):
    lens = rng.integers(0, most + 1, size=R)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    pos = rng.integers(0, N, size=int(off[-1])).astype(np.int32)            # unsorted, with repeats
    return off, pos


@pytest.mark.parametrize('seed,R,N,C,most', [(0, 1, 1, 3, 2), (1, 4, 7, 9, 5), (2, 6, 33, 12, 40), (3, 3, 20, 5, 0)])
def test_twin_equals_the_double_loop_on_random_relations(seed, R, N, C, most):
    rng = np.random.default_rng(seed)
    off, pos = random_relation(rng, R, N, most)
    row = rng.integers(-1, R + 1, size=C).astype(np.int32)                  # -1 and R among them: nothing seen
    skip = rng.choice(np.array([0, 0, 0, 1, 255], dtype=np.uint8), size=(C, N))
    for sk in (None, skip):
        got = spec.seen_mask(off, pos, row, N, sk)
        assert got.dtype == np.uint8 and got.shape == (C, N) and set(np.unique(got)) <= {0, 1}
        assert np.array_equal(got, brute(off, pos, row, N, sk))


def test_unsorted_and_repeated_entries():
    off, pos = np.array([0, 6]), np.array([5, 2, 5, 0, 2, 5])
    assert spec.seen_mask(off, pos, [0], 7).tolist() == [[1, 0, 1, 0, 0, 1, 0]]


@pytest.mark.parametrize('bad', [-1, 7, I32_MAX, -(2 ** 31)])
def test_entries_outside_the_candidates_are_ignored(bad):
    off, pos = np.array([0, 3]), np.array([1, bad, 6], dtype=np.int64)
    got = spec.seen_mask(off, pos, [0], 7)
    assert got.tolist() == [[0, 1, 0, 0, 0, 0, 1]] and np.array_equal(got, brute(off, pos, [0], 7))


@pytest.mark.parametrize('r', [-1, 2, I32_MAX, -(2 ** 31)])
def test_a_row_outside_the_relation_sees_nothing(r):
    off, pos = np.array([0, 2, 3]), np.array([0, 1, 2])
    got = spec.seen_mask(off, pos, [r, 1, 0], 4)
    assert got.tolist() == [[0, 0, 0, 0], [0, 0, 1, 0], [1, 1, 0, 0]]


def test_decreasing_offsets_give_an_empty_row():
    off, pos = np.array([0, 3, 1, 4]), np.array([0, 1, 2, 3])
    got = spec.seen_mask(off, pos, [0, 1, 2], 4)
    assert got.tolist() == [[1, 1, 1, 0], [0, 0, 0, 0], [0, 1, 1, 1]]
    assert np.array_equal(got, brute(off, pos, [0, 1, 2], 4))


def test_offsets_are_clamped_into_the_relation():
    pos = np.array([0, 1, 2, 3, 3, 3])
    off = np.array([-5, 2, 9, I32_MAX, -(2 ** 31)])
    # nnz = 4: rows [0, 2), [2, 4), [4, 4) and a decreasing pair; the entries 4 and 5 of pos are beyond the relation
    got = spec.seen_mask(off, pos, [0, 1, 2, 3], 5, nnz=4)
    assert got.tolist() == [[1, 1, 0, 0, 0], [0, 0, 1, 1, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    assert np.array_equal(got, brute(off, pos, [0, 1, 2, 3], 5, nnz=4))
    # the default nnz is all of pos
    assert spec.seen_mask(off, pos, [1], 5).tolist() == [[0, 0, 1, 1, 0]]
    assert spec.seen_mask(np.array([0, 0]), np.zeros(0), [0], 3, nnz=0).tolist() == [[0, 0, 0]]
    with pytest.raises(ValueError):
        spec.seen_mask(off, pos, [0], 5, nnz=7)


def test_skip_in_bytes_are_normalised():
    skip = np.array([[0, 1, 255, 0], [2, 0, 0, 128]], dtype=np.uint8)
    got = spec.seen_mask(np.array([0, 1]), np.array([3]), [0, -1], 4, skip)
    assert got.tolist() == [[0, 1, 1, 1], [1, 0, 0, 1]]
    assert not np.shares_memory(got, skip) and skip[0, 2] == 255              # the caller's mask is left alone
    with pytest.raises(ValueError):
        spec.seen_mask(np.array([0, 1]), np.array([3]), [0, -1], 4, skip[:, :3])


def test_seen_index_round_trip():
    rng = np.random.default_rng(5)
    N = 40
    owner = rng.choice(np.array([3, 11, 12, 500, 2 ** 40]), size=300)
    p = rng.integers(0, N, size=300)                                          # 300 pairs over 5 x 40 cells: many duplicates
    keys, off, pos = spec.seen_index(owner, p)
    assert keys.tolist() == sorted(set(owner.tolist())) and off.dtype == np.int32 and pos.dtype == np.int32
    assert off[0] == 0 and off[-1] == pos.size == len(set(zip(owner.tolist(), p.tolist()))) and (np.diff(off) > 0).all()
    for r in range(keys.size):
        assert (np.diff(pos[off[r]:off[r + 1]]) > 0).all()                    # ascending and distinct within a row
    # expand: owners with no pairs (7, and 4 looked up as "missing") see nothing
    ask = np.array([11, 7, 2 ** 40, 3, 4])
    at = np.searchsorted(keys, ask)
    row = np.where((at < keys.size) & (keys[np.minimum(at, keys.size - 1)] == ask), at, -1)
    mask = spec.seen_mask(off, pos, row, N)
    want = {(int(u), int(n)) for u, n in zip(owner, p) if u in ask}
    assert {(int(ask[c]), int(n)) for c, n in zip(*np.nonzero(mask))} == want
    assert not mask[1].any() and not mask[4].any()


def test_seen_index_edges():
    keys, off, pos = spec.seen_index([], [])
    assert keys.size == 0 and off.tolist() == [0] and pos.size == 0
    assert not spec.seen_mask(off, pos, [-1, 0], 3).any()
    keys, off, pos = spec.seen_index([9, 9, 9], [2, 2, 2])                    # one pair three times
    assert keys.tolist() == [9] and off.tolist() == [0, 1] and pos.tolist() == [2]
    with pytest.raises(ValueError):
        spec.seen_index([1, 2], [0])
    with pytest.raises(ValueError):
        spec.seen_index([1], [-1])
