"""GPU: cffm_seen_mask (cffm_amd/csrc/seen.hip) through the C ABI, bit for bit against cffm_amd.spec.seen_mask.

Every output sits in a Guard of tests/test_gpu_rows.py - canaries on both sides, a NaN poison payload - and the WHOLE payload is
compared with an image of what it must hold: the twin's bytes in [0, N) of every row, the poison everywhere else, the bytes
[N, mask_stride) of a row included.  off, pos and row sit in Guards too, and behind the last entry each of them may read lie LIVE
TRAPS the twin never sees: pos holds TRAP more in-range positions beyond nnz, off two more offsets that select them, row an entry
that names a real CSR row.  A read past the end of an array therefore changes the mask instead of fetching a harmless poison value.

Shapes: N around the 16-byte slot (15, 16, 17), around the 4096-position chunk (4095, 4096, 4097) and over several chunks (8200), with
rows that start 16-byte aligned (mask_stride = N a multiple of 16) and rows that do not (N + 5, and odd N), the output begun 0 or 3
bytes into the payload, and the caller's mask absent, in rows of N + 3 bytes (another alignment than the output's: the byte path) and
in rows of the output's own stride (the same alignment: the vector path, what HipEngine.seen_mask does)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cffm_amd import spec  # noqa: E402
from oracle import rows_check as rc  # noqa: E402
from tests.test_gpu_rows import Guard, dev_of, stream  # noqa: E402

pytestmark = pytest.mark.gpu

I32_MAX = 2 ** 31 - 1
TRAP = 8                                            # live entries behind the end of pos


@functools.lru_cache(maxsize=None)
def lib():
    from cffm_amd import hip
    hip.load()
    return hip.fast()


def guarded(values, dtype=np.int32):
    """values on the device inside a Guard whose payload is exactly theirs (padded to whole words with zeros)."""
    a = np.ascontiguousarray(values, dtype=dtype).reshape(-1).view(np.uint8)
    a = np.concatenate([a, np.zeros(-a.size % 4, dtype=np.uint8)])
    g = Guard(max(a.size, 4))
    if a.size:
        g.view(torch.uint8)[:a.size].copy_(dev_of(a))
    return g


def poison_bytes(n):
    return np.resize(np.array([rc.POISON], dtype=np.uint32).view(np.uint8), n)


class Relation(object):
    """off [R + 1], pos [nnz] and row [C] as the twin sees them, and on the device with the traps behind them."""

    def __init__(self, off, pos, row, N, trap_rng=None, null_pos=False):
        self.off, self.pos, self.row = (np.asarray(a, dtype=np.int64) for a in (off, pos, row))
        self.R, self.nnz, self.C, self.N = len(off) - 1, len(pos), len(row), N
        rng = trap_rng or np.random.default_rng(0)
        trap = rng.integers(0, N, size=TRAP)
        self.d_pos = None if null_pos else guarded(np.concatenate([self.pos, trap]))
        self.d_off = guarded(np.concatenate([self.off, [self.nnz, self.nnz + TRAP]]))     # off[R + 1], off[R + 2]: never read
        self.d_row = guarded(np.concatenate([self.row, [0 if self.R else -1]]))

    def twin(self, skip=None):
        return spec.seen_mask(self.off, self.pos, self.row, self.N, skip)


def run(rel, mask_stride, skip=None, skip_stride=None, lead=0, fill=None, name=''):
    """One call into a guarded output that begins `lead` bytes into the payload -> the payload's bytes, checked against the image."""
    C, N = rel.C, rel.N
    span = (C - 1) * mask_stride + N if C else 0
    nbytes = (lead + span + 3 + 16) // 4 * 4
    out = Guard(nbytes)
    if fill is not None:
        out.view(torch.uint8).fill_(fill)
    d_skip, sp = None, 0
    if skip is not None:
        img = np.full((C, skip_stride), 1, dtype=np.uint8)                       # the gap holds "skip": it must not be read
        img[:, :N] = skip
        d_skip = guarded(img, np.uint8)
        sp = d_skip.ptr
    rcode = lib().cffm_seen_mask(rel.d_off.ptr, rel.d_pos.ptr if rel.d_pos is not None else 0, rel.R, rel.nnz, rel.d_row.ptr, sp,
                                 skip_stride or 0, C, N, out.ptr + lead, mask_stride, stream())
    assert rcode == 0, '%s: cffm_seen_mask returned %d' % (name, rcode)
    got = out.read(name, np.uint8)
    want = poison_bytes(nbytes) if fill is None else np.full(nbytes, fill, dtype=np.uint8)
    ref = rel.twin(skip)
    for c in range(C):
        want[lead + c * mask_stride:lead + c * mask_stride + N] = ref[c]
    bad = np.flatnonzero(got != want)
    if bad.size:
        at = int(bad[0]) - lead
        raise AssertionError('%s: %d bytes differ, first at row %d byte %d (N = %d, stride %d): got 0x%02x, want 0x%02x'
                             % (name, bad.size, at // mask_stride if at >= 0 else -1, at % mask_stride if at >= 0 else at, N, mask_stride,
                                got[bad[0]], want[bad[0]]))
    for g, what in ((rel.d_off, 'off'), (rel.d_pos, 'pos'), (rel.d_row, 'row'), (d_skip, 'skip_in')):
        if g is not None:
            g.read('%s: input %s' % (name, what), np.uint8)                       # its canaries
    return got


def standard(C, N, seed):
    """Rows: 0 empty; 1 holds position 0 and position N - 1; 2 all N positions, shuffled; 3 more than 256 entries with repeats, shuffled;
    4.. random.  The contexts cycle through the rows, with -1 (nothing seen) among them."""
    rng = np.random.default_rng(seed)
    rows = [np.zeros(0, dtype=np.int64), np.array([0, N - 1]), rng.permutation(N), rng.integers(0, N, size=700)]
    rows += [rng.integers(0, N, size=int(rng.integers(0, 40))) for _ in range(3)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    row = np.array([[1, 2, 3, -1, 0, 4, 5, 6][c % 8] for c in range(C)])
    return Relation(off, np.concatenate(rows), row, N, rng)


def skip_of(C, N, seed):
    return np.random.default_rng(seed).choice(np.array([0, 0, 0, 1, 255, 2], dtype=np.uint8), size=(C, N))


# (C, N, mask_stride - N, skip: None / 'gap' = rows of N + 3 bytes / 'same' = rows of mask_stride bytes, lead)
CASES = [
    (1, 1, 0, None, 0), (3, 1, 5, 'gap', 0), (70, 1, 0, 'same', 3),
    (1, 15, 0, 'gap', 0), (70, 15, 5, None, 3), (3, 16, 0, None, 0), (3, 16, 0, 'same', 0), (3, 16, 5, 'gap', 0),
    (3, 17, 5, 'same', 0), (70, 17, 0, 'gap', 0),
    (3, 4095, 0, 'same', 0), (1, 4095, 5, None, 3), (3, 4096, 0, None, 0), (3, 4096, 0, 'same', 0), (1, 4096, 5, 'gap', 0),
    (3, 4097, 5, None, 0), (70, 4097, 0, 'gap', 0), (3, 4097, 0, 'same', 3),
    (3, 8200, 0, 'same', 0), (3, 8200, 5, 'gap', 3), (1, 8200, 5, None, 0),
]


@pytest.mark.parametrize('C,N,gap,skip,lead', CASES)
def test_mask_equals_the_twin(C, N, gap, skip, lead):
    rel = standard(C, N, C * 100003 + N)
    name = 'seen_mask C=%d N=%d stride N+%d skip=%s lead=%d' % (C, N, gap, skip, lead)
    sk = None if skip is None else skip_of(C, N, N)
    first = run(rel, N + gap, sk, {None: None, 'gap': N + 3, 'same': N + gap}[skip], lead, name=name)
    assert spec.seen_mask(rel.off, rel.pos, rel.row, N, sk).any()
    again = run(rel, N + gap, sk, {None: None, 'gap': N + 3, 'same': N + gap}[skip], lead, name=name + ' (again)')
    assert np.array_equal(first, again)


@pytest.mark.parametrize('N', [17, 4097])
def test_a_dirty_output_ends_as_a_clean_one(N):
    rel = standard(3, N, N)
    sk = skip_of(3, N, 1)
    for skip, st in ((None, None), (sk, N + 3), (sk, N + 5)):
        clean = run(rel, N + 5, skip, st, fill=0, name='clean output N=%d' % N)
        for fill in (1, 0xff):
            dirty = run(rel, N + 5, skip, st, fill=fill, name='output of 0x%02x N=%d' % (fill, N))
            rows = np.concatenate([np.arange(N) + c * (N + 5) for c in range(3)])
            assert np.array_equal(clean[rows], dirty[rows])


def test_the_empty_relation_with_a_null_pos():
    for N in (1, 33, 4100):
        rel = Relation([0, 0], [], [0, -1, 0], N, null_pos=True)
        run(rel, N, name='nnz=0 N=%d' % N)
        sk = skip_of(3, N, 2)
        got = run(rel, N + 5, sk, N + 3, name='nnz=0 with skip_in N=%d' % N)
        assert got[:N].tolist() == (sk[0] != 0).astype(np.uint8).tolist()        # the mask is skip_in, normalised


MALFORMED = {
    # name: (off, pos, row) at N = 40; the traps behind pos are in range, so an offset that is not clamped shows
    'unsorted-and-repeated': ([0, 7], [39, 3, 3, 0, 39, 17, 3], [0, 0]),
    'entries-outside': ([0, 6], [5, -1, 40, I32_MAX, -(2 ** 31), 39], [0]),
    # the last offset stops short of nnz: a row[c] == R taken for a row would run from off[R] to the trap behind it, over pos[3]
    'rows-outside': ([0, 2, 3], [1, 2, 3, 4], [-1, 2, I32_MAX, -(2 ** 31), 1, 0, 3]),
    'decreasing-offsets': ([0, 3, 1, 4], [10, 11, 12, 13], [0, 1, 2]),
    'offsets-beyond-nnz': ([0, 2, 9, I32_MAX, I32_MAX], [20, 21, 22, 23], [0, 1, 2, 3]),
    'negative-offsets': ([-5, 2, -(2 ** 31), 4, -1], [20, 21, 22, 23], [0, 1, 2, 3]),
    'first-offset-beyond-nnz': ([I32_MAX, I32_MAX], [20, 21], [0]),
}


@pytest.mark.parametrize('case', sorted(MALFORMED))
def test_malformed_relations(case):
    off, pos, row = MALFORMED[case]
    N = 40
    rel = Relation(off, pos, row, N, np.random.default_rng(7))
    want = rel.twin()
    assert case != 'offsets-beyond-nnz' or want[1].sum() == 2                    # [2, 9) is clamped to [2, 4): entries 22 and 23
    run(rel, N + 5, name=case)
    run(rel, N, skip_of(len(row), N, 3), N + 3, lead=3, name=case + ' with skip_in')


def test_skip_in_bytes_are_normalised():
    N = 50
    sk = np.tile(np.array([0, 1, 255, 0, 2, 128], dtype=np.uint8), 25)[:3 * N].reshape(3, N)
    rel = Relation([0, 1], [49], [0, -1, 0], N)
    for st in (N, N + 3):                                                         # the vector path and the byte path
        got = run(rel, N, sk, st, name='normalised skip_in stride %d' % st)
        assert set(np.unique(got[:3 * N])) == {0, 1}


def test_more_contexts_than_a_grid_axis_holds():
    """C = 70000 at N = 1: the units are flattened over grid.x (grid.y would stop at 65535) and walked grid-stride."""
    C = 70000
    rng = np.random.default_rng(9)
    rel = Relation([0, 1, 1, 2, 4], [0, -1, 0, 0], rng.integers(-1, 5, size=C), 1, rng)
    got = run(rel, 1, name='C=70000 N=1')
    assert 0 < got[:C].sum() < C
    run(rel, 3, skip_of(C, 1, 4), 4, name='C=70000 N=1 stride 3 with skip_in')
