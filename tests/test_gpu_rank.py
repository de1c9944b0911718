"""GPU: candidate ranking (cffm_amd/csrc/rank.hip) - cffm_expand_candidates, cffm_topk and cffm_rank_of through the C ABI, bit for
bit against the numpy references of tests/_rank_ref.py (written with lexsort from the order in prose, not from the kernels' key),
then the engine's score_candidates, the class's recommend / evaluate_ranking on the committed frappe slice, and
evaluate_ranking at world size 2.

Every output buffer of the three kernels (and the top-k scratch) is a Guard of tests/test_gpu_rows.py: canaries on both sides, a
NaN poison payload.  The scores sit in rows of N + 5 floats whose 5-float gap holds 3e38 - a value that would win every row if a
kernel read it - and the skip masks in rows of N + 3 bytes.

Shapes: N around every boundary of the top-k plan - one sort of 64 (the smallest), the 8192-candidate chunk, two chunks, three
(16401), and 70001, where k = 1024 survivors of 9 chunks need a third level - with k in {1, 7, 64, 1024} (k > N included) and
C in {1, 3, 130} rows per call.  The rows of one case cycle through 8 score patterns x 4 skip patterns, so that one sort per row
in numpy serves every k, every target and both the skip = NULL and the masked calls."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cffm_amd.spec import CFFMConfig, init_params  # noqa: E402
from oracle import rows_check as rc  # noqa: E402
from tests import _rank_ref as R  # noqa: E402
from tests import test_dist_cpu as H  # noqa: E402   (the spawn / gloo harness)
from tests.test_gpu_rows import Guard, dev_of, stream  # noqa: E402

pytestmark = pytest.mark.gpu

GAP, SKIP_GAP, WINNER = 5, 3, np.float32(3e38)
KS = (1, 7, 64, 1024)
PATTERNS = ('normal', 'five-values', 'all-equal', 'ascending', 'descending', 'max-at-the-end', 'nan-10pct', 'zeros-and-infs')
SKIPS = ('none', '30pct', 'all-but-two', 'all')


@functools.lru_cache(maxsize=None)
def lib():
    from cffm_amd import hip
    hip.load()
    return hip.fast()


# ---- cffm_expand_candidates -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('first,rows', [(0, 15), (4, 7), (14, 1)])
def test_expand(first, rows):
    from cffm_amd import hip
    import ctypes
    F, C, N = 4, 3, 5
    shape = hip.make_shape(CFFMConfig(M=50, F=F, K=8, D=8))
    rng = np.random.default_rng(first + rows)
    ctx = rng.integers(0, 50, size=(C, F)).astype(np.int32)
    cand = np.array([49, -1, 0, 50, 7], dtype=np.int32)                      # ids are not validated here: they travel as they are
    dctx, dcand = dev_of(ctx), dev_of(cand)
    for field in range(F):
        name = 'expand first=%d rows=%d field=%d' % (first, rows, field)
        out = Guard(C * N * F * 4)
        rcode = lib().cffm_expand_candidates(ctypes.addressof(shape), dctx.data_ptr(), C, field, dcand.data_ptr(), N, first, rows, out.ptr,
                                             stream())
        assert rcode == 0, '%s returned %d' % (name, rcode)
        got = out.read(name, np.int32)
        rc.check_exact(name, got[:rows * F], R.expand_ref(ctx, field, cand, first, rows).reshape(-1))
        rc.check_untouched(name + ': beyond rows * F values', got[rows * F:].view(np.float32))


# ---- cffm_topk / cffm_rank_of ---------------------------------------------------------------------------------------------
def score_row(rng, pattern, N):
    if pattern == 'normal':
        return rng.standard_normal(N)
    if pattern == 'five-values':
        return rng.choice([-1.0, -0.5, 0.0, 0.5, 1.0], size=N)
    if pattern == 'all-equal':
        return np.full(N, 0.75)
    if pattern == 'ascending':
        return np.arange(N) * 0.5 - 3.0
    if pattern == 'descending':
        return 3.0 - np.arange(N) * 0.5
    if pattern == 'max-at-the-end':                  # the unique maximum at the last position of the last chunk
        s = rng.random(N)
        s[N - 1] = 10.0
        return s
    s = rng.standard_normal(N)
    if pattern == 'nan-10pct':
        s[rng.random(N) < 0.1] = np.nan
        return s
    assert pattern == 'zeros-and-infs'
    special = np.array([0.0, -0.0, np.inf, -np.inf])
    where = rng.random(N) < 0.4
    s[where] = special[rng.integers(0, 4, size=int(where.sum()))]
    return s


def skip_row(rng, mode, N):
    if mode == 'none':
        return np.zeros(N, dtype=np.uint8)
    if mode == '30pct':
        return (rng.random(N) < 0.3).astype(np.uint8)
    sk = np.ones(N, dtype=np.uint8)
    if mode == 'all-but-two':
        sk[rng.choice(N, size=min(2, N), replace=False)] = 0
    return sk


class Case(object):
    """rows x N scores (rows cycle through PATTERNS x SKIPS), on the device inside gapped rows, and one numpy sort per row."""

    def __init__(self, N, rows):
        rng = np.random.default_rng(N)
        self.N, self.rows = N, rows
        combos = [(p, m) for m in SKIPS for p in PATTERNS]
        self.labels = [combos[r % len(combos)] for r in range(rows)]
        self.scores = np.stack([score_row(rng, p, N) for p, _ in self.labels]).astype(np.float32)
        self.skip = np.stack([skip_row(rng, m, N) for _, m in self.labels])
        self.orders = R.orders_of(self.scores)
        img = np.full((rows, N + GAP), WINNER, dtype=np.float32)
        img[:, :N] = self.scores
        simg = np.ones((rows, N + SKIP_GAP), dtype=np.uint8)
        simg[:, :N] = self.skip
        self.d_scores, self.d_skip = dev_of(img), dev_of(simg)
        self.topk = {}                               # masked? -> topk_ref at k = 1024: every smaller k is its prefix
        for masked in (False, True):
            self.topk[masked] = R.topk_ref(self.scores, 1024, self.skip if masked else None, self.orders)
        # rank-of targets: position 0, position N - 1, a skipped position (the row's first; N / 2 where nothing is skipped), -1, N
        skipped = np.array([int(np.nonzero(sk)[0][0]) if sk.any() else N // 2 for sk in self.skip], dtype=np.int32)
        self.targets = [np.zeros(rows, dtype=np.int32), np.full(rows, N - 1, dtype=np.int32), skipped,
                        np.full(rows, -1, dtype=np.int32), np.full(rows, N, dtype=np.int32)]
        self.ranks = {(masked, t): R.rank_ref(self.scores, tg, self.skip if masked else None, self.orders)
                      for masked in (False, True) for t, tg in enumerate(self.targets)}
        self.d_targets = [dev_of(t) for t in self.targets]

    def ptrs(self, r0, masked):
        return (self.d_scores.data_ptr() + r0 * (self.N + GAP) * 4, self.N + GAP,
                self.d_skip.data_ptr() + r0 * (self.N + SKIP_GAP) if masked else 0, self.N + SKIP_GAP if masked else 0)


@functools.lru_cache(maxsize=2)
def case(N, rows):
    return Case(N, rows)


def run_topk(c, r0, C, k, masked, name):
    nb = int(lib().cffm_topk_scratch_bytes(C, c.N, k))
    assert nb > 0
    scratch, idx, val, count = Guard(nb), Guard(C * k * 4), Guard(C * k * 4), Guard(C * 4)
    sp, ss, kp, ks = c.ptrs(r0, masked)
    rcode = lib().cffm_topk(sp, ss, kp, ks, C, c.N, k, scratch.ptr, idx.ptr, val.ptr, count.ptr, stream())
    assert rcode == 0, '%s: cffm_topk returned %d' % (name, rcode)
    scratch.read(name + ' scratch', np.uint8)                                  # its canaries
    ridx, rval, rcount = c.topk[masked]
    rows = slice(r0, r0 + C)
    rc.check_exact(name + ' count', count.read(name + ' count', np.int32), np.minimum(rcount[rows], k))
    rc.check_exact(name + ' idx', idx.read(name + ' idx', np.int32), ridx[rows, :k].reshape(-1))
    rc.check_exact(name + ' val', val.read(name + ' val', np.uint32), rval[rows, :k].reshape(-1))


def run_rank(c, r0, C, t, masked, name):
    out = Guard(C * 4)
    sp, ss, kp, ks = c.ptrs(r0, masked)
    rcode = lib().cffm_rank_of(sp, ss, kp, ks, C, c.N, c.d_targets[t].data_ptr() + r0 * 4, out.ptr, stream())
    assert rcode == 0, '%s: cffm_rank_of returned %d' % (name, rcode)
    rc.check_exact(name, out.read(name, np.int32), c.ranks[(masked, t)][r0:r0 + C])


# C = 3 at every N; one row per call and 130 rows per call where the plan changes: one sort, two levels, three levels
SHAPES = [(N, 3) for N in (1, 63, 64, 65, 8191, 8192, 8193, 16401, 70001)] + [(1, 1), (8193, 1), (70001, 1)] + \
    [(1, 130), (65, 130), (8193, 130)]


@pytest.mark.parametrize('N,C', SHAPES)
def test_topk_and_rank_of(N, C):
    rows = 130 if C == 130 else 32                   # every (pattern, skip) pair once; 130 rows: four times
    c = case(N, rows)
    assert set(c.labels) == {(p, m) for p in PATTERNS for m in SKIPS}
    if N >= 64:
        assert any(np.unique(r).size < r.size for r in c.scores) and np.isnan(c.scores).any() and (c.scores == -np.inf).any()
    groups = [(r0, min(C, rows - r0)) for r0 in range(0, rows, C)]
    if C == 1:
        groups = groups[::3] + [groups[-1]]          # one row per call: a third of the rows, every pattern and skip still among them
    for r0, n in groups:
        for masked in (False, True):
            for k in KS:
                run_topk(c, r0, n, k, masked, 'topk N=%d rows %d..%d k=%d %s' % (N, r0, r0 + n, k, 'masked' if masked else 'skip=NULL'))
            for t in range(5):
                run_rank(c, r0, n, t, masked, 'rank_of N=%d rows %d..%d target %d %s' % (N, r0, r0 + n, t, 'masked' if masked else 'skip=NULL'))


def test_topk_prefix_and_rank_agree_on_the_device():
    """The two kernels share one order: the candidate cffm_topk puts at place j has rank j by cffm_rank_of (N = 8193: two levels)."""
    c = case(8193, 32)
    k = 64
    idx, count = Guard(32 * k * 4), Guard(32 * 4)
    val, scratch = Guard(32 * k * 4), Guard(int(lib().cffm_topk_scratch_bytes(32, c.N, k)))
    sp, ss, kp, ks = c.ptrs(0, True)
    assert lib().cffm_topk(sp, ss, kp, ks, 32, c.N, k, scratch.ptr, idx.ptr, val.ptr, count.ptr, stream()) == 0
    got = idx.read('idx', np.int32).reshape(32, k)
    cnt = count.read('count', np.int32)
    for j in (0, 5, 63):
        out = Guard(32 * 4)
        assert lib().cffm_rank_of(sp, ss, kp, ks, 32, c.N, dev_of(got[:, j].copy()).data_ptr(), out.ptr, stream()) == 0
        rc.check_exact('rank of the candidate at place %d' % j, out.read('rank', np.int32), np.where(cnt > j, j, -1).astype(np.int32))


# ---- HipEngine.score_candidates / topk / rank_of ---------------------------------------------------------------------------
def ref_scores(eng, ctx, field, cand, block):
    """engine.predict over the numpy-expanded ids, cut into the pieces score_candidates cuts the flattened range into."""
    C, N = ctx.shape[0], cand.size
    out = np.empty(C * N, dtype=np.float32)
    for s0 in range(0, C * N, block):
        m = min(block, C * N - s0)
        out[s0:s0 + m] = eng.predict(dev_of(R.expand_ref(ctx, field, cand, s0, m))).cpu().numpy()
    return out.reshape(C, N)


@pytest.mark.parametrize('name,cfg,C,N,block', [
    ('small', CFFMConfig(M=50, F=4, K=8, D=8), 3, 7, 8),                       # pieces of 8 rows cut the contexts of 7
    ('frappe', CFFMConfig(M=5382, F=10, K=32, D=32, activation='selu'), 2, 300, 256),
])
def test_score_candidates_equals_predict_on_the_expanded_ids(name, cfg, C, N, block):
    from cffm_amd.engine import HipEngine
    rng = np.random.default_rng(C + N)
    p = init_params(cfg, seed=3)
    p['feature_bias'] = (rng.standard_normal(p['feature_bias'].shape) * 0.3).astype(np.float32)
    eng = HipEngine(cfg, params=p)
    ctx = rng.integers(0, cfg.M, size=(C, cfg.F)).astype(np.int32)
    cand = rng.permutation(cfg.M)[:N].astype(np.int32)
    cand[1], cand[N - 1] = -1, cfg.M                                           # clamped by the forward, as predict clamps them
    for field in (0, cfg.F - 1):
        got = eng.score_candidates(dev_of(ctx), field, dev_of(cand), block=block)
        assert got.shape == (C, N) and got.dtype == torch.float32
        want = ref_scores(eng, ctx, field, cand, block)
        assert np.unique(want).size > N // 2, 'the scores do not depend on the candidate'
        rc.check_exact('%s field %d' % (name, field), got.cpu().numpy().reshape(-1), want.reshape(-1))
        # the engine's top-k and rank-of on that buffer, through the cached scratch
        for k in (1, 5):
            idx, val, count = eng.topk(got, k)
            ridx, rval, rcount = R.topk_ref(want, k)
            rc.check_exact('%s topk idx' % name, idx.cpu().numpy(), ridx)
            rc.check_exact('%s topk val' % name, val.cpu().numpy().view(np.uint32), rval)
            rc.check_exact('%s topk count' % name, count.cpu().numpy(), rcount)
        target = rng.integers(0, N, size=C).astype(np.int32)
        mask = rng.random((C, N)) < 0.3
        rc.check_exact('%s rank_of' % name, eng.rank_of(got, dev_of(target), skip=dev_of(mask)).cpu().numpy(), R.rank_ref(want, target, mask))


# ---- CFFM.recommend / CFFM.evaluate_ranking ----------------------------------------------------------------------------------
FIELD = 1


def _frappe_model(tmp_path):
    import contextlib
    import io
    from cffm_amd import CFFM as M
    from cffm_amd.LoadData import LoadData
    with contextlib.redirect_stdout(io.StringIO()):
        data = LoadData(os.path.join(ROOT, 'tests', 'golden', 'frappe_slice') + '/', 'frappe', 'square_loss')
    m = M.CFFM(data.features_M, 0, str(tmp_path / 'm'), 32, 32, 'square_loss', 1, 16, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer', 0, 0, 0,
               10, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'selu', batch_rng=np.random.RandomState(3))
    m.train(data)
    return M, m, data


def test_class_recommend_and_evaluate_ranking(tmp_path):
    M, m, data = _frappe_model(tmp_path)
    column = lambda split: np.array([r[FIELD] for r in split['X']], dtype=np.int32)
    # recommend: the default candidates are the train column's distinct ids, sorted
    cand = np.unique(column(data.Train_data))
    ctx = np.asarray(data.Test_data['X'][:6], dtype=np.int32)
    want = ref_scores(m.engine, ctx, FIELD, cand, 8192)
    skip = np.random.default_rng(1).random(want.shape) < 0.2
    for sk in (None, skip):
        ids, val = m.recommend(ctx, FIELD, k=5, skip=sk)
        ridx, rval, _ = R.topk_ref(want, 5, sk)
        rc.check_exact('recommend ids', ids, cand[ridx])
        rc.check_exact('recommend scores', val.view(np.uint32), rval)
    ids, val = m.recommend(ctx[:2], FIELD, candidates=cand[:3], k=5)           # k beyond the candidates: -1 / NaN padding
    assert (ids[:, 3:] == -1).all() and np.isnan(val[:, 3:]).all() and (ids[:, :3] >= 0).all()
    # evaluate_ranking: every positive row of the test split, its own id at FIELD among train + test ids
    test = data.Test_data
    pos = np.asarray(test['Y']) > 0
    rows = np.asarray(test['X'], dtype=np.int32)[pos]
    cand = np.union1d(column(data.Train_data), column(test)).astype(np.int32)
    scores = ref_scores(m.engine, rows, FIELD, cand, 8192)
    ranks = R.rank_ref(scores, np.searchsorted(cand, rows[:, FIELD]))
    want = M.ranking_metrics(ranks, 10)
    got = m.evaluate_ranking(test, FIELD, k=10)
    print('frappe slice: %d positive rows, %d candidates, HR@10 %.6f NDCG@10 %.6f' % (rows.shape[0], cand.size, got[0], got[1]))
    assert abs(got[0] - want[0]) <= 1e-12 and abs(got[1] - want[1]) <= 1e-12, (got, want)
    again = m.evaluate_ranking(test, FIELD, k=10)
    assert np.array_equal(np.array(got).view(np.uint64), np.array(again).view(np.uint64))
    want50 = M.ranking_metrics(ranks, 50)                                      # a k that separates hits from misses
    got50 = m.evaluate_ranking(test, FIELD, k=50)
    assert 0.0 < want50[0] < 1.0, ranks
    assert abs(got50[0] - want50[0]) <= 1e-12 and abs(got50[1] - want50[1]) <= 1e-12, (got50, want50)


def _ranking_worker(rank, world, tmp):
    """evaluate_ranking of the SAME untrained model (one seed; under a group rank 0's parameters are broadcast) at any world size."""
    from cffm_amd import CFFM as M
    from cffm_amd import synth

    class Split(dict):
        pass
    rng = np.random.default_rng(11)
    Mf, F = 200, 4                                                           # 50 ids per field (cffm_amd.synth.field_ranges)
    test = Split(X=synth.sample_ids(rng, Mf, F, 91).tolist(), Y=synth.sample_labels(rng, 91).tolist())
    m = M.CFFM(Mf, 0, os.path.join(tmp, 'k%d_w%d' % (rank, world)), 8, 8, 'square_loss', 1, 8, 0.05, 0, [1.0, 1.0],
               'AdagradOptimizer', 0, 0, 0, F, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'relu')
    m.build_graph()
    assert m.world == world
    return m.evaluate_ranking(test, 2, k=10, candidates=np.arange(100, 150)), sum(1 for v in test['Y'] if v > 0)


def test_evaluate_ranking_world2_equals_world1(tmp_path):
    one, n_pos = H._run(_ranking_worker, 1, str(tmp_path))[0]
    two = H._run(_ranking_worker, 2, str(tmp_path))
    assert n_pos >= 16
    assert 0.0 < one[0] < 1.0, one                                             # the case separates hits from misses
    for rank in (0, 1):
        got = two[rank][0]
        assert abs(got[0] - one[0]) <= 1e-12 and abs(got[1] - one[1]) <= 1e-12, (rank, got, one)
