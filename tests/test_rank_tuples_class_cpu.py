"""CFFM.recommend_tuples / CFFM.evaluate_ranking_tuples on a stub engine (no GPU): the four candidate shapes and what is refused,
counts merged into the skip mask, positions (not ids) returned, the sampled protocol's lists (target once, distinct negatives, a
drawn target position, the same seed the same lists), which scoring method runs under each sweep= value, and the sharded refusal.
The engine's score / top-k / rank-of are the numpy references of tests/_rank_ref.py over the id rows of tests/_cand_ref.py and a
score that is a plain function of the ids, as in tests/test_rank_class_cpu.py."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from cffm_amd import CFFM as M
from cffm_amd.LoadData import LoadData
from tests import _cand_ref as CR
from tests import _rank_ref as R
from tests.test_rank_class_cpu import _score

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'golden', 'frappe_slice') + '/'
FIELDS = (1, 6)


class _StubEngine(object):
    device = torch.device('cpu')
    opt_step = 0
    served = True

    def __init__(self, cfg, seed):
        self.cfg, self.calls = cfg, []

    def sweep_ok(self):
        return self.served

    def score_candidate_tuples(self, ctx, fields, cand, block=8192):
        ctx, cand = ctx.numpy(), cand.numpy()
        self.calls.append(('tuples', list(fields), ctx.copy(), cand.copy()))
        return torch.from_numpy(_score(CR.expand_tuples(ctx, list(fields), cand)).reshape(ctx.shape[0], cand.shape[-2]))

    def score_candidates(self, ctx, field, cand, block=8192):               # what evaluate_ranking calls: the same score
        return torch.from_numpy(_score(R.expand_ref(ctx.numpy(), field, cand.numpy(), 0, ctx.shape[0] * cand.numel())).reshape(ctx.shape[0], -1))

    def score_candidates_shared(self, ctx, field, cand):
        assert cand.dim() == 1
        self.calls.append(('shared', [field], ctx.numpy().copy(), cand.numpy().copy()))
        return torch.from_numpy(_score(CR.expand_tuples(ctx.numpy(), [field], cand.numpy()[:, None])).reshape(ctx.shape[0], -1))

    def score_candidate_lists_shared(self, ctx, field, cand):
        assert cand.dim() == 2 and cand.shape[0] == ctx.shape[0]
        self.calls.append(('lists_shared', [field], ctx.numpy().copy(), cand.numpy().copy()))
        return torch.from_numpy(_score(CR.expand_tuples(ctx.numpy(), [field], cand.numpy()[:, :, None])).reshape(ctx.shape[0], -1))

    def topk(self, scores, k, skip=None):
        idx, val, count = R.topk_ref(scores.numpy(), k, None if skip is None else skip.numpy())
        return torch.from_numpy(idx), torch.from_numpy(val.view(np.float32)), torch.from_numpy(count)

    def rank_of(self, scores, target, skip=None):
        return torch.from_numpy(R.rank_ref(scores.numpy(), target.numpy(), None if skip is None else skip.numpy()))


@pytest.fixture(scope='module')
def data():
    with contextlib.redirect_stdout(io.StringIO()):
        return LoadData(PATH, 'frappe', 'square_loss')


@pytest.fixture
def model(tmp_path, data, monkeypatch):
    monkeypatch.setattr(M.CFFM, 'engine_factory', _StubEngine)
    monkeypatch.setattr(_StubEngine, 'served', True)
    monkeypatch.delenv('CFFM_TABLES', raising=False)
    m = M.CFFM(data.features_M, 0, str(tmp_path / 'm'), 8, 8, 'square_loss', 1, 16, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer', 0, 0, 0,
               10, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'relu')
    m.build_graph()
    m._train_split = data.Train_data
    return m


def _kinds(m):
    kinds = [c[0] for c in m.engine.calls]
    del m.engine.calls[:]
    return kinds


def _rows(split, fields=FIELDS):
    return np.asarray(split['X'], dtype=np.int32)[:, list(fields)]


def _want(ctx, fields, cand, k, skip=None):
    scores = _score(CR.expand_tuples(ctx, list(fields), cand)).reshape(ctx.shape[0], -1)
    idx, bits_, count = R.topk_ref(scores, k, skip)
    return idx, bits_, count


CTX = slice(0, 5)


def test_the_four_candidate_shapes(model, data):
    ctx = np.asarray(data.Test_data['X'][CTX], dtype=np.int32)
    rng = np.random.default_rng(4)
    C, N, k = ctx.shape[0], 9, 4
    one = rng.integers(0, 200, size=N).astype(np.int32)
    two = rng.integers(0, 200, size=(N, 2)).astype(np.int32)
    one_pc = rng.integers(0, 200, size=(C, N)).astype(np.int32)
    two_pc = rng.integers(0, 200, size=(C, N, 2)).astype(np.int32)
    for fields, cand, pc, full in ((1, one, False, one[:, None]), ([1], one[:, None], False, one[:, None]), (FIELDS, two, False, two),
                                   (1, one_pc, True, one_pc[:, :, None]), (FIELDS, two_pc, True, two_pc)):
        pos, val = model.recommend_tuples(ctx, fields, cand, per_context=pc, k=k, score_rows=2 * N)     # groups of 2 + 2 + 1 contexts
        assert _kinds(model) == ['tuples'] * 3
        cols = [fields] if isinstance(fields, int) else list(fields)
        idx, bits_, count = _want(ctx, cols, full, k)
        assert pos.dtype == np.int32 and val.dtype == np.float32 and pos.shape == (C, k)
        assert np.array_equal(pos, idx) and np.array_equal(val.view(np.uint32), bits_)                  # POSITIONS in the caller's list
    # the per-context group really gets the lists of its own contexts
    model.recommend_tuples(ctx, FIELDS, two_pc, per_context=True, k=k, score_rows=2 * N)
    got = [c[3] for c in model.engine.calls]
    assert [g.shape[0] for g in got] == [2, 2, 1] and np.array_equal(np.concatenate(got), two_pc)
    assert np.array_equal(np.concatenate([c[2] for c in model.engine.calls]), ctx)
    del model.engine.calls[:]
    # what is refused
    for fields, cand, pc in ((FIELDS, one, False),                   # tuples need a last axis of nf
                             (FIELDS, two[:, :1], False), (1, two, False), (1, two_pc, False), (FIELDS, two_pc, False),
                             (FIELDS, two, True), (1, one, True), (FIELDS, two_pc[:3], True), (1, one_pc[:, :0], True),
                             (1, one.astype(np.float32), False)):
        with pytest.raises(ValueError, match='candidates'):
            model.recommend_tuples(ctx, fields, cand, per_context=pc)
    for fields in ((1, 1), (), (10,), -1, (1, 10), 10):
        with pytest.raises(ValueError, match='fields'):
            model.recommend_tuples(ctx, fields, two)
    for bad_k in (0, 1025):
        with pytest.raises(ValueError, match='k must'):
            model.recommend_tuples(ctx, FIELDS, two, k=bad_k)
    with pytest.raises(ValueError, match='contexts'):
        model.recommend_tuples(ctx[:, :-1], FIELDS, two)
    with pytest.raises(ValueError, match='skip'):
        model.recommend_tuples(ctx, FIELDS, two, skip=np.zeros((C, N + 1), dtype=bool))
    assert _kinds(model) == []                                                # refused before anything is scored


def test_counts_are_merged_into_the_skip_mask(model, data):
    ctx = np.asarray(data.Test_data['X'][CTX], dtype=np.int32)
    rng = np.random.default_rng(5)
    C, N, k = ctx.shape[0], 8, 6
    lists = rng.integers(0, 200, size=(C, N, 2)).astype(np.int32)
    counts = np.array([8, 0, 3, 7, 1])
    skip = rng.random((C, N)) < 0.3
    pad = np.arange(N)[None, :] >= counts[:, None]
    for sk, mask in ((None, pad), (skip, skip | pad)):
        pos, val = model.recommend_tuples(ctx, FIELDS, lists, per_context=True, counts=counts, k=k, skip=sk)
        idx, bits_, count = _want(ctx, FIELDS, lists, k, mask)
        assert np.array_equal(pos, idx) and np.array_equal(val.view(np.uint32), bits_)
        assert (count <= np.minimum(counts, k)).all() and (pos[1] == -1).all() and np.isnan(val[1]).all()
        for c in range(C):
            assert (pos[c][pos[c] >= 0] < counts[c]).all()                      # never a padded position
    # any id may sit in the padding
    junk = lists.copy()
    junk[pad] = -77
    again, _ = model.recommend_tuples(ctx, FIELDS, junk, per_context=True, counts=counts, k=k)
    assert np.array_equal(again, _want(ctx, FIELDS, lists, k, pad)[0])
    for bad in (counts[:3], counts + 8, -counts - 1, counts.astype(np.float64)):
        with pytest.raises(ValueError, match='counts'):
            model.recommend_tuples(ctx, FIELDS, lists, per_context=True, counts=bad)
    with pytest.raises(ValueError, match='counts'):
        model.recommend_tuples(ctx, FIELDS, lists[0], counts=counts)          # a shared list has no counts


def test_which_scoring_method_runs(model, data, monkeypatch):
    ctx = np.asarray(data.Test_data['X'][CTX], dtype=np.int32)
    rng = np.random.default_rng(6)
    one, two = np.arange(30, dtype=np.int32), rng.integers(0, 200, size=(30, 2)).astype(np.int32)
    one_pc = rng.integers(0, 200, size=(5, 30)).astype(np.int32)
    base = model.recommend_tuples(ctx, 1, one)
    base_pc = model.recommend_tuples(ctx, 1, one_pc, per_context=True)
    assert _kinds(model) == ['tuples', 'tuples']
    # 'shared': one field only
    assert np.array_equal(model.recommend_tuples(ctx, 1, one, sweep='shared')[0], base[0]) and _kinds(model) == ['shared']
    assert np.array_equal(model.recommend_tuples(ctx, 1, one_pc, per_context=True, sweep='shared')[0], base_pc[0])
    assert _kinds(model) == ['lists_shared']
    with pytest.raises(ValueError, match='shared'):
        model.recommend_tuples(ctx, FIELDS, two, sweep='shared')
    with pytest.raises(ValueError, match='shared'):
        model.evaluate_ranking_tuples(data.Test_data, FIELDS, sweep='shared')
    # 'auto': the shared sweep for one field, a served shape and N >= SWEEP_MIN_N only
    monkeypatch.setattr(M, 'SWEEP_MIN_N', 30)
    model.recommend_tuples(ctx, 1, one, sweep='auto')
    model.recommend_tuples(ctx, 1, one_pc, per_context=True, sweep='auto')
    model.recommend_tuples(ctx, FIELDS, two, sweep='auto')                    # nf = 2 takes expand
    assert _kinds(model) == ['shared', 'lists_shared', 'tuples']
    monkeypatch.setattr(M, 'SWEEP_MIN_N', 31)
    model.recommend_tuples(ctx, 1, one, sweep='auto')
    monkeypatch.setattr(M, 'SWEEP_MIN_N', None)
    model.recommend_tuples(ctx, 1, one, sweep='auto')
    assert _kinds(model) == ['tuples', 'tuples']
    monkeypatch.setattr(M, 'SWEEP_MIN_N', 1)
    monkeypatch.setattr(_StubEngine, 'served', False)
    model.recommend_tuples(ctx, 1, one, sweep='auto')
    assert _kinds(model) == ['tuples']
    with pytest.raises(ValueError, match='shared'):
        model.recommend_tuples(ctx, 1, one, sweep='shared')
    for bad in ('fast', None, 'EXPAND'):
        with pytest.raises(ValueError, match='sweep'):
            model.recommend_tuples(ctx, 1, one, sweep=bad)
        with pytest.raises(ValueError, match='sweep'):
            model.evaluate_ranking_tuples(data.Test_data, 1, sweep=bad)
    assert _kinds(model) == []


def _positives(split):
    pos = np.asarray(split['Y']).reshape(-1) > 0
    return np.asarray(split['X'], dtype=np.int32)[pos]


def test_evaluate_with_one_shared_list(model, data):
    test = data.Test_data
    ctx = _positives(test)
    distinct = np.unique(np.concatenate([_rows(data.Train_data), _rows(test)]), axis=0)          # sorted rows, as torch.unique(dim=0)
    scores = _score(CR.expand_tuples(ctx, list(FIELDS), distinct)).reshape(ctx.shape[0], -1)
    target = np.array([int(np.nonzero((distinct == t).all(axis=1))[0][0]) for t in ctx[:, list(FIELDS)]])
    ranks = R.rank_ref(scores, target)
    assert 0 < (ranks < 10).sum() < ranks.size                                                     # the case separates hits from misses
    got = model.evaluate_ranking_tuples(test, FIELDS, k=10, score_rows=3 * distinct.shape[0])
    assert got == pytest.approx(M.ranking_metrics(ranks, 10), abs=1e-12)
    calls = model.engine.calls
    assert all(np.array_equal(c[3], distinct) for c in calls) and max(c[2].shape[0] for c in calls) == 3
    assert np.array_equal(np.concatenate([c[2] for c in calls]), ctx)
    del calls[:]
    # explicit candidates in the caller's order, with a repeated tuple: the first position counts
    perm = np.random.default_rng(3).permutation(distinct.shape[0])
    cand = np.concatenate([distinct[perm], distinct[perm][:4]])
    scores = _score(CR.expand_tuples(ctx, list(FIELDS), cand)).reshape(ctx.shape[0], -1)
    target = np.array([int(np.nonzero((cand == t).all(axis=1))[0][0]) for t in ctx[:, list(FIELDS)]])
    got = model.evaluate_ranking_tuples(test, FIELDS, k=10, candidates=cand)
    assert got == pytest.approx(M.ranking_metrics(R.rank_ref(scores, target), 10), abs=1e-12)
    # one field: the distinct ids of the column, as evaluate_ranking ranks them
    assert model.evaluate_ranking_tuples(test, 1, k=10) == pytest.approx(model.evaluate_ranking(test, 1, k=10), abs=1e-12)
    # explicit candidates that lack a target
    first = ctx[0, list(FIELDS)]
    lacking = distinct[~(distinct == first).all(axis=1)]
    with pytest.raises(ValueError, match=r'target \(%d, %d\) at fields \(1, 6\)' % tuple(first)):
        model.evaluate_ranking_tuples(test, FIELDS, candidates=lacking)
    with pytest.raises(ValueError, match='k must'):
        model.evaluate_ranking_tuples(test, FIELDS, k=0)


def _lists_of(model, data, m, seed, **kw):
    """evaluate_ranking_tuples(negatives=m): the result and the (contexts, lists) the engine was handed, whole."""
    del model.engine.calls[:]
    got = model.evaluate_ranking_tuples(data.Test_data, FIELDS, k=3, negatives=m, seed=seed, **kw)
    calls = model.engine.calls[:]
    del model.engine.calls[:]
    assert all(c[0] == 'tuples' and c[3].ndim == 3 for c in calls)
    return got, np.concatenate([c[2] for c in calls]), np.concatenate([c[3] for c in calls])


def test_sampled_negatives(model, data):
    test = data.Test_data
    ctx = _positives(test)
    distinct = np.unique(np.concatenate([_rows(data.Train_data), _rows(test)]), axis=0)
    U, m = distinct.shape[0], 7
    assert U > m + 2
    got, seen_ctx, lists = _lists_of(model, data, m, seed=11, score_rows=4 * (m + 1))
    assert np.array_equal(seen_ctx, ctx) and lists.shape == (ctx.shape[0], m + 1, 2)
    tgt = ctx[:, list(FIELDS)]
    is_target = (lists == tgt[:, None, :]).all(axis=2)
    assert (is_target.sum(axis=1) == 1).all()                                  # the target is in every list exactly once
    place = is_target.argmax(axis=1)
    assert np.unique(place).size > 1                                           # and not always at the same position
    known = {tuple(t) for t in distinct.tolist()}
    for row in lists:
        rows = [tuple(t) for t in row.tolist()]
        assert len(set(rows)) == m + 1 and set(rows) <= known                  # distinct tuples of the distinct set
    assert np.unique(lists.reshape(ctx.shape[0], -1), axis=0).shape[0] > 1     # the rows do not share one list
    # the metrics are those of the lists the engine saw, with the target at its drawn position
    scores = _score(CR.expand_tuples(ctx, list(FIELDS), lists)).reshape(ctx.shape[0], m + 1)
    assert got == pytest.approx(M.ranking_metrics(R.rank_ref(scores, place), 3), abs=1e-12)
    # the same seed gives the same lists, whatever the grouping; another seed gives others
    got2, _, lists2 = _lists_of(model, data, m, seed=11)
    assert np.array_equal(lists2, lists) and got2 == got
    _, _, lists3 = _lists_of(model, data, m, seed=12)
    assert not np.array_equal(lists3, lists)
    # m = U - 1: every list is the whole distinct set; m = U is too many
    _, _, whole = _lists_of(model, data, U - 1, seed=0)
    assert all({tuple(t) for t in row.tolist()} == known for row in whole)
    for bad in (U, U + 5, 0, -1):
        with pytest.raises(ValueError, match='negatives'):
            model.evaluate_ranking_tuples(test, FIELDS, negatives=bad)
    # explicit candidates: the draw is from their distinct tuples
    sub = np.concatenate([distinct, distinct[:5]])
    _, _, lists4 = _lists_of(model, data, m, seed=11, candidates=sub)
    assert np.array_equal(lists4, lists)
    with pytest.raises(ValueError, match='negatives'):
        model.evaluate_ranking_tuples(test, FIELDS, negatives=U, candidates=sub)


def test_ranks_take_disjoint_shares_of_the_same_lists(model, data, monkeypatch):
    """Under a process group every rank draws all lists and scores its contiguous share: the shares of a world of 3 are disjoint,
    cover every row and hold the lists world size 1 holds."""
    m = 5
    _, ctx1, lists1 = _lists_of(model, data, m, seed=2)
    parts = []
    monkeypatch.setattr(model, '_all_reduce_sum', lambda t: t)                  # no group here: every rank's own sums
    for rank in range(3):
        model.world, model.rank = 3, rank
        _, c, l = _lists_of(model, data, m, seed=2)
        parts.append((c, l))
    model.world, model.rank = 1, 0
    assert all(p[0].shape[0] > 0 for p in parts)
    assert np.array_equal(np.concatenate([p[0] for p in parts]), ctx1) and np.array_equal(np.concatenate([p[1] for p in parts]), lists1)


def test_both_refuse_row_sharded_tables(model, data):
    model._sh = object()
    msg = 'CFFM_TABLES=sharded: recommend / evaluate_ranking run on replicated tables'
    with pytest.raises(ValueError) as e:
        model.recommend_tuples(np.asarray(data.Test_data['X'][:2]), FIELDS, [[1, 2]])
    assert str(e.value) == msg
    with pytest.raises(ValueError) as e:
        model.evaluate_ranking_tuples(data.Test_data, FIELDS, negatives=3)
    assert str(e.value) == msg


def test_evaluate_raises_on_nan(model, data, monkeypatch):
    def nan_scores(self, ctx, fields, cand, block=8192):
        out = torch.zeros((ctx.shape[0], cand.shape[-2]))
        out[0, 0] = float('nan')
        return out
    monkeypatch.setattr(_StubEngine, 'score_candidate_tuples', nan_scores)
    with pytest.raises(ValueError, match='NaN'):
        model.evaluate_ranking_tuples(data.Test_data, FIELDS)
