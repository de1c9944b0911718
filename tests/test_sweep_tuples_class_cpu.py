"""CFFM.recommend_tuples / CFFM.evaluate_ranking_tuples with sweep='tuples' on a stub engine (no GPU), as
tests/test_rank_tuples_class_cpu.py does for the other values: which engine method runs for a shared list and for per-context lists,
that positions and scores are the numpy order of the scores that method returned, and what is refused where the stub says the
(shape, nf) is not served."""
import numpy as np
import pytest
import torch

from cffm_amd import CFFM as M
from tests import _cand_ref as CR
from tests import _rank_ref as R
from tests.test_rank_class_cpu import _score
from tests.test_rank_tuples_class_cpu import FIELDS, _StubEngine, _kinds, _positives, _rows, data, model  # noqa: F401  (fixtures)


class _TupleStub(_StubEngine):
    served_nf = (1, 2)

    def sweep_tuples_ok(self, nf):
        return nf in self.served_nf

    def score_candidate_tuples_shared(self, ctx, fields, cand):
        assert cand.dim() in (2, 3) and cand.shape[-1] == len(fields)
        ctx, cand = ctx.numpy(), cand.numpy()
        self.calls.append(('tuples_shared', list(fields), ctx.copy(), cand.copy()))
        # another score than the expand stub's, so that the order can only come from this method's return value
        s = _score(CR.expand_tuples(ctx, list(fields), cand)).reshape(ctx.shape[0], cand.shape[-2])
        return torch.from_numpy((-s).astype(np.float32))


@pytest.fixture
def tmodel(model, monkeypatch):
    monkeypatch.setattr(_TupleStub, 'served_nf', (1, 2))
    stub = _TupleStub(model.engine.cfg, 0)
    monkeypatch.setattr(model, 'engine', stub)
    return model


def _neg_scores(ctx, fields, cand):
    return (-_score(CR.expand_tuples(ctx, list(fields), cand)).reshape(ctx.shape[0], -1)).astype(np.float32)


def test_recommend_takes_the_tuple_sweep(tmodel, data):  # noqa: F811
    ctx = np.asarray(data.Test_data['X'][:5], dtype=np.int32)
    rng = np.random.default_rng(8)
    C, N, k = 5, 9, 4
    one, two = rng.integers(0, 200, size=N).astype(np.int32), rng.integers(0, 200, size=(N, 2)).astype(np.int32)
    one_pc, two_pc = rng.integers(0, 200, size=(C, N)).astype(np.int32), rng.integers(0, 200, size=(C, N, 2)).astype(np.int32)
    skip = rng.random((C, N)) < 0.3
    for fields, cand, pc, full in ((1, one, False, one[:, None]), (FIELDS, two, False, two), ((6, 1), two, False, two),
                                   (1, one_pc, True, one_pc[:, :, None]), (FIELDS, two_pc, True, two_pc)):
        cols = [fields] if isinstance(fields, int) else list(fields)
        for sk in (None, skip):
            pos, val = tmodel.recommend_tuples(ctx, fields, cand, per_context=pc, k=k, skip=sk, score_rows=2 * N, sweep='tuples')
            calls = tmodel.engine.calls[:]
            assert _kinds(tmodel) == ['tuples_shared'] * 3                       # groups of 2 + 2 + 1 contexts, nothing else runs
            assert all(c[1] == cols for c in calls)                              # the caller's field order reaches the engine
            assert np.array_equal(np.concatenate([c[2] for c in calls]), ctx)
            if pc:
                assert np.array_equal(np.concatenate([c[3] for c in calls]), full)
            else:
                assert all(np.array_equal(c[3], full) for c in calls)
            idx, bits_, _ = R.topk_ref(_neg_scores(ctx, cols, full), k, sk)
            assert np.array_equal(pos, idx) and np.array_equal(val.view(np.uint32), bits_)
    # the other values are what they were: 'shared' refuses tuples, 'auto' sends them to expand
    with pytest.raises(ValueError, match='shared'):
        tmodel.recommend_tuples(ctx, FIELDS, two, sweep='shared')
    tmodel.recommend_tuples(ctx, FIELDS, two, sweep='auto')
    tmodel.recommend_tuples(ctx, FIELDS, two)
    assert _kinds(tmodel) == ['tuples', 'tuples']


def test_evaluate_takes_the_tuple_sweep(tmodel, data):  # noqa: F811
    test = data.Test_data
    ctx = _positives(test)
    distinct = np.unique(np.concatenate([_rows(data.Train_data), _rows(test)]), axis=0)
    target = np.array([int(np.nonzero((distinct == t).all(axis=1))[0][0]) for t in ctx[:, list(FIELDS)]])
    got = tmodel.evaluate_ranking_tuples(test, FIELDS, k=10, score_rows=3 * distinct.shape[0], sweep='tuples')
    calls = tmodel.engine.calls[:]
    assert set(_kinds(tmodel)) == {'tuples_shared'} and all(c[3].ndim == 2 and np.array_equal(c[3], distinct) for c in calls)
    ranks = R.rank_ref(_neg_scores(ctx, FIELDS, distinct), target)
    assert got == pytest.approx(M.ranking_metrics(ranks, 10), abs=1e-12)
    # the sampled protocol: a list per row goes to the same method
    got = tmodel.evaluate_ranking_tuples(test, FIELDS, k=3, negatives=7, seed=11, sweep='tuples')
    calls = tmodel.engine.calls[:]
    assert set(_kinds(tmodel)) == {'tuples_shared'} and all(c[3].ndim == 3 for c in calls)
    lists = np.concatenate([c[3] for c in calls])
    place = (lists == ctx[:, None, list(FIELDS)]).all(axis=2).argmax(axis=1)
    assert got == pytest.approx(M.ranking_metrics(R.rank_ref(_neg_scores(ctx, FIELDS, lists), place), 3), abs=1e-12)


def test_unserved_is_refused_by_name(tmodel, data, monkeypatch):  # noqa: F811
    ctx = np.asarray(data.Test_data['X'][:3], dtype=np.int32)
    three = np.arange(27, dtype=np.int32).reshape(9, 3)
    with pytest.raises(ValueError, match="'tuples'"):
        tmodel.recommend_tuples(ctx, (1, 6, 8), three, sweep='tuples')           # the stub serves nf = 1 and 2
    monkeypatch.setattr(_TupleStub, 'served_nf', ())
    with pytest.raises(ValueError, match="'tuples'"):
        tmodel.recommend_tuples(ctx, 1, np.arange(9, dtype=np.int32), sweep='tuples')
    with pytest.raises(ValueError, match="'tuples'"):
        tmodel.evaluate_ranking_tuples(data.Test_data, FIELDS, sweep='tuples')
    assert _kinds(tmodel) == []                                                  # refused before anything is scored
    for bad in ('tuple', 'TUPLES', None):
        with pytest.raises(ValueError, match='sweep'):
            tmodel.recommend_tuples(ctx, FIELDS, three[:, :2], sweep=bad)
