"""CFFM.recommend / CFFM.evaluate_ranking on a stub engine (no GPU): what they refuse, and the host logic around the three engine
calls - default candidates, the cut of the contexts into groups, the target's position among explicit candidates, the mapping of
candidate positions back to feature ids and the metric sums - with the engine's score / top-k / rank-of replaced by the numpy
references of tests/_rank_ref.py over a score that is a plain function of the ids."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from cffm_amd import CFFM as M
from cffm_amd.LoadData import LoadData
from tests import _rank_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'golden', 'frappe_slice') + '/'
FIELD = 1


def _score(ids):
    """A score with many ties that depends on every id of the row."""
    ids = np.asarray(ids, dtype=np.int64)
    return (((ids * np.arange(1, ids.shape[1] + 1)).sum(axis=1) * 2654435761) % 7).astype(np.float32) - 3.0


class _StubEngine(object):
    device = torch.device('cpu')
    opt_step = 0

    def __init__(self, cfg, seed):
        self.cfg, self.calls = cfg, []

    def score_candidates(self, ctx, field, cand, block=8192):
        ctx, cand = ctx.numpy(), cand.numpy()
        C, N = ctx.shape[0], cand.size
        self.calls.append(C)
        return torch.from_numpy(_score(R.expand_ref(ctx, field, cand, 0, C * N)).reshape(C, N))

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
    monkeypatch.delenv('CFFM_TABLES', raising=False)
    m = M.CFFM(data.features_M, 0, str(tmp_path / 'm'), 8, 8, 'square_loss', 1, 16, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer', 0, 0, 0,
               10, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'relu')
    m.build_graph()
    return m


def _column(split, field=FIELD):
    return np.array([row[field] for row in split['X']], dtype=np.int64)


def test_recommend_without_a_train_split_raises(model, data):
    ctx = np.asarray(data.Test_data['X'][:2])
    with pytest.raises(ValueError, match='train split'):
        model.recommend(ctx, FIELD)
    ids, _ = model.recommend(ctx, FIELD, candidates=[3, 4, 5], k=2)          # explicit candidates need none
    assert ids.shape == (2, 2) and set(ids.reshape(-1)) <= {3, 4, 5}


def test_evaluate_ranking_names_the_first_missing_target(model, data):
    tgt = _column(data.Test_data)[np.asarray(data.Test_data['Y']) > 0]
    distinct = tgt[np.sort(np.unique(tgt, return_index=True)[1])]           # in order of first appearance
    assert distinct.size >= 3
    cand = np.setdiff1d(np.union1d(_column(data.Train_data), tgt), distinct[[1, 2]])     # two targets are no candidates
    first = int(distinct[1])                                                  # the one a row meets first is named
    with pytest.raises(ValueError, match=r'target id %d ' % first):
        model.evaluate_ranking(data.Test_data, FIELD, candidates=cand)


def test_both_refuse_row_sharded_tables(model, data):
    model._sh = object()
    msg = 'CFFM_TABLES=sharded: recommend / evaluate_ranking run on replicated tables'
    with pytest.raises(ValueError) as e:
        model.recommend(np.asarray(data.Test_data['X'][:2]), FIELD, candidates=[1, 2])
    assert str(e.value) == msg
    with pytest.raises(ValueError) as e:
        model.evaluate_ranking(data.Test_data, FIELD)
    assert str(e.value) == msg


def test_recommend_maps_positions_to_ids_in_groups(model, data):
    model._train_split = data.Train_data                                    # what train() records
    cand = np.unique(_column(data.Train_data)).astype(np.int32)             # the default: sorted distinct ids of the train column
    ctx = np.asarray(data.Test_data['X'][:5], dtype=np.int32)
    N = cand.size
    skip = np.zeros((5, N), dtype=bool)
    skip[1, :] = True
    skip[2, 2:] = True
    skip[3, ::2] = True
    k = 4
    ids, val = model.recommend(ctx, FIELD, k=k, skip=skip, score_rows=2 * N)  # groups of two contexts: 2 + 2 + 1
    assert model.engine.calls == [2, 2, 1]
    scores = _score(R.expand_ref(ctx, FIELD, cand, 0, 5 * N)).reshape(5, N)
    idx, bits_, count = R.topk_ref(scores, k, skip)
    assert count.tolist() == [k, 0, 2, k]+ [k]
    assert ids.dtype == np.int32 and val.dtype == np.float32
    assert np.array_equal(ids, np.where(idx >= 0, cand[np.maximum(idx, 0)], -1))
    assert np.array_equal(val.view(np.uint32), bits_)
    for bad_k in (0, 1025):
        with pytest.raises(ValueError):
            model.recommend(ctx, FIELD, k=bad_k)


@pytest.mark.parametrize('explicit', [False, True])
def test_evaluate_ranking_equals_the_host_metrics(model, data, explicit):
    model._train_split = data.Train_data
    test = data.Test_data
    pos = np.asarray(test['Y']) > 0
    ctx = np.asarray(test['X'], dtype=np.int32)[pos]
    cand = np.union1d(_column(data.Train_data), _column(test)).astype(np.int32)
    if explicit:
        cand = cand[np.random.default_rng(3).permutation(cand.size)]         # an unsorted list: positions are the caller's
    scores = _score(R.expand_ref(ctx, FIELD, cand, 0, ctx.shape[0] * cand.size)).reshape(ctx.shape[0], cand.size)
    target = np.array([int(np.nonzero(cand == t)[0][0]) for t in ctx[:, FIELD]])
    ranks = R.rank_ref(scores, target)
    assert (ranks >= 0).all() and 0 < (ranks < 10).sum() < ranks.size          # the case separates hits from misses
    got = model.evaluate_ranking(test, FIELD, k=10, candidates=cand if explicit else None, score_rows=3 * cand.size)
    want = M.ranking_metrics(ranks, 10)
    assert got == pytest.approx(want, abs=1e-12) and want == pytest.approx(R.metrics_ref(ranks, 10), abs=1e-12)
    assert sum(model.engine.calls) == ctx.shape[0] and max(model.engine.calls) == 3


def test_evaluate_ranking_raises_on_nan(model, data, monkeypatch):
    def nan_scores(self, ctx, field, cand, block=8192):
        out = torch.zeros((ctx.shape[0], cand.numel()))
        out[0, 0] = float('nan')
        return out
    monkeypatch.setattr(_StubEngine, 'score_candidates', nan_scores)
    with pytest.raises(ValueError, match='NaN'):
        model.evaluate_ranking(data.Test_data, FIELD)
