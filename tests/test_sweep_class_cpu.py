"""CFFM.recommend / CFFM.evaluate_ranking(sweep=...) on a stub engine (no GPU): which of the engine's two scoring methods runs
under 'expand', 'shared' and 'auto' on both sides of SWEEP_MIN_N, what is refused, and that the default still calls
score_candidates with exactly the arguments it always received."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from cffm_amd import CFFM as M
from cffm_amd.LoadData import LoadData
from tests import _rank_ref as R
from tests.test_rank_class_cpu import _score

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'golden', 'frappe_slice') + '/'
FIELD = 1


class _StubEngine(object):
    """Both scoring methods over the same plain function of the ids; every call is recorded with its arguments."""
    device = torch.device('cpu')
    opt_step = 0
    served = True

    def __init__(self, cfg, seed):
        self.cfg, self.calls = cfg, []

    def sweep_ok(self):
        return self.served

    def _scores(self, ctx, field, cand):
        ctx, cand = ctx.numpy(), cand.numpy()
        C, N = ctx.shape[0], cand.size
        return torch.from_numpy(_score(R.expand_ref(ctx, field, cand, 0, C * N)).reshape(C, N))

    def score_candidates(self, *args, **kwargs):
        self.calls.append(('expand', args, kwargs))
        return self._scores(*args)

    def score_candidates_shared(self, *args, **kwargs):
        self.calls.append(('shared', args, kwargs))
        if not self.served:
            raise ValueError('not served')
        return self._scores(*args)

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
    m._train_split = data.Train_data
    return m


def _paths(m):
    kinds = [c[0] for c in m.engine.calls]
    del m.engine.calls[:]
    return kinds


CAND = np.arange(20, 50, dtype=np.int32)                                    # N = 30


def _both(m, data, **kw):
    """One recommend and one evaluate_ranking call; returns their results and the scoring methods that ran."""
    ctx = np.asarray(data.Test_data['X'][:5], dtype=np.int32)
    rec = m.recommend(ctx, FIELD, candidates=CAND, k=4, score_rows=2 * CAND.size, **kw)
    kinds = _paths(m)
    ev = m.evaluate_ranking(data.Test_data, FIELD, k=10, **kw)
    return rec, ev, kinds, _paths(m)


def test_sweep_min_n_is_a_module_constant():
    assert M.SWEEP_MIN_N is None or (isinstance(M.SWEEP_MIN_N, int) and M.SWEEP_MIN_N >= 1)


def test_the_default_is_expand_called_as_before(model, data):
    ctx = np.asarray(data.Test_data['X'][:3], dtype=np.int32)
    model.recommend(ctx, FIELD, candidates=CAND, k=4)
    (kind, args, kwargs), = model.engine.calls
    assert kind == 'expand' and kwargs == {} and len(args) == 3                # eng.score_candidates(ctx, field, cand)
    assert isinstance(args[0], torch.Tensor) and args[0].dtype == torch.int32 and np.array_equal(args[0].numpy(), ctx)
    assert type(args[1]) is int and args[1] == FIELD
    assert isinstance(args[2], torch.Tensor) and args[2].dtype == torch.int32 and np.array_equal(args[2].numpy(), CAND)
    del model.engine.calls[:]
    model.evaluate_ranking(data.Test_data, FIELD, k=10)
    assert model.engine.calls and all(c[0] == 'expand' and c[2] == {} and len(c[1]) == 3 and c[1][1] == FIELD
                                      for c in model.engine.calls)
    del model.engine.calls[:]
    rec_d, ev_d, k1, k2 = _both(model, data)
    rec_e, ev_e, k3, k4 = _both(model, data, sweep='expand')
    assert set(k1 + k2 + k3 + k4) == {'expand'} and k1 == ['expand'] * 3      # 5 contexts in groups of two
    assert np.array_equal(rec_d[0], rec_e[0]) and np.array_equal(rec_d[1].view(np.uint32), rec_e[1].view(np.uint32)) and ev_d == ev_e


def test_shared_uses_the_new_path(model, data):
    rec_d, ev_d, _, _ = _both(model, data)
    rec_s, ev_s, k1, k2 = _both(model, data, sweep='shared')
    assert set(k1) == {'shared'} and set(k2) == {'shared'} and len(k1) == 3
    assert np.array_equal(rec_d[0], rec_s[0]) and ev_d == ev_s                # the stub's two methods return the same scores


def test_auto_on_both_sides_of_sweep_min_n(model, data, monkeypatch):
    ctx = np.asarray(data.Test_data['X'][:5], dtype=np.int32)
    for min_n, want in ((CAND.size, 'shared'), (CAND.size - 1, 'shared'), (1, 'shared'), (CAND.size + 1, 'expand'), (None, 'expand')):
        monkeypatch.setattr(M, 'SWEEP_MIN_N', min_n)
        model.recommend(ctx, FIELD, candidates=CAND, k=4, sweep='auto')
        assert set(_paths(model)) == {want}, (min_n, want)
    # evaluate_ranking's default candidates: N = the distinct ids of the column over both splits
    col = lambda split: {row[FIELD] for row in split['X']}
    N = len(col(data.Train_data) | col(data.Test_data))
    for min_n, want in ((N, 'shared'), (N + 1, 'expand')):
        monkeypatch.setattr(M, 'SWEEP_MIN_N', min_n)
        model.evaluate_ranking(data.Test_data, FIELD, k=10, sweep='auto')
        assert set(_paths(model)) == {want}, (min_n, want)
    # a shape the shared sweep does not serve: 'auto' is the default path whatever N is
    monkeypatch.setattr(M, 'SWEEP_MIN_N', 1)
    monkeypatch.setattr(_StubEngine, 'served', False)
    model.recommend(ctx, FIELD, candidates=CAND, k=4, sweep='auto')
    model.evaluate_ranking(data.Test_data, FIELD, k=10, sweep='auto')
    assert set(_paths(model)) == {'expand'}


def test_refusals(model, data, monkeypatch):
    ctx = np.asarray(data.Test_data['X'][:2], dtype=np.int32)
    for bad in ('fast', '', None, 'EXPAND', 1):
        with pytest.raises(ValueError, match='sweep'):
            model.recommend(ctx, FIELD, candidates=CAND, k=2, sweep=bad)
        with pytest.raises(ValueError, match='sweep'):
            model.evaluate_ranking(data.Test_data, FIELD, sweep=bad)
    assert _paths(model) == []                                                # refused before anything is scored
    monkeypatch.setattr(_StubEngine, 'served', False)
    with pytest.raises(ValueError, match='shared'):
        model.recommend(ctx, FIELD, candidates=CAND, k=2, sweep='shared')
    with pytest.raises(ValueError, match='shared'):
        model.evaluate_ranking(data.Test_data, FIELD, sweep='shared')
    assert _paths(model) == []
