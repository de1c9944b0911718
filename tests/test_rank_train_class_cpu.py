"""CFFM.train_ranking on a stub engine (no GPU): what lists it hands the engine's list step - every list holds its row's own tuple at
`target`, distinct negatives without it, the same seed the same lists and another epoch others - the default lists_per_step, every
ValueError, and that the drawing code it shares with evaluate_ranking_tuples(negatives=m, seed) left that method's random stream
alone: the lists its scorer is handed are those recorded before the helper was factored out (tests/golden/rank_tuples_sampled_lists.npz)."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from cffm_amd import CFFM as M
from cffm_amd.LoadData import LoadData
from tests.test_rank_tuples_class_cpu import _StubEngine as _RankStub

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'golden', 'frappe_slice') + '/'
FIELDS = (1, 6)


class _StubEngine(_RankStub):
    """The ranking stub plus a list step that records its arguments and returns a loss that falls from call to call."""

    def __init__(self, cfg, seed):
        _RankStub.__init__(self, cfg, seed)
        self.steps = []

    def train_step_lists(self, ctx, fields, cand, target, kind):
        assert cand.is_contiguous() and cand.dtype == torch.int32 and target.dtype == torch.int32
        self.steps.append((ctx.numpy().copy(), list(fields), cand.numpy().copy(), target.numpy().copy(), kind))
        return torch.tensor([1.0 / len(self.steps)])


@pytest.fixture(scope='module')
def data():
    with contextlib.redirect_stdout(io.StringIO()):
        return LoadData(PATH, 'frappe', 'square_loss')


def _model(tmp_path, data, monkeypatch, loss_type='square_loss', optimizer='AdagradOptimizer', batch_size=16):
    monkeypatch.setattr(M.CFFM, 'engine_factory', _StubEngine)
    monkeypatch.delenv('CFFM_TABLES', raising=False)
    m = M.CFFM(data.features_M, 0, str(tmp_path / 'm'), 8, 8, loss_type, 1, batch_size, 0.05, 0, [1.0, 1.0], optimizer, 0, 0, 0,
               10, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'relu')
    m.build_graph()
    return m


@pytest.fixture
def model(tmp_path, data, monkeypatch):
    return _model(tmp_path, data, monkeypatch)


def _steps(m):
    steps = m.engine.steps[:]
    del m.engine.steps[:]
    return steps


def _whole(steps):
    return (np.concatenate([s[0] for s in steps]), np.concatenate([s[2] for s in steps]), np.concatenate([s[3] for s in steps]))


def _positives(split):
    X, Y = np.asarray(split['X'], dtype=np.int32), np.asarray(split['Y']).reshape(-1)
    return X[Y > 0]


def test_the_lists_of_an_epoch(model, data):
    train = data.Train_data
    pos = _positives(train)
    P, m = pos.shape[0], 4
    distinct = np.unique(np.asarray(train['X'], dtype=np.int32)[:, list(FIELDS)], axis=0)
    known = {tuple(t) for t in distinct.tolist()}
    means = model.train_ranking(train, FIELDS, negatives=m, loss='bpr', epochs=1, lists_per_step=7, seed=5)
    steps = _steps(model)
    assert [s[0].shape[0] for s in steps] == [7] * (P // 7) + ([P % 7] if P % 7 else [])          # ragged last step
    assert all(s[1] == list(FIELDS) and s[4] == 'bpr' and s[2].shape[1:] == (m + 1, 2) for s in steps)
    ctx, lists, target = _whole(steps)
    # the positives, each once, permuted by RandomState(seed + epoch)
    perm = np.random.RandomState(5).permutation(P)
    assert np.array_equal(ctx, pos[perm]) and not np.array_equal(ctx, pos)
    # every list holds its row's own tuple at `target`, and nowhere else; the negatives are distinct tuples of the distinct set
    own = ctx[:, list(FIELDS)]
    assert np.array_equal(lists[np.arange(P), target], own)
    assert ((lists == own[:, None, :]).all(axis=2).sum(axis=1) == 1).all()
    for row in lists:
        rows = [tuple(t) for t in row.tolist()]
        assert len(set(rows)) == m + 1 and set(rows) <= known
    assert ((target >= 0) & (target <= m)).all() and np.unique(target).size > 1                    # drawn, not fixed
    # the mean over the lists of the step losses (the stub's k-th step returns 1 / k as float32, summed in float64)
    sizes = np.array([s[0].shape[0] for s in steps], dtype=np.float64)
    step_loss = (1.0 / np.arange(1, len(steps) + 1)).astype(np.float32).astype(np.float64)
    assert means == pytest.approx([float((sizes * step_loss).sum() / P)], rel=1e-12)
    # the same seed gives the same lists whatever the grouping; epoch e of seed s is epoch 0 of seed s + e; another epoch gives others
    model.train_ranking(train, FIELDS, negatives=m, epochs=2, lists_per_step=1000, seed=5)
    two = _steps(model)
    assert [s[0].shape[0] for s in two] == [P, P]
    assert all(np.array_equal(a, b) for a, b in zip(_whole(two[:1]), (ctx, lists, target)))
    assert not np.array_equal(two[1][2], two[0][2]) and not np.array_equal(two[1][0], two[0][0])
    model.train_ranking(train, FIELDS, negatives=m, loss='softmax', epochs=1, lists_per_step=1000, seed=6)
    six = _steps(model)
    assert six[0][4] == 'softmax' and all(np.array_equal(a, b) for a, b in zip(_whole(six), _whole(two[1:])))


def test_default_lists_per_step(tmp_path, data, monkeypatch):
    m = _model(tmp_path, data, monkeypatch, batch_size=23)
    P = _positives(data.Train_data).shape[0]
    for neg, per in ((4, 4), (1, 11), (22, 1)):                                # batch_size // (negatives + 1)
        m.train_ranking(data.Train_data, FIELDS, negatives=neg)
        sizes = [s[0].shape[0] for s in _steps(m)]
        assert sizes[:-1] == [per] * (len(sizes) - 1) and sum(sizes) == P and 0 < sizes[-1] <= per
    with pytest.raises(ValueError, match='lists_per_step'):
        m.train_ranking(data.Train_data, FIELDS, negatives=23)                 # a batch that holds no list
    with pytest.raises(ValueError, match='lists_per_step'):
        m.train_ranking(data.Train_data, FIELDS, lists_per_step=0)
    assert _steps(m) == []


def test_refusals(tmp_path, data, monkeypatch, model):
    train = data.Train_data
    U = np.unique(np.asarray(train['X'], dtype=np.int32)[:, list(FIELDS)], axis=0).shape[0]
    for bad in (0, -1, U, U + 3):
        with pytest.raises(ValueError, match=r'negatives must be in \[1, %d\)' % U):
            model.train_ranking(train, FIELDS, negatives=bad)
    with pytest.raises(ValueError, match='loss must be'):
        model.train_ranking(train, FIELDS, loss='hinge')
    with pytest.raises(ValueError, match='fields'):
        model.train_ranking(train, (1, 1))
    none = {'X': [x for x, y in zip(train['X'], train['Y']) if np.asarray(y).reshape(-1)[0] <= 0][:20]}
    none['Y'] = [-1.0] * len(none['X'])
    assert len(none['X']) > 0
    with pytest.raises(ValueError, match='positive label'):
        model.train_ranking(none, FIELDS)
    # a process group, and row-sharded tables
    model.world = 2
    with pytest.raises(ValueError, match='process group of 2 ranks'):
        model.train_ranking(train, FIELDS)
    model.world = 1
    model._sh = object()
    with pytest.raises(ValueError, match='CFFM_TABLES=sharded'):
        model.train_ranking(train, FIELDS)
    model._sh = None
    monkeypatch.setenv('CFFM_TABLES', 'sharded')
    with pytest.raises(ValueError, match='CFFM_TABLES=sharded'):
        model.train_ranking(train, FIELDS)
    monkeypatch.delenv('CFFM_TABLES')
    assert _steps(model) == []
    # the optimizers the list step does not implement, and log_loss, by name
    for opt in ('AdamOptimizer', 'GradientDescentOptimizer', 'MomentumOptimizer'):
        other = _model(tmp_path, data, monkeypatch, optimizer=opt)
        with pytest.raises(ValueError, match=opt):
            other.train_ranking(train, FIELDS)
        assert _steps(other) == []
    logm = _model(tmp_path, data, monkeypatch, loss_type='log_loss')
    with pytest.raises(ValueError, match='log_loss'):
        logm.train_ranking(train, FIELDS)
    assert _steps(logm) == []


def test_evaluate_ranking_tuples_hands_its_scorer_the_recorded_lists(model, data):
    """The sampled protocol's lists, recorded through the same stub before its drawing code became the helper train_ranking shares."""
    gold = np.load(os.path.join(HERE, 'golden', 'rank_tuples_sampled_lists.npz'))
    model._train_split = data.Train_data
    for neg, seed in ((7, 11), (3, 0)):
        del model.engine.calls[:]
        got = model.evaluate_ranking_tuples(data.Test_data, FIELDS, k=3, negatives=neg, seed=seed)
        calls = model.engine.calls
        tag = 'm%d_s%d' % (neg, seed)
        assert np.array_equal(np.concatenate([c[2] for c in calls]), gold['ctx_' + tag])
        assert np.array_equal(np.concatenate([c[3] for c in calls]), gold['lists_' + tag])
        assert np.array_equal(np.asarray(got, dtype=np.float64), gold['metrics_' + tag])
