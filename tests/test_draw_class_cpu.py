"""The sampler keyword of CFFM.train_ranking and CFFM.evaluate_ranking_tuples on a stub engine (no GPU) whose draw_lists is the numpy
twin (cffm_amd.spec.draw_lists): sampler='device' hands the list step the twin's lists for list0 = epoch * P, the same under every
lists_per_step; sampler='host' hands over what the default does; evaluation draws list r for row r, every rank its own share; a bad
sampler and more than 1023 negatives raise."""
import numpy as np
import pytest
import torch

from cffm_amd import CFFM as M
from cffm_amd.spec import draw_lists
from tests import _rank_ref as R
from tests.test_rank_class_cpu import _score
from tests import _cand_ref as CR
from tests.test_rank_train_class_cpu import FIELDS, _StubEngine as _TrainStub, _positives, _steps, _whole, data  # noqa: F401


class _StubEngine(_TrainStub):
    """The list-step stub plus a draw_lists that is the twin and records its calls."""

    def __init__(self, cfg, seed):
        _TrainStub.__init__(self, cfg, seed)
        self.draws = []

    def draw_lists(self, seed, list0, at, U, m, cand=None):
        assert at.dtype in (torch.int32, torch.int64) and at.dim() == 1
        self.draws.append((int(seed), int(list0), int(at.shape[0]), int(U), int(m)))
        lists, place = draw_lists(seed, list0, at.numpy(), U, m)
        lists = torch.from_numpy(lists)
        tuples = None if cand is None else cand[lists].to(torch.int32).contiguous()
        return tuples, lists.to(torch.int32), torch.from_numpy(place.astype(np.int32))


@pytest.fixture
def model(tmp_path, data, monkeypatch):  # noqa: F811
    monkeypatch.setattr(M.CFFM, 'engine_factory', _StubEngine)
    monkeypatch.delenv('CFFM_TABLES', raising=False)
    m = M.CFFM(data.features_M, 0, str(tmp_path / 'm'), 8, 8, 'square_loss', 1, 16, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer', 0, 0, 0,
               10, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'relu')
    m.build_graph()
    return m


def _distinct(split):
    return np.unique(np.asarray(split['X'], dtype=np.int32)[:, list(FIELDS)], axis=0)


def _at(distinct, own):
    """Index in the sorted distinct tuples of every row of own."""
    return np.array([int(np.nonzero((distinct == t).all(axis=1))[0][0]) for t in own])


def test_device_sampler_hands_the_list_step_the_twins_lists(model, data):  # noqa: F811
    train = data.Train_data
    pos, distinct = _positives(train), _distinct(train)
    P, U, m, seed = pos.shape[0], distinct.shape[0], 4, 5
    model.train_ranking(train, FIELDS, negatives=m, epochs=2, lists_per_step=7, seed=seed, sampler='device')
    steps = _steps(model)
    assert [s[0].shape[0] for s in steps] == ([7] * (P // 7) + ([P % 7] if P % 7 else [])) * 2
    per_epoch = len(steps) // 2
    assert sum(d[2] for d in model.engine.draws) == 2 * P and all(d[0] == seed and d[3:] == (U, m) for d in model.engine.draws)
    for epoch in range(2):
        ctx, lists, target = _whole(steps[epoch * per_epoch:(epoch + 1) * per_epoch])
        perm = np.random.RandomState(seed + epoch).permutation(P)                # the epoch permutation stays the host's
        assert np.array_equal(ctx, pos[perm])
        at = _at(distinct, pos[perm][:, list(FIELDS)])
        want, place = draw_lists(seed, epoch * P, at, U, m)
        assert np.array_equal(lists, distinct[want]) and np.array_equal(target, place)
        assert np.array_equal(lists[np.arange(P), target], ctx[:, list(FIELDS)])
    # the same lists under another grouping
    del model.engine.draws[:]
    model.train_ranking(train, FIELDS, negatives=m, epochs=2, lists_per_step=1000, seed=seed, sampler='device')
    big = _steps(model)
    assert [s[0].shape[0] for s in big] == [P, P]
    for epoch in range(2):
        for a, b in zip(_whole(big[epoch:epoch + 1]), _whole(steps[epoch * per_epoch:(epoch + 1) * per_epoch])):
            assert np.array_equal(a, b)
    assert not np.array_equal(big[0][2], big[1][2])


def test_host_sampler_is_the_default(model, data):  # noqa: F811
    train = data.Train_data
    model.train_ranking(train, FIELDS, negatives=3, epochs=2, lists_per_step=9, seed=4)
    default = _steps(model)
    model.train_ranking(train, FIELDS, negatives=3, epochs=2, lists_per_step=9, seed=4, sampler='host')
    host = _steps(model)
    assert model.engine.draws == [] and len(host) == len(default)
    for a, b in zip(host, default):
        assert all(np.array_equal(x, y) for x, y in zip(a[:1] + a[2:4], b[:1] + b[2:4])) and a[1] == b[1] and a[4] == b[4]
    # and it is the stream documented for it: the permutation, then one permutation of the set without the target per row
    pos, distinct = _positives(train), _distinct(train)
    P, U = pos.shape[0], distinct.shape[0]
    rng = np.random.RandomState(4)
    perm = rng.permutation(P)
    at = _at(distinct, pos[perm][:, list(FIELDS)])
    neg = np.stack([rng.permutation(U - 1)[:3] for _ in range(P)])
    neg = neg + (neg >= at[:, None])
    ctx, lists, target = _whole(default[:len(default) // 2])
    assert np.array_equal(ctx, pos[perm])
    rest = np.stack([np.delete(row, t, axis=0) for row, t in zip(lists, target)])
    assert np.array_equal(np.sort(rest.reshape(P, -1), axis=1), np.sort(distinct[neg].reshape(P, -1), axis=1))
    model.train_ranking(train, FIELDS, negatives=3, epochs=1, lists_per_step=9, seed=4, sampler='device')
    assert not np.array_equal(_whole(_steps(model))[1], lists)                   # another stream, not another spelling of this one


def test_evaluation_draws_list_r_for_row_r(model, data):  # noqa: F811
    model._train_split = data.Train_data
    test = data.Test_data
    pos = _positives(test)
    distinct = np.unique(np.concatenate([_distinct(data.Train_data), _distinct(test)]), axis=0)
    P, U, m, seed, k = pos.shape[0], distinct.shape[0], 3, 11, 2
    at = _at(distinct, pos[:, list(FIELDS)])
    want, place = draw_lists(seed, 0, at, U, m)
    scores = _score(CR.expand_tuples(pos, list(FIELDS), distinct[want])).reshape(P, m + 1)
    ranks = R.rank_ref(scores, place)
    got = model.evaluate_ranking_tuples(test, FIELDS, k=k, negatives=m, seed=seed, sampler='device')
    assert got == pytest.approx(R.metrics_ref(ranks, k), rel=1e-12)
    assert model.engine.draws == [(seed, 0, P, U, m)]
    handed = np.concatenate([c[3] for c in model.engine.calls])
    assert np.array_equal(handed, distinct[want])
    # under a process group every rank draws its own rows only, at list0 = its first row: the shares add up to the whole
    model._all_reduce_sum = lambda t: t
    share = -(-P // 2)
    parts = []
    for rank in (0, 1):
        del model.engine.draws[:], model.engine.calls[:]
        model.world, model.rank = 2, rank
        model.evaluate_ranking_tuples(test, FIELDS, k=k, negatives=m, seed=seed, sampler='device')
        r0, r1 = min(rank * share, P), min((rank + 1) * share, P)
        assert model.engine.draws == [(seed, r0, r1 - r0, U, m)]
        parts.append(np.concatenate([c[3] for c in model.engine.calls]))
    model.world, model.rank = 1, 0
    assert np.array_equal(np.concatenate(parts), distinct[want])


def test_refusals(model, data):  # noqa: F811
    train = data.Train_data
    for bad in ('gpu', 'Device', None, 1):
        with pytest.raises(ValueError, match='sampler must be .*%s' % (repr(bad).replace('(', r'\(').replace(')', r'\)'),)):
            model.train_ranking(train, FIELDS, sampler=bad)
        with pytest.raises(ValueError, match='sampler must be .*%s' % (repr(bad),)):
            model.evaluate_ranking_tuples(data.Test_data, FIELDS, negatives=3, sampler=bad)
    with pytest.raises(ValueError, match='1023'):
        model.train_ranking(train, FIELDS, negatives=1024, sampler='device')
    with pytest.raises(ValueError, match='1023'):
        model.evaluate_ranking_tuples(data.Test_data, FIELDS, negatives=1024, sampler='device')
    assert _steps(model) == [] and model.engine.draws == []
