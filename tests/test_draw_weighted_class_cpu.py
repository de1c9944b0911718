"""negative_weights / negative_power of CFFM.train_ranking and CFFM.evaluate_ranking_tuples on a stub engine (no GPU) whose
draw_lists_weighted is the numpy twin (cffm_amd.spec.draw_lists_weighted): the list ids and the cdf the class hands over, the
'popularity' counts and power, the default path untouched (no weighted draw), and every new ValueError."""
import numpy as np
import pytest
import torch

from cffm_amd import CFFM as M
from cffm_amd.spec import draw_lists, draw_lists_weighted, weight_cdf
from tests import _rank_ref as R
from tests.test_rank_class_cpu import _score
from tests import _cand_ref as CR
from tests.test_draw_class_cpu import _StubEngine as _DrawStub, _at, _distinct
from tests.test_rank_train_class_cpu import FIELDS, _positives, _steps, _whole, data  # noqa: F401


class _StubEngine(_DrawStub):
    """The uniform-draw stub plus a draw_lists_weighted that is the twin and records its calls, the cdf words included."""

    def __init__(self, cfg, seed):
        _DrawStub.__init__(self, cfg, seed)
        self.wdraws = []

    def draw_lists_weighted(self, seed, list0, at, cdf, m, cand=None):
        assert at.dtype in (torch.int32, torch.int64) and at.dim() == 1
        assert cdf.dtype == torch.int32 and cdf.dim() == 1
        words = cdf.numpy().view(np.uint32).copy()
        self.wdraws.append((int(seed), int(list0), int(at.shape[0]), int(m), words))
        lists, place = draw_lists_weighted(seed, list0, at.numpy(), words, m)
        lists = torch.from_numpy(lists)
        tuples = None
        if cand is not None:
            tuples = torch.where((lists >= 0)[:, :, None], cand[lists.clamp(min=0)], torch.zeros_like(cand[:1])).to(torch.int32).contiguous()
        return tuples, lists.to(torch.int32), torch.from_numpy(place.astype(np.int32))


@pytest.fixture
def model(tmp_path, data, monkeypatch):  # noqa: F811
    monkeypatch.setattr(M.CFFM, 'engine_factory', _StubEngine)
    monkeypatch.delenv('CFFM_TABLES', raising=False)
    m = M.CFFM(data.features_M, 0, str(tmp_path / 'm'), 8, 8, 'square_loss', 1, 16, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer', 0, 0, 0,
               10, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'relu')
    m.build_graph()
    return m


def _counts(*splits):
    """(distinct tuples, occurrence counts over all rows of the splits, any label), in lexicographic order."""
    rows = np.concatenate([np.asarray(s['X'], dtype=np.int32)[:, list(FIELDS)] for s in splits])
    return np.unique(rows, axis=0, return_counts=True)


def test_popularity_hands_the_list_step_the_twins_lists(model, data):  # noqa: F811
    train = data.Train_data
    pos = _positives(train)
    distinct, counts = _counts(train)
    assert np.array_equal(distinct, _distinct(train)) and counts.max() > 1       # the counts do differ
    P, U, m, seed = pos.shape[0], distinct.shape[0], 4, 5
    for power in (0.75, 0.5):
        cdf = weight_cdf(counts.astype(np.float64) ** power)
        del model.engine.wdraws[:]
        kw = {} if power == 0.75 else dict(negative_power=power)                 # 0.75 is the default
        model.train_ranking(train, FIELDS, negatives=m, epochs=2, lists_per_step=7, seed=seed, sampler='device',
                            negative_weights='popularity', **kw)
        steps = _steps(model)
        per_epoch = len(steps) // 2
        assert model.engine.draws == [] and [d[:4] for d in model.engine.wdraws] == [(seed, 0, P, m), (seed, P, P, m)]
        assert all(np.array_equal(d[4], cdf) for d in model.engine.wdraws)
        for epoch in range(2):
            ctx, lists, target = _whole(steps[epoch * per_epoch:(epoch + 1) * per_epoch])
            perm = np.random.RandomState(seed + epoch).permutation(P)            # the epoch permutation stays the host's
            assert np.array_equal(ctx, pos[perm])
            want, place = draw_lists_weighted(seed, epoch * P, _at(distinct, pos[perm][:, list(FIELDS)]), cdf, m)
            assert (place >= 0).all()
            assert np.array_equal(lists, distinct[want]) and np.array_equal(target, place)
    # an array of weights is taken as it is, in the order of the distinct set; a zero weight is never drawn
    w = np.arange(U) % 3 * 1.0
    del model.engine.wdraws[:]
    model.train_ranking(train, FIELDS, negatives=m, epochs=1, lists_per_step=1000, seed=seed, sampler='device', negative_weights=w)
    assert len(model.engine.wdraws) == 1 and np.array_equal(model.engine.wdraws[0][4], weight_cdf(w))
    ctx, lists, target = _whole(_steps(model))
    never = {tuple(t) for t in distinct[w == 0]}
    for row, t in zip(lists, target):
        assert not any(tuple(c) in never for p, c in enumerate(row) if p != t)
    # equal weights are not the uniform device lists
    model.train_ranking(train, FIELDS, negatives=m, epochs=1, lists_per_step=1000, seed=seed, sampler='device', negative_weights=np.ones(U))
    equal = _whole(_steps(model))[1]
    model.train_ranking(train, FIELDS, negatives=m, epochs=1, lists_per_step=1000, seed=seed, sampler='device')
    assert not np.array_equal(equal, _whole(_steps(model))[1])


def test_the_default_path_is_untouched(model, data):  # noqa: F811
    train = data.Train_data
    P, U = _positives(train).shape[0], _distinct(train).shape[0]
    runs = []
    for kw in (dict(), dict(negative_weights=None), dict(negative_weights=None, negative_power=0.1)):
        del model.engine.draws[:]
        model.train_ranking(train, FIELDS, negatives=3, epochs=2, lists_per_step=9, seed=4, sampler='device', **kw)
        assert model.engine.draws == [(4, 0, P, U, 3), (4, P, P, U, 3)] and model.engine.wdraws == []
        runs.append(_steps(model))
    for other in runs[1:]:
        assert len(other) == len(runs[0])
        for a, b in zip(other, runs[0]):
            assert all(np.array_equal(x, y) for x, y in zip(a[:1] + a[2:4], b[:1] + b[2:4])) and a[1] == b[1] and a[4] == b[4]
    model.train_ranking(train, FIELDS, negatives=3, epochs=1, lists_per_step=9, seed=4, negative_weights=None)     # the host sampler
    host = _steps(model)
    model.train_ranking(train, FIELDS, negatives=3, epochs=1, lists_per_step=9, seed=4)
    assert all(np.array_equal(a[2], b[2]) for a, b in zip(host, _steps(model))) and model.engine.wdraws == []
    model._train_split = data.Train_data
    del model.engine.draws[:]
    a = model.evaluate_ranking_tuples(data.Test_data, FIELDS, k=2, negatives=3, seed=11, sampler='device')
    b = model.evaluate_ranking_tuples(data.Test_data, FIELDS, k=2, negatives=3, seed=11, sampler='device', negative_weights=None)
    assert a == b and model.engine.wdraws == [] and len(model.engine.draws) == 2 and model.engine.draws[0] == model.engine.draws[1]


def test_evaluation_counts_both_splits_and_draws_list_r_for_row_r(model, data):  # noqa: F811
    model._train_split = data.Train_data
    test = data.Test_data
    pos = _positives(test)
    distinct, counts = _counts(data.Train_data, test)
    P, U, m, seed, k = pos.shape[0], distinct.shape[0], 3, 11, 2
    cdf = weight_cdf(counts.astype(np.float64) ** 0.75)
    at = _at(distinct, pos[:, list(FIELDS)])
    want, place = draw_lists_weighted(seed, 0, at, cdf, m)
    assert (place >= 0).all()
    scores = _score(CR.expand_tuples(pos, list(FIELDS), distinct[want])).reshape(P, m + 1)
    ranks = R.rank_ref(scores, place)
    got = model.evaluate_ranking_tuples(test, FIELDS, k=k, negatives=m, seed=seed, sampler='device', negative_weights='popularity')
    assert got == pytest.approx(R.metrics_ref(ranks, k), rel=1e-12)
    assert [d[:4] for d in model.engine.wdraws] == [(seed, 0, P, m)] and np.array_equal(model.engine.wdraws[0][4], cdf)
    assert model.engine.draws == []
    assert np.array_equal(np.concatenate([c[3] for c in model.engine.calls]), distinct[want])
    assert not np.array_equal(want, draw_lists(seed, 0, at, U, m)[0])
    # under a process group every rank draws its own rows only, at list0 = its first row: the shares add up to the whole
    model._all_reduce_sum = lambda t: t
    share = -(-P // 2)
    parts = []
    for rank in (0, 1):
        del model.engine.wdraws[:], model.engine.calls[:]
        model.world, model.rank = 2, rank
        model.evaluate_ranking_tuples(test, FIELDS, k=k, negatives=m, seed=seed, sampler='device', negative_weights='popularity')
        r0, r1 = min(rank * share, P), min((rank + 1) * share, P)
        assert [d[:4] for d in model.engine.wdraws] == [(seed, r0, r1 - r0, m)]
        parts.append(np.concatenate([c[3] for c in model.engine.calls]))
    model.world, model.rank = 1, 0
    assert np.array_equal(np.concatenate(parts), distinct[want])
    # explicit candidates: an array serves, 'popularity' has nothing to count
    del model.engine.wdraws[:]
    w = 1.0 + np.arange(U) % 5
    model.evaluate_ranking_tuples(test, FIELDS, k=k, candidates=distinct, negatives=m, seed=seed, sampler='device', negative_weights=w)
    assert np.array_equal(model.engine.wdraws[0][4], weight_cdf(w))
    with pytest.raises(ValueError, match='negative_weights.*array'):
        model.evaluate_ranking_tuples(test, FIELDS, k=k, candidates=distinct, negatives=m, sampler='device', negative_weights='popularity')


def test_refusals(model, data):  # noqa: F811
    train, test = data.Train_data, data.Test_data
    U = _distinct(train).shape[0]
    model._train_split = train
    Ue = _counts(train, test)[0].shape[0]
    calls = [(lambda **kw: model.train_ranking(train, FIELDS, negatives=3, **kw), U),
             (lambda **kw: model.evaluate_ranking_tuples(test, FIELDS, negatives=3, **kw), Ue)]
    for call, n in calls:
        for kw in (dict(), dict(sampler='host')):                                # only 'device' serves it
            with pytest.raises(ValueError, match="negative_weights needs sampler='device'"):
                call(negative_weights='popularity', **kw)
            with pytest.raises(ValueError, match="negative_weights needs sampler='device'"):
                call(negative_weights=np.ones(n), **kw)
        for bad in (np.ones(n + 1), np.ones(n - 1), np.ones((n, 1)), 2.0):
            with pytest.raises(ValueError, match='negative_weights must hold one weight per distinct tuple'):
                call(negative_weights=bad, sampler='device')
        for j, v in ((0, -1.0), (1, np.nan), (n - 1, np.inf)):
            w = np.ones(n)
            w[j] = v
            with pytest.raises(ValueError, match='negative_weights must be non-negative and finite'):
                call(negative_weights=w, sampler='device')
        with pytest.raises(ValueError, match="negative_weights must be None, 'popularity' or an array"):
            call(negative_weights='frequency', sampler='device')
        with pytest.raises(ValueError, match='negative_power must be finite'):
            call(negative_weights='popularity', negative_power=float('nan'), sampler='device')
        w = np.zeros(n)
        w[:3] = 1.0                                                              # three positive weights serve no list of four
        with pytest.raises(ValueError, match='negative_weights has 3 positive weights.*at least 4'):
            call(negative_weights=w, sampler='device')
        w[3] = 1e-9                                                              # four do, but the fourth is never reached
        w[0] = 1e9
        with pytest.raises(ValueError, match=r'negative_weights is too skewed for lists of 4 under the word cap.*\d+ of \d+ lists'):
            call(negative_weights=w, sampler='device')
    with pytest.raises(ValueError, match='negative_weights.*needs negatives=m'):
        model.evaluate_ranking_tuples(test, FIELDS, sampler='device', negative_weights='popularity')
    assert _steps(model) == []                                                   # the skewed draw stopped ahead of the first step
