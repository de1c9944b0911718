"""The logq keyword of CFFM.train_ranking on a recording stub engine (no GPU) whose draws are the numpy twins (cffm_amd.spec): the
table is built once per call - cffm_amd.spec.logq_table of the cdf of negative_weights, the uniform table without them - and every
step is handed the indices of its lists and that table; every new ValueError names the keyword at fault and comes before any engine
call; logq=False makes exactly the calls of the call without the keyword."""
import numpy as np
import pytest
import torch

from cffm_amd import CFFM as M
from cffm_amd.spec import draw_lists, draw_lists_weighted, logq_table, weight_cdf
from tests.test_draw_class_cpu import _at, _distinct
from tests.test_draw_weighted_class_cpu import _StubEngine as _DrawStub, _counts
from tests.test_rank_train_class_cpu import FIELDS, _positives, data  # noqa: F401


class _StubEngine(_DrawStub):
    """The draw stubs plus list steps that take the two operands of the corrected softmax and log every call in order:
    ('step', route, ctx, cand, target, kind, lists or None, corr or None, id(corr))."""

    def __init__(self, cfg, seed):
        _DrawStub.__init__(self, cfg, seed)
        self.seq = []

    def list_step_ok(self, B):
        return int(B) >= 24

    def _log(self, route, ctx, fields, cand, target, kind, extra):
        assert set(extra) <= {'lists', 'corr'}
        lists, corr = extra.get('lists'), extra.get('corr')
        if extra:
            assert lists is not None and corr is not None                        # they go together
            assert lists.dtype == torch.int32 and tuple(lists.shape) == tuple(cand.shape[:2])
            assert corr.dtype == torch.float32 and corr.dim() == 2 and corr.shape[1] == 2 and corr.is_contiguous()
        self.seq.append(('step', route, ctx.numpy().copy(), cand.numpy().copy(), target.numpy().copy(), kind,
                         None if lists is None else lists.numpy().copy(), None if corr is None else corr.numpy().copy(), id(corr),
                         sorted(extra)))
        return _DrawStub.train_step_lists(self, ctx, fields, cand, target, kind)

    def train_step_lists(self, ctx, fields, cand, target, kind, **extra):
        return self._log('stages', ctx, fields, cand, target, kind, extra)

    def train_step_lists_fused(self, ctx, fields, cand, target, kind, **extra):
        return self._log('fused', ctx, fields, cand, target, kind, extra)


@pytest.fixture
def model(tmp_path, data, monkeypatch):  # noqa: F811
    monkeypatch.setattr(M.CFFM, 'engine_factory', _StubEngine)
    monkeypatch.delenv('CFFM_TABLES', raising=False)
    m = M.CFFM(data.features_M, 0, str(tmp_path / 'm'), 8, 8, 'square_loss', 1, 16, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer', 0, 0, 0,
               10, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'relu')
    m.build_graph()
    return m


def _seq(m):
    seq = m.engine.seq[:]
    del m.engine.seq[:], m.engine.steps[:], m.engine.calls[:]
    return seq


def _check_epochs(seq, pos, distinct, drawn, table, P, per, m, seed, epochs, route_of):
    n_steps = -(-P // per)
    assert len(seq) == n_steps * epochs
    assert len({c[8] for c in seq}) == 1                                          # one table object: built once per call
    for epoch in range(epochs):
        perm = np.random.RandomState(seed + epoch).permutation(P)                # the epoch permutation stays the host's
        rows = pos[perm]
        want, place = drawn[epoch]
        for i, r0 in enumerate(range(0, P, per)):
            r1 = min(P, r0 + per)
            c = seq[epoch * n_steps + i]
            assert c[0] == 'step' and c[1] == route_of(r1 - r0) and c[5] == 'softmax' and c[9] == ['corr', 'lists']
            assert np.array_equal(c[2], rows[r0:r1]) and np.array_equal(c[4], place[r0:r1])
            assert np.array_equal(c[6], want[r0:r1]) and np.array_equal(c[3], distinct[want[r0:r1]])   # the indices of these tuples
            assert c[7].dtype == np.float32 and np.array_equal(c[7].view(np.uint32), table.view(np.uint32))


@pytest.mark.parametrize('per', [7, 1000])
def test_popularity_negatives_hand_every_step_its_indices_and_the_table(model, data, per):  # noqa: F811
    train = data.Train_data
    pos = _positives(train)
    distinct, counts = _counts(train)
    P, U, m, seed, epochs = pos.shape[0], distinct.shape[0], 3, 5, 2
    cdf = weight_cdf(counts.astype(np.float64) ** 0.75)
    means = model.train_ranking(train, FIELDS, negatives=m, loss='softmax', epochs=epochs, lists_per_step=per, seed=seed, step='auto',
                                sampler='device', negative_weights='popularity', logq=True)
    assert len(means) == epochs
    assert model.engine.draws == [] and [d[:4] for d in model.engine.wdraws] == [(seed, e * P, P, m) for e in range(epochs)]
    drawn = []
    for epoch in range(epochs):
        perm = np.random.RandomState(seed + epoch).permutation(P)
        drawn.append(draw_lists_weighted(seed, epoch * P, _at(distinct, pos[perm][:, list(FIELDS)]), cdf, m))
        assert (drawn[-1][1] >= 0).all()
    table = logq_table(cdf, m)
    assert table.shape == (U, 2)
    _check_epochs(_seq(model), pos, distinct, drawn, table, P, min(per, P), m, seed, epochs,
                  lambda g: 'fused' if g * (m + 1) >= 24 else 'stages')


def test_uniform_negatives_take_the_uniform_table(model, data):  # noqa: F811
    train = data.Train_data
    pos, distinct = _positives(train), _distinct(train)
    P, U, m, seed = pos.shape[0], distinct.shape[0], 4, 9
    model.train_ranking(train, FIELDS, negatives=m, loss='softmax', epochs=1, lists_per_step=10, seed=seed, sampler='device', logq=True)
    assert model.engine.draws == [(seed, 0, P, U, m)] and model.engine.wdraws == []
    perm = np.random.RandomState(seed).permutation(P)
    drawn = [draw_lists(seed, 0, _at(distinct, pos[perm][:, list(FIELDS)]), U, m)]
    table = logq_table(None, m, U)
    assert np.array_equal(table[:, 0], np.full(U, np.log(m / U), dtype=np.float32))
    _check_epochs(_seq(model), pos, distinct, drawn, table, P, 10, m, seed, 1, lambda g: 'stages')
    # an array of weights: its own cdf
    w = 1.0 + np.arange(U) % 3
    model.train_ranking(train, FIELDS, negatives=m, loss='softmax', epochs=1, lists_per_step=1000, seed=seed, sampler='device',
                        negative_weights=w, logq=True)
    (c,) = _seq(model)
    assert np.array_equal(c[7].view(np.uint32), logq_table(weight_cdf(w), m).view(np.uint32))


def test_refusals_come_before_any_engine_call(model, data):  # noqa: F811
    train = data.Train_data
    for kw in (dict(), dict(sampler='host')):                                    # only 'device' hands on indices and a proposal
        with pytest.raises(ValueError, match=r"logq=True needs sampler='device'.*sampler='host'"):
            model.train_ranking(train, FIELDS, negatives=3, loss='softmax', logq=True, **kw)
    for kw in (dict(), dict(loss='bpr')):                                        # bpr is the default loss
        with pytest.raises(ValueError, match=r"logq=True.*needs loss='softmax', not loss='bpr'"):
            model.train_ranking(train, FIELDS, negatives=3, sampler='device', logq=True, **kw)
    with pytest.raises(ValueError, match=r'logq=True needs hard_pool=None.*hard_pool=8'):
        model.train_ranking(train, FIELDS, negatives=3, loss='softmax', sampler='device', hard_pool=8, logq=True)
    # what was refused by name without the keyword is refused by the same name with it
    with pytest.raises(ValueError, match='sampler must be'):
        model.train_ranking(train, FIELDS, negatives=3, loss='softmax', sampler='gpu', logq=True)
    with pytest.raises(ValueError, match='loss must be one of'):
        model.train_ranking(train, FIELDS, negatives=3, loss='hinge', sampler='device', logq=True)
    model.world = 2
    with pytest.raises(ValueError, match='process group of 2 ranks'):
        model.train_ranking(train, FIELDS, negatives=3, loss='softmax', sampler='device', logq=True)
    model.world = 1
    model.optimizer_type = 'AdamOptimizer'
    with pytest.raises(ValueError, match='AdamOptimizer'):
        model.train_ranking(train, FIELDS, negatives=3, loss='softmax', sampler='device', logq=True)
    model.optimizer_type = 'AdagradOptimizer'
    with pytest.raises(TypeError, match='logq'):                                 # evaluation keeps its signature: raw scores
        model.evaluate_ranking_tuples(data.Test_data, FIELDS, negatives=3, sampler='device', logq=True)
    assert model.engine.seq == [] and model.engine.draws == [] and model.engine.wdraws == [] and model.engine.calls == []


def test_logq_false_is_the_call_without_the_keyword(model, data):  # noqa: F811
    train = data.Train_data
    runs = []
    for sampler, extra in (('device', dict()), ('device', dict(negative_weights='popularity')), ('host', dict())):
        pair = []
        for kw in (dict(), dict(logq=False)):
            del model.engine.draws[:], model.engine.wdraws[:]
            model.train_ranking(train, FIELDS, negatives=3, loss='softmax', epochs=2, lists_per_step=9, seed=4, step='auto',
                                sampler=sampler, **dict(extra, **kw))
            calls = model.engine.calls[:]
            pair.append((_seq(model), model.engine.draws[:], [d[:4] for d in model.engine.wdraws], len(calls)))
        a, b = pair
        assert a[1:] == b[1:] and len(a[0]) == len(b[0]) > 0
        for x, y in zip(a[0], b[0]):
            assert x[9] == y[9] == [] and x[6] is None and x[7] is None          # neither operand is passed, not even as None
            assert x[1] == y[1] and x[5] == y[5] and all(np.array_equal(u, v) for u, v in zip(x[2:5], y[2:5]))
        runs.append(a)
    assert runs[0][1] and not runs[0][2] and runs[1][2] and not runs[1][1] and not runs[2][1]
