"""The hard_pool keyword of CFFM.train_ranking on a recording stub engine (no GPU) whose draws and whose pick_hard are the numpy twins
(cffm_amd.spec): per step the class scores the step's pool lists, picks, and steps on what the pick returned; the pool is the device
draw at m = hard_pool under the list ids epoch * P + j; pick_hard is handed the id of the step's first list under every
lists_per_step; every new ValueError names the keyword and comes before any engine call; hard_pool=None makes exactly the calls of
the call without the keyword."""
import numpy as np
import pytest
import torch

from cffm_amd import CFFM as M
from cffm_amd.spec import draw_lists, draw_lists_weighted, pick_hard, weight_cdf
from tests import _cand_ref as CR
from tests.test_draw_class_cpu import _at, _distinct
from tests.test_draw_weighted_class_cpu import _StubEngine as _DrawStub, _counts
from tests.test_rank_class_cpu import _score
from tests.test_rank_train_class_cpu import FIELDS, _positives, data  # noqa: F401


class _StubEngine(_DrawStub):
    """The draw stubs plus a pick_hard that is the twin, a fused list step that is the stage stub's, and one log of every engine
    call in order: ('score', ctx, pool tuples), ('pick', seed, list0, scores, target_pool, m, pool tuples), ('step', ...)."""

    def __init__(self, cfg, seed):
        _DrawStub.__init__(self, cfg, seed)
        self.seq = []

    def list_step_ok(self, B):
        return int(B) >= 24

    def score_candidate_tuples(self, ctx, fields, cand, block=8192):
        assert cand.dim() == 3 and cand.shape[0] == ctx.shape[0] and list(fields) == list(FIELDS)
        assert ctx.shape[0] * cand.shape[1] <= block                             # one piece: an expand and a predict launch
        self.seq.append(('score', ctx.numpy().copy(), cand.numpy().copy()))
        return _DrawStub.score_candidate_tuples(self, ctx, fields, cand, block)

    def pick_hard(self, seed, list0, scores, target_pool, m, lists=None, tuples=None):
        assert lists is None and tuples is not None and tuples.dtype == torch.int32 and target_pool.dtype == torch.int32
        assert scores.dtype == torch.float32 and scores.shape == tuples.shape[:2]
        self.seq.append(('pick', int(seed), int(list0), scores.numpy().copy(), target_pool.numpy().copy(), int(m), tuples.numpy().copy()))
        sel, place = pick_hard(seed, list0, scores.numpy(), target_pool.numpy(), m)
        assert (place >= 0).all()
        out = torch.gather(tuples, 1, torch.from_numpy(sel)[:, :, None].expand(-1, -1, tuples.shape[2])).contiguous()
        return out, None, torch.from_numpy(place.astype(np.int32))

    def train_step_lists(self, ctx, fields, cand, target, kind):
        self.seq.append(('step', 'stages', ctx.numpy().copy(), cand.numpy().copy(), target.numpy().copy(), kind))
        return _DrawStub.train_step_lists(self, ctx, fields, cand, target, kind)

    def train_step_lists_fused(self, ctx, fields, cand, target, kind):
        self.seq.append(('step', 'fused', ctx.numpy().copy(), cand.numpy().copy(), target.numpy().copy(), kind))
        return _DrawStub.train_step_lists(self, ctx, fields, cand, target, kind)


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


def _check_epochs(seq, pos, distinct, pools, P, per, m, p, seed, epochs, kind, step_kinds):
    """seq is, per step, (score, pick, step) on the rows r0:r1 of the epoch's pool; pools[epoch] = (pool lists, pool target)."""
    n_steps = -(-P // per)
    assert len(seq) == 3 * n_steps * epochs and [c[0] for c in seq] == ['score', 'pick', 'step'] * (n_steps * epochs)
    for epoch in range(epochs):
        perm = np.random.RandomState(seed + epoch).permutation(P)                # the epoch permutation stays the host's
        rows = pos[perm]
        want, place = pools[epoch]
        for i, r0 in enumerate(range(0, P, per)):
            r1 = min(P, r0 + per)
            score, pick, step = seq[3 * (epoch * n_steps + i):3 * (epoch * n_steps + i) + 3]
            pool = distinct[want[r0:r1]]
            assert np.array_equal(score[1], rows[r0:r1]) and np.array_equal(score[2], pool)
            scores = _score(CR.expand_tuples(rows[r0:r1], list(FIELDS), pool)).reshape(r1 - r0, p + 1).astype(np.float32)
            assert pick[1:3] == (seed, epoch * P + r0) and pick[5] == m          # the id of the step's first list
            assert np.array_equal(pick[3].view(np.uint32), scores.view(np.uint32)) and np.array_equal(pick[4], place[r0:r1])
            assert np.array_equal(pick[6], pool)
            sel, pl = pick_hard(seed, epoch * P + r0, scores, place[r0:r1], m)
            assert step[1] == step_kinds(r1 - r0) and step[5] == kind
            assert np.array_equal(step[2], rows[r0:r1]) and np.array_equal(step[4], pl)
            assert np.array_equal(step[3], np.take_along_axis(pool, sel[:, :, None], axis=1))
            assert np.array_equal(step[3][np.arange(r1 - r0), pl], rows[r0:r1][:, list(FIELDS)])      # the positive at its place


@pytest.mark.parametrize('per', [7, 1000])
def test_score_pick_step_on_the_uniform_pool(model, data, per):  # noqa: F811
    train = data.Train_data
    pos, distinct = _positives(train), _distinct(train)
    P, U, m, p, seed, epochs = pos.shape[0], distinct.shape[0], 3, 8, 5, 2
    assert P * (p + 1) <= 8192
    model.train_ranking(train, FIELDS, negatives=m, loss='softmax', epochs=epochs, lists_per_step=per, seed=seed, step='auto',
                        sampler='device', hard_pool=p)
    assert model.engine.draws == [(seed, e * P, P, U, p) for e in range(epochs)] and model.engine.wdraws == []   # pools of p + 1
    pools = []
    for epoch in range(epochs):
        perm = np.random.RandomState(seed + epoch).permutation(P)
        pools.append(draw_lists(seed, epoch * P, _at(distinct, pos[perm][:, list(FIELDS)]), U, p))
    # chosen as today, on (r1 - r0) * (m + 1) rows: the stub serves the fused step from 24 rows
    _check_epochs(_seq(model), pos, distinct, pools, P, min(per, P), m, p, seed, epochs, 'softmax',
                  lambda g: 'fused' if g * (m + 1) >= 24 else 'stages')


def test_the_pool_is_the_weighted_draw_under_negative_weights(model, data):  # noqa: F811
    train = data.Train_data
    pos = _positives(train)
    distinct, counts = _counts(train)
    P, U, m, p, seed = pos.shape[0], distinct.shape[0], 2, 6, 9
    cdf = weight_cdf(counts.astype(np.float64) ** 0.75)
    model.train_ranking(train, FIELDS, negatives=m, epochs=1, lists_per_step=10, seed=seed, sampler='device', hard_pool=p,
                        negative_weights='popularity')
    assert model.engine.draws == [] and [d[:4] for d in model.engine.wdraws] == [(seed, 0, P, p)]
    perm = np.random.RandomState(seed).permutation(P)
    pool = draw_lists_weighted(seed, 0, _at(distinct, pos[perm][:, list(FIELDS)]), cdf, p)
    assert (pool[1] >= 0).all()
    _check_epochs(_seq(model), pos, distinct, [pool], P, 10, m, p, seed, 1, 'bpr', lambda g: 'stages')
    # the checks of the weighted draw speak of the pool's lists of p + 1
    w = np.zeros(U)
    w[:p] = 1.0
    with pytest.raises(ValueError, match='negative_weights has %d positive weights.*at least %d' % (p, p + 1)):
        model.train_ranking(train, FIELDS, negatives=m, sampler='device', hard_pool=p, negative_weights=w)
    w[p] = 1e-9
    w[0] = 1e9
    with pytest.raises(ValueError, match=r'negative_weights is too skewed for lists of %d under the word cap' % (p + 1)):
        model.train_ranking(train, FIELDS, negatives=m, sampler='device', hard_pool=p, negative_weights=w)
    assert [c for c in _seq(model) if c[0] != 'draw'] == []


def test_refusals_come_before_any_engine_call(model, data):  # noqa: F811
    train = data.Train_data
    U = _distinct(train).shape[0]
    assert U - 1 < 1023
    for kw in (dict(), dict(sampler='host')):                                    # only 'device' draws the pool
        with pytest.raises(ValueError, match=r"hard_pool needs sampler='device'.*sampler='host'"):
            model.train_ranking(train, FIELDS, negatives=3, hard_pool=8, **kw)
    for bad in (3, 2, 0, -1, U, U + 5, 1024):                                    # negatives < p <= min(U - 1, 1023)
        with pytest.raises(ValueError, match=r'hard_pool must be in \(negatives, min\(U - 1, 1023\)\] = \(3, %d\]' % (U - 1)):
            model.train_ranking(train, FIELDS, negatives=3, sampler='device', hard_pool=bad)
    # what was refused by name without the keyword is refused by the same name with it
    with pytest.raises(ValueError, match='sampler must be'):
        model.train_ranking(train, FIELDS, negatives=3, sampler='gpu', hard_pool=8)
    model.world = 2
    with pytest.raises(ValueError, match='process group of 2 ranks'):
        model.train_ranking(train, FIELDS, negatives=3, sampler='device', hard_pool=8)
    model.world = 1
    model.optimizer_type = 'AdamOptimizer'
    with pytest.raises(ValueError, match='AdamOptimizer'):
        model.train_ranking(train, FIELDS, negatives=3, sampler='device', hard_pool=8)
    model.optimizer_type = 'AdagradOptimizer'
    with pytest.raises(TypeError, match='hard_pool'):                            # evaluation keeps its signature
        model.evaluate_ranking_tuples(data.Test_data, FIELDS, negatives=3, sampler='device', hard_pool=8)
    assert model.engine.seq == [] and model.engine.draws == [] and model.engine.wdraws == [] and model.engine.calls == []
    model.train_ranking(train, FIELDS, negatives=3, sampler='device', hard_pool=U - 1, epochs=1)       # the largest pool is served
    assert model.engine.draws[0][3:] == (U, U - 1)


def test_no_pool_is_the_call_without_the_keyword(model, data):  # noqa: F811
    train = data.Train_data
    runs = []
    for sampler, extra in (('device', dict()), ('device', dict(negative_weights='popularity')), ('host', dict())):
        pair = []
        for kw in (dict(), dict(hard_pool=None)):
            del model.engine.draws[:], model.engine.wdraws[:]
            model.train_ranking(train, FIELDS, negatives=3, epochs=2, lists_per_step=9, seed=4, step='auto', sampler=sampler,
                                **dict(extra, **kw))
            pair.append((_seq(model), model.engine.draws[:], [d[:4] for d in model.engine.wdraws]))
        a, b = pair
        assert a[1:] == b[1:] and len(a[0]) == len(b[0]) > 0
        assert all(c[0] == 'step' for c in a[0])                                  # no score, no pick
        for x, y in zip(a[0], b[0]):
            assert x[1] == y[1] and x[5] == y[5] and all(np.array_equal(u, v) for u, v in zip(x[2:5], y[2:5]))
        runs.append(a)
    assert runs[0][1] and not runs[0][2] and runs[1][2] and not runs[1][1] and not runs[2][1]
