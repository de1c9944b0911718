"""hard_pool at class level on the tiny model of tests/test_gpu_rank_draw.py (F = 4, D = 8, 60 positives, 3 negatives, about 25
distinct tuples).  Training: train_ranking(sampler='device', hard_pool=8) returns, bit for bit, the losses of a replay here that draws
every epoch's pools with the numpy twin of the draw, scores each step's pools with a second engine of the same seed as its parameters
stand, picks with cffm_amd.spec.pick_hard and drives that engine's list step; the parameters and accumulators are equal afterwards.
hard_pool=None is the call without the keyword, bit for bit.  The picked lists' loss on the GPU is at least that of the pool's first
negatives.  A refused hard_pool leaves the parameters alone."""
import numpy as np
import pytest
import torch

from cffm_amd.spec import draw_lists, draw_lists_weighted, pick_hard
from tests.test_gpu_rank_draw import FIELDS, NEG, model, positions, split
from tests.test_gpu_rank_draw_weighted import counted
from tests.test_pick_hard_ref import _terms

pytestmark = pytest.mark.gpu

POOL = 8


def _bytes_equal(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        assert np.asarray(a[name]).tobytes() == np.asarray(b[name]).tobytes(), name


@pytest.mark.parametrize('kind,step,per,weights', [('bpr', 'stages', 7, None), ('softmax', 'fused', 16, None),
                                                   ('softmax', 'fused', 16, 'popularity')])
def test_training_is_the_replay_of_score_pick_step(kind, step, per, weights, tmp_path):
    from cffm_amd.engine import HipEngine
    data, X, y = split(3)
    pos = X[y > 0]
    distinct, cdf = counted(X)
    P, U, seed, epochs = pos.shape[0], distinct.shape[0], 6, 2
    assert P == 60 and NEG < POOL <= U - 1
    m = model(tmp_path, 'a')
    got = m.train_ranking(data, FIELDS, negatives=NEG, loss=kind, epochs=epochs, lists_per_step=per, seed=seed, step=step,
                          sampler='device', hard_pool=POOL, negative_weights=weights)
    eng = HipEngine(m.config, seed=m.random_seed, device=str(m.engine.device))
    run = eng.train_step_lists_fused if step == 'fused' else eng.train_step_lists
    want = []
    for epoch in range(epochs):
        perm = np.random.RandomState(seed + epoch).permutation(P)
        rows = pos[perm]
        at = positions(distinct, rows[:, list(FIELDS)])
        lists, place = draw_lists(seed, epoch * P, at, U, POOL) if weights is None else draw_lists_weighted(seed, epoch * P, at, cdf, POOL)
        assert (place >= 0).all()
        pool = distinct[lists].astype(np.int32)                                 # [P, POOL + 1, 2]
        ctx = torch.from_numpy(rows).cuda()
        total = torch.zeros(1, dtype=torch.float64, device='cuda')
        for r0 in range(0, P, per):
            r1 = min(P, r0 + per)
            scores = eng.score_candidate_tuples(ctx[r0:r1], list(FIELDS), torch.from_numpy(pool[r0:r1]).cuda()).cpu().numpy()
            sel, pl = pick_hard(seed, epoch * P + r0, scores, place[r0:r1], NEG)
            tuples = torch.from_numpy(np.take_along_axis(pool[r0:r1], sel[:, :, None], axis=1)).cuda().contiguous()
            total += run(ctx[r0:r1], list(FIELDS), tuples, torch.from_numpy(pl.astype(np.int32)).cuda(), kind).double() * (r1 - r0)
        want.append(float(total.cpu()[0]) / P)
    assert got == want and np.isfinite(got).all()
    _bytes_equal(m.engine.export_params(), eng.export_params())
    _bytes_equal(m.engine.export_accumulators(), eng.export_accumulators())
    # without the pool the drawn lists are trained on: another first epoch from the same start
    other = model(tmp_path, 'b').train_ranking(data, FIELDS, negatives=NEG, loss=kind, epochs=1, lists_per_step=per, seed=seed, step=step,
                                               sampler='device', negative_weights=weights)
    assert other[0] != got[0]


def test_no_pool_is_the_call_without_the_keyword(tmp_path):
    data, X, y = split(3)
    ma, mb = model(tmp_path, 'a'), model(tmp_path, 'b')
    a = ma.train_ranking(data, FIELDS, negatives=NEG, epochs=2, lists_per_step=16, seed=6, step='fused', sampler='device')
    b = mb.train_ranking(data, FIELDS, negatives=NEG, epochs=2, lists_per_step=16, seed=6, step='fused', sampler='device', hard_pool=None)
    assert a == b
    _bytes_equal(ma.engine.export_params(), mb.engine.export_params())
    _bytes_equal(ma.engine.export_accumulators(), mb.engine.export_accumulators())
    h = model(tmp_path, 'd').train_ranking(data, FIELDS, negatives=NEG, epochs=1, lists_per_step=16, seed=6)
    assert h == model(tmp_path, 'e').train_ranking(data, FIELDS, negatives=NEG, epochs=1, lists_per_step=16, seed=6, hard_pool=None)


@pytest.mark.parametrize('kind', ['bpr', 'softmax'])
def test_the_picked_lists_lose_at_least_what_the_pools_first_negatives_lose(kind, tmp_path):
    """On the scores of a model two epochs into training: the pick of the GPU, then (1) in float64 on the scores read back, each
    picked list's term against the term of the pool's first NEG negatives, to 1e-12 relative (both terms are monotone in every
    negative's score; the tolerance covers the order of the float64 summation); (2) cffm_list_loss itself on both sets of lists, the
    positive at the same place in both.  Its terms are float32: a term sums at most NEG + 1 values, each within a few ulp, so two
    terms whose exact values are ordered can come out reversed by a few ulp of the larger; 16 ulp of max(|term|, 1) bounds that."""
    data, X, y = split(3)
    pos = X[y > 0]
    distinct = np.unique(X[:, list(FIELDS)], axis=0)
    P, U, seed = pos.shape[0], distinct.shape[0], 6
    m = model(tmp_path, 'a')
    m.train_ranking(data, FIELDS, negatives=NEG, loss=kind, epochs=2, lists_per_step=16, seed=seed, sampler='device', hard_pool=POOL)
    eng = m.engine
    lists, place = draw_lists(seed, 7 * P, positions(distinct, pos[:, list(FIELDS)]), U, POOL)
    pool = torch.from_numpy(distinct[lists].astype(np.int32)).cuda()
    ctx = torch.from_numpy(pos).cuda()
    scores = eng.score_candidate_tuples(ctx, list(FIELDS), pool)
    index = torch.arange(POOL + 1, dtype=torch.int32, device='cuda').repeat(P, 1)
    _, sel, target = eng.pick_hard(seed, 7 * P, scores, torch.from_numpy(place.astype(np.int32)).cuda(), NEG, lists=index)
    s, sel, target = scores.cpu().numpy(), sel.cpu().numpy().astype(np.int64), target.cpu().numpy().astype(np.int64)
    assert np.array_equal(sel[np.arange(P), target], place)
    off = np.arange(NEG + 1)[None, :] != target[:, None]
    picked = sel[off].reshape(P, NEG)
    first = np.stack([np.delete(np.arange(POOL + 1), t)[:NEG] for t in place])
    k = 0 if kind == 'bpr' else 1
    hard64, drawn64 = _terms(s, place, picked)[k], _terms(s, place, first)[k]
    assert (hard64 >= drawn64 - 1e-12 * np.abs(drawn64)).all()
    assert (hard64 > drawn64).any()                                             # the pools do hold harder negatives than their first three
    other = sel.copy()
    other[off] = first.reshape(-1)                                              # the same place, the pool's first negatives around it
    gather = lambda idx: torch.from_numpy(np.take_along_axis(s, idx, axis=1)).cuda().contiguous()
    t_dev = torch.from_numpy(target.astype(np.int32)).cuda()
    loss_h, _, terms_h = eng.list_loss(gather(sel), t_dev, P, NEG + 1, kind)
    loss_h, terms_h = float(loss_h.cpu()[0]), terms_h.cpu().numpy().astype(np.float64)
    loss_d, _, terms_d = eng.list_loss(gather(other), t_dev, P, NEG + 1, kind)
    loss_d, terms_d = float(loss_d.cpu()[0]), terms_d.cpu().numpy().astype(np.float64)
    ulp = 2.0 ** -23
    assert (terms_h >= terms_d - 16 * ulp * np.maximum(np.abs(terms_d), 1.0)).all()
    assert loss_h >= loss_d - 16 * ulp * max(abs(loss_d), 1.0)


def test_a_refused_pool_leaves_the_parameters_alone(tmp_path):
    data, X, y = split(3)
    U = np.unique(X[:, list(FIELDS)], axis=0).shape[0]
    m = model(tmp_path, 'a')
    m.build_graph()
    before = (m.engine.export_params(), m.engine.export_accumulators())
    for bad in (NEG, NEG - 1, U, 1024):
        with pytest.raises(ValueError, match=r'train_ranking\(\): hard_pool must be in \(negatives, min\(U - 1, 1023\)\] = \(%d, %d\]' % (NEG, U - 1)):
            m.train_ranking(data, FIELDS, negatives=NEG, sampler='device', hard_pool=bad)
    for kw in (dict(), dict(sampler='host')):
        with pytest.raises(ValueError, match=r"train_ranking\(\): hard_pool needs sampler='device'"):
            m.train_ranking(data, FIELDS, negatives=NEG, hard_pool=POOL, **kw)
    _bytes_equal(before[0], m.engine.export_params())
    _bytes_equal(before[1], m.engine.export_accumulators())
