"""negative_weights at class level on a tiny model (F = 4, D = 8, 60 positives, 3 negatives).  Training: train_ranking(sampler='device',
negative_weights='popularity') returns, bit for bit, the losses of a replay here that builds every epoch's lists from the numpy twin
(cffm_amd.spec.draw_lists_weighted at list0 = epoch * P over the cdf of count ** 0.75) and drives the list step of a second engine
of the same seed; the parameters and accumulators are equal afterwards.  Evaluation: evaluate_ranking_tuples equals the metrics of
tests/_rank_ref.py on the engine's scores of the twin's lists.  negative_weights=None is the call without the keyword, bit for bit.
Weights too skewed for the word cap raise."""
import numpy as np
import pytest
import torch

from cffm_amd.spec import draw_lists_weighted, weight_cdf
from tests import _rank_ref as R
from tests.test_gpu_rank_draw import FIELDS, NEG, model, positions, split

pytestmark = pytest.mark.gpu


def counted(X):
    """(distinct tuples at FIELDS, the cdf of count ** 0.75) over all rows, any label."""
    distinct, counts = np.unique(X[:, list(FIELDS)], axis=0, return_counts=True)
    assert counts.max() > 1
    return distinct, weight_cdf(counts.astype(np.float64) ** 0.75)


@pytest.mark.parametrize('kind,step,per', [('bpr', 'stages', 7), ('softmax', 'fused', 16)])
def test_training_is_the_replay_of_the_twins_lists(kind, step, per, tmp_path):
    from cffm_amd.engine import HipEngine
    data, X, y = split(3)
    pos = X[y > 0]
    distinct, cdf = counted(X)
    P, U, seed, epochs = pos.shape[0], distinct.shape[0], 6, 2
    assert P == 60 and NEG < U
    m = model(tmp_path, 'a')
    got = m.train_ranking(data, FIELDS, negatives=NEG, loss=kind, epochs=epochs, lists_per_step=per, seed=seed, step=step,
                          sampler='device', negative_weights='popularity')
    eng = HipEngine(m.config, seed=m.random_seed, device=str(m.engine.device))
    run = eng.train_step_lists_fused if step == 'fused' else eng.train_step_lists
    want = []
    for epoch in range(epochs):
        perm = np.random.RandomState(seed + epoch).permutation(P)
        rows = pos[perm]
        lists, place = draw_lists_weighted(seed, epoch * P, positions(distinct, rows[:, list(FIELDS)]), cdf, NEG)
        assert (place >= 0).all()
        tuples = torch.from_numpy(distinct[lists].astype(np.int32)).cuda()
        target = torch.from_numpy(place.astype(np.int32)).cuda()
        ctx = torch.from_numpy(rows).cuda()
        total = torch.zeros(1, dtype=torch.float64, device='cuda')
        for r0 in range(0, P, per):
            r1 = min(P, r0 + per)
            total += run(ctx[r0:r1], list(FIELDS), tuples[r0:r1].contiguous(), target[r0:r1], kind).double() * (r1 - r0)
        want.append(float(total.cpu()[0]) / P)
    assert got == want and np.isfinite(got).all()
    for a, b in ((m.engine.export_params(), eng.export_params()), (m.engine.export_accumulators(), eng.export_accumulators())):
        assert sorted(a) == sorted(b)
        for name in a:
            assert np.asarray(a[name]).tobytes() == np.asarray(b[name]).tobytes(), name
    # the uniform device sampler draws other lists: another first epoch from the same start
    other = model(tmp_path, 'b').train_ranking(data, FIELDS, negatives=NEG, loss=kind, epochs=1, lists_per_step=per, seed=seed, step=step,
                                               sampler='device')
    assert other[0] != got[0]


def test_evaluation_ranks_the_twins_lists(tmp_path):
    data, X, y = split(5)
    pos = X[y > 0]
    distinct, cdf = counted(X)
    P, seed, k = pos.shape[0], 9, 2
    m = model(tmp_path, 'e')
    got = m.evaluate_ranking_tuples(data, FIELDS, k=k, negatives=NEG, seed=seed, sampler='device', negative_weights='popularity')
    lists, place = draw_lists_weighted(seed, 0, positions(distinct, pos[:, list(FIELDS)]), cdf, NEG)
    assert (place >= 0).all()
    scores = m.engine.score_candidate_tuples(torch.from_numpy(pos).cuda(), list(FIELDS),
                                             torch.from_numpy(distinct[lists].astype(np.int32)).cuda())
    ranks = R.rank_ref(scores.cpu().numpy().reshape(P, NEG + 1), place)
    assert got == pytest.approx(R.metrics_ref(ranks, k), rel=1e-12)
    assert 0 < got[0] < 1                                                       # neither every target on top nor none
    small = m.evaluate_ranking_tuples(data, FIELDS, k=k, negatives=NEG, seed=seed, sampler='device', negative_weights='popularity',
                                      score_rows=40)
    assert small == pytest.approx(got, rel=1e-12)                               # the same lists in groups of 10 rows
    power1 = m.evaluate_ranking_tuples(data, FIELDS, k=k, negatives=NEG, seed=seed, sampler='device', negative_weights='popularity',
                                       negative_power=1.0)
    counts = np.unique(X[:, list(FIELDS)], axis=0, return_counts=True)[1].astype(np.float64)
    byarray = m.evaluate_ranking_tuples(data, FIELDS, k=k, negatives=NEG, seed=seed, sampler='device', negative_weights=counts)
    assert power1 == byarray


def test_no_weights_is_the_call_without_the_keyword(tmp_path):
    data, X, y = split(3)
    a = model(tmp_path, 'a').train_ranking(data, FIELDS, negatives=NEG, epochs=2, lists_per_step=16, seed=6, step='fused', sampler='device')
    mb = model(tmp_path, 'b')
    b = mb.train_ranking(data, FIELDS, negatives=NEG, epochs=2, lists_per_step=16, seed=6, step='fused', sampler='device',
                         negative_weights=None)
    assert a == b
    ma = model(tmp_path, 'c')
    ea = ma.evaluate_ranking_tuples(data, FIELDS, k=2, negatives=NEG, seed=9, sampler='device')
    assert ea == ma.evaluate_ranking_tuples(data, FIELDS, k=2, negatives=NEG, seed=9, sampler='device', negative_weights=None)
    h = model(tmp_path, 'd').train_ranking(data, FIELDS, negatives=NEG, epochs=1, lists_per_step=16, seed=6)
    assert h == model(tmp_path, 'e').train_ranking(data, FIELDS, negatives=NEG, epochs=1, lists_per_step=16, seed=6, negative_weights=None)


def test_weights_too_skewed_for_the_cap_raise(tmp_path):
    data, X, y = split(3)
    U = np.unique(X[:, list(FIELDS)], axis=0).shape[0]
    w = np.full(U, 1e-9)
    w[0] = 1e9
    m = model(tmp_path, 'a')
    m.build_graph()
    before = m.engine.export_params()
    with pytest.raises(ValueError, match=r'train_ranking\(\): negative_weights is too skewed for lists of 4 under the word cap.*\d+ of 60 lists'):
        m.train_ranking(data, FIELDS, negatives=NEG, sampler='device', negative_weights=w)
    after = m.engine.export_params()
    assert all(np.asarray(before[n]).tobytes() == np.asarray(after[n]).tobytes() for n in before)       # no step was taken
    with pytest.raises(ValueError, match=r'evaluate_ranking_tuples\(\): negative_weights is too skewed'):
        m.evaluate_ranking_tuples(data, FIELDS, negatives=NEG, sampler='device', negative_weights=w)
