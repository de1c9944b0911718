"""sampler='device' at class level on a tiny model (F = 4, D = 8, 60 positives, 3 negatives).  Training: train_ranking returns, bit
for bit, the losses of a replay here that builds every epoch's lists from the numpy twin (cffm_amd.spec.draw_lists at
list0 = epoch * P) and drives the list step of a second engine of the same seed; the parameters and accumulators are equal
afterwards.  Evaluation: evaluate_ranking_tuples equals the metrics of tests/_rank_ref.py on the engine's scores of the twin's lists."""
import numpy as np
import pytest
import torch

from cffm_amd.spec import draw_lists
from tests import _rank_ref as R

pytestmark = pytest.mark.gpu

F, MF, FIELDS, NEG = 4, 200, (1, 3), 3


def split(seed, n=120):
    """n rows, every second one positive; few distinct (field 1, field 3) tuples, so that lists share candidates."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, MF, size=(n, F)).astype(np.int32)
    y = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32)
    pool = rng.integers(0, MF, size=(25, 2))
    pick = pool[rng.integers(0, 25, size=n)]
    X[:, 1], X[:, 3] = pick[:, 0], pick[:, 1]
    return {'X': X.tolist(), 'Y': y.tolist()}, X, y


def model(tmp_path, name):
    from cffm_amd import CFFM as M
    return M.CFFM(MF, 0, str(tmp_path / name), 8, 8, 'square_loss', 1, 64, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer', 0, 0, 0,
                  F, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'relu')


def positions(distinct, own):
    return np.array([int(np.nonzero((distinct == t).all(axis=1))[0][0]) for t in own])


@pytest.mark.parametrize('kind,step,per', [('bpr', 'stages', 7), ('softmax', 'fused', 16)])
def test_training_is_the_replay_of_the_twins_lists(kind, step, per, tmp_path):
    from cffm_amd.engine import HipEngine
    data, X, y = split(3)
    pos = X[y > 0]
    distinct = np.unique(X[:, list(FIELDS)], axis=0)
    P, U, seed, epochs = pos.shape[0], distinct.shape[0], 6, 2
    assert P == 60 and NEG < U
    m = model(tmp_path, 'a')
    got = m.train_ranking(data, FIELDS, negatives=NEG, loss=kind, epochs=epochs, lists_per_step=per, seed=seed, step=step,
                          sampler='device')
    eng = HipEngine(m.config, seed=m.random_seed, device=str(m.engine.device))
    run = eng.train_step_lists_fused if step == 'fused' else eng.train_step_lists
    want = []
    for epoch in range(epochs):
        perm = np.random.RandomState(seed + epoch).permutation(P)
        rows = pos[perm]
        lists, place = draw_lists(seed, epoch * P, positions(distinct, rows[:, list(FIELDS)]), U, NEG)
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
    # the host sampler draws other lists: another first epoch from the same start
    other = model(tmp_path, 'b').train_ranking(data, FIELDS, negatives=NEG, loss=kind, epochs=1, lists_per_step=per, seed=seed, step=step)
    assert other[0] != got[0]


def test_evaluation_ranks_the_twins_lists(tmp_path):
    data, X, y = split(5)
    pos = X[y > 0]
    distinct = np.unique(X[:, list(FIELDS)], axis=0)
    P, U, seed, k = pos.shape[0], distinct.shape[0], 9, 2
    m = model(tmp_path, 'e')
    got = m.evaluate_ranking_tuples(data, FIELDS, k=k, negatives=NEG, seed=seed, sampler='device')
    lists, place = draw_lists(seed, 0, positions(distinct, pos[:, list(FIELDS)]), U, NEG)
    scores = m.engine.score_candidate_tuples(torch.from_numpy(pos).cuda(), list(FIELDS),
                                             torch.from_numpy(distinct[lists].astype(np.int32)).cuda())
    ranks = R.rank_ref(scores.cpu().numpy().reshape(P, NEG + 1), place)
    assert got == pytest.approx(R.metrics_ref(ranks, k), rel=1e-12)
    assert 0 < got[0] < 1                                                       # neither every target on top nor none
    small = m.evaluate_ranking_tuples(data, FIELDS, k=k, negatives=NEG, seed=seed, sampler='device', score_rows=40)
    assert small == pytest.approx(got, rel=1e-12)                               # the same lists in groups of 10 rows
