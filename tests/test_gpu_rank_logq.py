"""logq=True at class level on the frappe slice (tests/golden/frappe_slice: 37 positives, 118 distinct (field 1, field 6) tuples) with
the frappe model (K = D = 32, selu).  train_ranking(sampler='device', loss='softmax', logq=True) returns, bit for bit, the losses of
a replay here that builds every epoch's lists from the numpy twins (cffm_amd.spec.draw_lists_weighted over the cdf of count ** 0.75,
cffm_amd.spec.draw_lists without weights), the table from cffm_amd.spec.logq_table, and drives the list step of a second engine of
the same seed with them; the parameters and accumulators are byte-equal afterwards, on both step routes.  The returned losses are
the means of the replay's terms.  logq=False is the call without the keyword, bit for bit."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from cffm_amd.spec import draw_lists, draw_lists_weighted, logq_table, weight_cdf
from tests.test_gpu_rank_draw import positions

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS, NEG = (1, 6), 3


@pytest.fixture(scope='module')
def frappe():
    from cffm_amd.LoadData import LoadData
    with contextlib.redirect_stdout(io.StringIO()):
        return LoadData(os.path.join(ROOT, 'tests', 'golden', 'frappe_slice') + '/', 'frappe', 'square_loss')


def model(frappe, tmp_path, name):
    from cffm_amd import CFFM as M
    return M.CFFM(frappe.features_M, 0, str(tmp_path / name), 32, 32, 'square_loss', 1, 64, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer', 0, 0,
                  0, 10, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'selu')


def same_engines(a, b):
    for x, y in ((a.export_params(), b.export_params()), (a.export_accumulators(), b.export_accumulators())):
        assert sorted(x) == sorted(y)
        for name in x:
            assert np.asarray(x[name]).tobytes() == np.asarray(y[name]).tobytes(), name


@pytest.mark.parametrize('weights', ['popularity', None])
@pytest.mark.parametrize('step,per', [('stages', 7), ('fused', 16)])
def test_training_is_the_replay_of_the_twins_lists_and_table(frappe, step, per, weights, tmp_path):
    from cffm_amd.engine import HipEngine
    data = frappe.Train_data
    X, y = np.asarray(data['X'], dtype=np.int32), np.asarray(data['Y']).reshape(-1)
    pos = X[y > 0]
    distinct, counts = np.unique(X[:, list(FIELDS)], axis=0, return_counts=True)
    P, U, seed, epochs = pos.shape[0], distinct.shape[0], 6, 2
    assert P == 37 and U == 118 and counts.max() > 1
    cdf = weight_cdf(counts.astype(np.float64) ** 0.75) if weights else None
    table = logq_table(cdf, NEG, U)
    m = model(frappe, tmp_path, 'a')
    got = m.train_ranking(data, FIELDS, negatives=NEG, loss='softmax', epochs=epochs, lists_per_step=per, seed=seed, step=step,
                          sampler='device', negative_weights=weights, logq=True)
    eng = HipEngine(m.config, seed=m.random_seed, device=str(m.engine.device))
    run = eng.train_step_lists_fused if step == 'fused' else eng.train_step_lists
    corr = torch.from_numpy(table).cuda()
    want, by_terms = [], []
    for epoch in range(epochs):
        perm = np.random.RandomState(seed + epoch).permutation(P)
        rows = pos[perm]
        at = positions(distinct, rows[:, list(FIELDS)])
        lists, place = draw_lists_weighted(seed, epoch * P, at, cdf, NEG) if weights else draw_lists(seed, epoch * P, at, U, NEG)
        assert (place >= 0).all()
        tuples = torch.from_numpy(distinct[lists].astype(np.int32)).cuda()
        idx = torch.from_numpy(lists.astype(np.int32)).cuda()
        target = torch.from_numpy(place.astype(np.int32)).cuda()
        ctx = torch.from_numpy(rows).cuda()
        total = torch.zeros(1, dtype=torch.float64, device='cuda')
        terms = []
        for r0 in range(0, P, per):
            r1 = min(P, r0 + per)
            total += run(ctx[r0:r1], list(FIELDS), tuples[r0:r1].contiguous(), target[r0:r1], 'softmax',
                         lists=idx[r0:r1], corr=corr).double() * (r1 - r0)
            terms.append(eng._ws[('list_out', r1 - r0, NEG + 1)][1].double().cpu().numpy().copy())
        want.append(float(total.cpu()[0]) / P)
        by_terms.append(float(np.concatenate(terms).sum()) / P)
    assert got == want and np.isfinite(got).all()
    # the returned loss is the mean corrected term: each step's loss is the float32 mean of its terms, within 2^-23 of it
    assert np.allclose(got, by_terms, rtol=2.0 ** -22, atol=0.0), (got, by_terms)
    same_engines(m.engine, eng)
    # the correction is felt: the uncorrected call from the same start returns another first epoch
    other = model(frappe, tmp_path, 'b').train_ranking(data, FIELDS, negatives=NEG, loss='softmax', epochs=1, lists_per_step=per, seed=seed,
                                                       step=step, sampler='device', negative_weights=weights)
    assert other[0] != got[0]


def test_logq_false_is_the_call_without_the_keyword(frappe, tmp_path):
    data = frappe.Train_data
    for i, kw in enumerate((dict(step='fused', negative_weights='popularity'), dict(step='stages'))):
        ma, mb = model(frappe, tmp_path, 'a%d' % i), model(frappe, tmp_path, 'b%d' % i)
        a = ma.train_ranking(data, FIELDS, negatives=NEG, loss='softmax', epochs=2, lists_per_step=16, seed=6, sampler='device', **kw)
        b = mb.train_ranking(data, FIELDS, negatives=NEG, loss='softmax', epochs=2, lists_per_step=16, seed=6, sampler='device',
                             logq=False, **kw)
        assert a == b and np.isfinite(a).all()
        same_engines(ma.engine, mb.engine)
