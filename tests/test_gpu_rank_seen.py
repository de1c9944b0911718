"""GPU: ranking without seen items - HipEngine.seen_mask feeding the unchanged cffm_rank_of / cffm_topk, and exclude= / by= of
CFFM.recommend and CFFM.evaluate_ranking on the committed frappe slice with a small trained model, against a numpy replay: scores
from predict on the expanded id rows (the 'expand' route equals them bit for bit), the mask from a plain Python loop over the
excluded rows, ranks and top-k from tests/_rank_ref.py, metrics from ranking_metrics.

by = 0 is frappe's user column.  The slice is sparse there: 29 positive test rows, ONE of whose users has another positive app in
the train split, and likewise one of the 19 positive validation rows (both checked below on the CPU, from the slice alone).  The
split that is evaluated here is the TEST split, as in tests/test_gpu_rank.py: it stands in for the validation split of the usual
protocol, which the slice serves no better.  That split is the case the replay is held to; for the property
"the excluded rank is at most the plain rank, and smaller for some row" the test also excludes a split of its own making in which
every test user has seen a seeded half of the catalogue, so that the property does not hang on one row's scores."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cffm_amd import spec  # noqa: E402
from cffm_amd.spec import CFFMConfig  # noqa: E402
from oracle import rows_check as rc  # noqa: E402
from tests import _rank_ref as R  # noqa: E402
from tests.test_gpu_rank import ref_scores  # noqa: E402
from tests.test_gpu_rows import dev_of  # noqa: E402

pytestmark = pytest.mark.gpu

FIELD, USER = 1, 0


# ---- HipEngine.seen_mask -> rank_of / topk -------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [33, 4100])
def test_engine_mask_feeds_rank_of_and_topk(N):
    from cffm_amd.engine import HipEngine
    eng = HipEngine(CFFMConfig(M=50, F=4, K=8, D=8))
    C = 5
    rng = np.random.default_rng(N)
    scores = rng.choice(np.array([-1.0, -0.5, 0.0, 0.5, 1.0], dtype=np.float32), size=(C, N))       # ties everywhere
    owner = rng.integers(0, 4, size=300)
    keys, off, pos = spec.seen_index(owner, rng.integers(0, N, size=300))
    row = np.array([0, 3, -1, 1, 4], dtype=np.int32)                           # 4 = R: nothing seen, like -1
    skip = rng.random((C, N)) < 0.2
    target = np.array([0, N - 1, 5, int(pos[off[1]]), 7], dtype=np.int32)      # context 3's target is one of its own seen items
    d_scores, d_target = dev_of(scores), dev_of(target)
    for sk in (None, skip):
        want = spec.seen_mask(off, pos, row, N, sk)
        assert want[3, target[3]] == 1 and want.any(axis=1).tolist()[:2] == [True, True]
        mask = eng.seen_mask(dev_of(off), dev_of(pos), dev_of(row), N, skip=None if sk is None else dev_of(sk))
        assert mask.dtype == torch.uint8 and tuple(mask.shape) == (C, N)
        assert np.array_equal(mask.cpu().numpy(), want), 'engine mask differs from the twin'
        rc.check_exact('rank_of under the mask', eng.rank_of(d_scores, d_target, skip=mask).cpu().numpy(), R.rank_ref(scores, target, want))
        for k in (1, 10):
            idx, val, count = eng.topk(d_scores, k, skip=mask)
            ridx, rval, rcount = R.topk_ref(scores, k, want)
            rc.check_exact('topk idx', idx.cpu().numpy(), ridx)
            rc.check_exact('topk val', val.cpu().numpy().view(np.uint32), rval)
            rc.check_exact('topk count', count.cpu().numpy(), rcount)
    again = eng.seen_mask(dev_of(off), dev_of(pos), dev_of(row), N)
    assert again.data_ptr() == mask.data_ptr()                                  # one buffer per (C, N)
    assert eng.seen_mask(dev_of(off), dev_of(pos), dev_of(row[:0]), N).shape == (0, N)
    for bad in (dict(N=0), dict(skip=dev_of(skip[:, :-1]))):
        with pytest.raises(ValueError):
            eng.seen_mask(dev_of(off), dev_of(pos), dev_of(row), **dict(dict(N=N), **bad))


# ---- the class on the frappe slice ---------------------------------------------------------------------------------------------
def group_scores(eng, ctx, cand, group):
    """ref_scores of the contexts in groups of `group`, the pieces the class cuts them into under score_rows = group * N: a forward
    of another batch size may pick other kernel instances and differ in the last bit, so every cut has a replay of its own."""
    return np.concatenate([ref_scores(eng, ctx[c0:c0 + group], FIELD, cand, 8192) for c0 in range(0, len(ctx), group)])


def X(split):
    return np.asarray(split['X'], dtype=np.int32)


def loop_mask(ctx, cand, field, splits, by):
    mask = np.zeros((len(ctx), len(cand)), dtype=np.uint8)
    for split in splits:
        for x, y in zip(split['X'], np.asarray(split['Y']).reshape(-1)):
            if not y > 0:
                continue
            for c in range(len(ctx)):
                if ctx[c][by] == x[by]:
                    for n in range(len(cand)):
                        if cand[n] == x[field]:
                            mask[c, n] = 1
    return mask


@pytest.fixture(scope='module')
def frappe(tmp_path_factory):
    from cffm_amd import CFFM as M
    from cffm_amd.LoadData import LoadData
    with contextlib.redirect_stdout(io.StringIO()):
        data = LoadData(os.path.join(ROOT, 'tests', 'golden', 'frappe_slice') + '/', 'frappe', 'square_loss')
    m = M.CFFM(data.features_M, 0, str(tmp_path_factory.mktemp('seen') / 'm'), 32, 32, 'square_loss', 1, 16, 0.05, 0, [1.0, 1.0],
               'AdagradOptimizer', 0, 0, 0, 10, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'selu', batch_rng=np.random.RandomState(3))
    m.train(data)
    test = data.Test_data
    rows = X(test)[np.asarray(test['Y']).reshape(-1) > 0]
    cand = np.union1d(X(data.Train_data)[:, FIELD], X(test)[:, FIELD]).astype(np.int32)       # evaluate_ranking's default candidates
    # a split of the test's own making: every test user has seen a seeded half of the candidates
    rng = np.random.default_rng(17)
    half = {'X': [], 'Y': []}
    for u in np.unique(rows[:, USER]):
        for v in cand[rng.random(cand.size) < 0.5]:
            x = rows[0].copy()
            x[USER], x[FIELD] = u, v
            half['X'].append([int(t) for t in x])
            half['Y'].append(1.0)
    return dict(M=M, m=m, data=data, rows=rows, cand=cand, half=half, target=np.searchsorted(cand, rows[:, FIELD]),
                scores=ref_scores(m.engine, rows, FIELD, cand, 8192), scores5=group_scores(m.engine, rows, cand, 5))


def test_evaluate_ranking_exclude_equals_the_replay(frappe):
    M, m, data = frappe['M'], frappe['m'], frappe['data']
    rows, cand, scores, target = frappe['rows'], frappe['cand'], frappe['scores'], frappe['target']
    # on the CPU, from the slice alone: some positive row's user has a positive train app that is not the row's target - in the test
    # split, which is evaluated here, and in the validation split it stands in for
    for split in (data.Test_data, data.Validation_data):
        own = X(split)[np.asarray(split['Y']).reshape(-1) > 0]
        others = loop_mask(own, cand, FIELD, [data.Train_data], USER)
        others[cand[None, :] == own[:, FIELD][:, None]] = 0
        assert others.any(axis=1).sum() >= 1
    plain = R.rank_ref(scores, target)
    for name, ex in (('train', data.Train_data), ('train + test', [data.Train_data, data.Test_data]), ('half', frappe['half'])):
        mask = loop_mask(rows, cand, FIELD, ex if isinstance(ex, list) else [ex], USER)
        ranks, ranks5 = R.rank_ref(scores, target, mask), R.rank_ref(frappe['scores5'], target, mask)
        assert mask.any() and (ranks >= 0).all() and (ranks <= plain).all(), name
        for k in (10, 50):
            want, want5 = M.ranking_metrics(ranks, k), M.ranking_metrics(ranks5, k)
            got = m.evaluate_ranking(data.Test_data, FIELD, k=k, exclude=ex, by=USER)
            cut = m.evaluate_ranking(data.Test_data, FIELD, k=k, exclude=ex, by=USER, score_rows=5 * cand.size)
            print('exclude=%s k=%d: HR %.17g NDCG %.17g (replay %.17g %.17g; plain %r)'
                  % (name, k, got[0], got[1], want[0], want[1], M.ranking_metrics(plain, k)))
            assert got[0] == want[0] and got[1] == want[1], (name, k, got, want)  # the sums themselves: no tolerance
            # groups of 5 contexts, against their own replay: the hits are a count; the gains are summed group by group, at most 29
            # terms <= 1 in float64 in another order (29 * 2^-52 = 6.4e-15)
            assert cut[0] == want5[0] and abs(cut[1] - want5[1]) <= 1e-12, (name, k, cut, want5)
    # the dense split of the test's own making moves ranks for certain; the device's ranks say so themselves
    mask = loop_mask(rows, cand, FIELD, [frappe['half']], USER)
    ranks = R.rank_ref(scores, target, mask)
    assert (ranks < plain).any()
    d_scores = m.engine.score_candidates(dev_of(rows), FIELD, dev_of(cand))
    rc.check_exact('scores of the expand route', d_scores.cpu().numpy(), scores)
    got = m.engine.rank_of(d_scores, dev_of(target.astype(np.int32)), skip=dev_of(mask)).cpu().numpy()
    rc.check_exact('device ranks under the looped mask', got, ranks)


def test_the_group_mask_does_not_synchronise(frappe):
    """What the group loops of _topk_sweep and _rank_targets call per group - a slice of the row vector and one seen_mask launch - with
    every host synchronisation turned into an error; the mode is shown to bite on a torch.unique first."""
    m, data, rows, cand = frappe['m'], frappe['data'], frappe['rows'], frappe['cand']
    seen = m._seen_args('evaluate_ranking()', frappe['half'], USER, [FIELD])
    seen_of = m._seen_masks(m.engine, seen, [FIELD], dev_of(cand), dev_of(rows), cand.size)
    seen_of(0, 5), seen_of(5, len(rows))                                        # the two output buffers exist now
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            torch.unique(dev_of(cand))
        a = seen_of(0, 5).clone()
        b = seen_of(5, len(rows)).clone()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    want = loop_mask(rows, cand, FIELD, [frappe['half']], USER)
    assert np.array_equal(torch.cat([a, b]).cpu().numpy(), want)


def test_recommend_exclude_equals_the_replay(frappe):
    m, data = frappe['m'], frappe['data']
    cand = np.unique(X(data.Train_data)[:, FIELD])                              # recommend's default candidates
    ctx = X(data.Train_data)[np.asarray(data.Train_data['Y']).reshape(-1) > 0][:12]      # rows whose users have seen something
    scores = {1 << 22: ref_scores(m.engine, ctx, FIELD, cand, 8192), 5 * cand.size: group_scores(m.engine, ctx, cand, 5)}
    seen = loop_mask(ctx, cand, FIELD, [data.Train_data], USER)
    assert seen.any(axis=1).all()
    skip = np.random.default_rng(1).random(seen.shape) < 0.2
    for sk, both in ((None, seen), (skip, seen | skip)):
        for score_rows in (1 << 22, 5 * cand.size):
            ids, val = m.recommend(ctx, FIELD, k=5, skip=sk, exclude=data.Train_data, by=USER, score_rows=score_rows)
            ridx, rval, _ = R.topk_ref(scores[score_rows], 5, both)
            rc.check_exact('recommend ids', ids, cand[ridx])
            rc.check_exact('recommend scores', val.view(np.uint32), rval)
            for c in range(len(ctx)):
                assert not set(ids[c]) & set(cand[both[c] != 0])                # no seen and no skipped id comes back
    plain, _ = m.recommend(ctx, FIELD, k=5)
    print('recommend: %d of %d contexts change under exclude' % ((plain != ids).any(axis=1).sum(), len(ctx)))


def test_shared_sweep_with_exclude(frappe):
    """sweep='shared' equals 'expand' only to rounding: positions and ranks are held to the scores that route returned."""
    M, m, data = frappe['M'], frappe['m'], frappe['data']
    rows, cand, target = frappe['rows'], frappe['cand'], frappe['target']
    assert m.engine.sweep_ok()
    shared = m.engine.score_candidates_shared(dev_of(rows), FIELD, dev_of(cand)).cpu().numpy()
    for ex in (data.Train_data, frappe['half']):
        mask = loop_mask(rows, cand, FIELD, [ex], USER)
        want = M.ranking_metrics(R.rank_ref(shared, target, mask), 10)
        got = m.evaluate_ranking(data.Test_data, FIELD, k=10, sweep='shared', exclude=ex, by=USER)
        assert got[0] == want[0] and got[1] == want[1], (got, want)
        ids, val = m.recommend(rows, FIELD, candidates=cand, k=7, sweep='shared', exclude=ex, by=USER)
        ridx, rval, _ = R.topk_ref(shared, 7, mask)
        rc.check_exact('shared recommend ids', ids, cand[ridx])
        rc.check_exact('shared recommend scores', val.view(np.uint32), rval)
