"""exclude= / by= of CFFM.recommend, recommend_tuples, evaluate_ranking and evaluate_ranking_tuples on a stub engine (no GPU), on the
committed frappe slice: the seen relation the class builds with torch and hands to HipEngine.seen_mask - here cffm_amd.spec.seen_mask,
the numpy twin - against a mask built by a plain Python loop over the excluded rows, the ranks and the top-k of tests/_rank_ref.py
under that mask, what is refused before any engine call, and that without the keywords every engine call is the one made before
they existed.  The score is the plain function of the ids of tests/test_rank_class_cpu.py (many ties)."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from cffm_amd import CFFM as M
from cffm_amd import spec
from cffm_amd.LoadData import LoadData
from tests import _cand_ref as CR
from tests import _rank_ref as R
from tests.test_rank_class_cpu import _score

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'golden', 'frappe_slice') + '/'
FIELD, FIELDS, USER = 1, (1, 6), 0


class _StubEngine(object):
    device = torch.device('cpu')
    opt_step = 0

    def __init__(self, cfg, seed):
        self.cfg, self.calls = cfg, []

    def score_candidates(self, ctx, field, cand, block=8192):
        self.calls.append(('score', int(ctx.shape[0])))
        return torch.from_numpy(_score(R.expand_ref(ctx.numpy(), field, cand.numpy(), 0, ctx.shape[0] * cand.numel())).reshape(ctx.shape[0], -1))

    def score_candidate_tuples(self, ctx, fields, cand, block=8192):
        self.calls.append(('score', int(ctx.shape[0])))
        return torch.from_numpy(_score(CR.expand_tuples(ctx.numpy(), list(fields), cand.numpy())).reshape(ctx.shape[0], cand.shape[-2]))

    def seen_mask(self, off, pos, row, N, skip=None):
        assert off.dtype == pos.dtype == row.dtype == torch.int32 and (skip is None or skip.dtype == torch.uint8)
        self.calls.append(('seen_mask', int(row.numel()), skip is not None))
        return torch.from_numpy(spec.seen_mask(off.numpy(), pos.numpy(), row.numpy(), N, None if skip is None else skip.numpy()))

    def topk(self, scores, k, **kw):
        self.calls.append(('topk', sorted(kw), kw.get('skip') is not None))
        skip = kw.get('skip')
        idx, val, count = R.topk_ref(scores.numpy(), k, None if skip is None else skip.numpy())
        return torch.from_numpy(idx), torch.from_numpy(val.view(np.float32)), torch.from_numpy(count)

    def rank_of(self, scores, target, **kw):
        self.calls.append(('rank_of', sorted(kw)))
        skip = kw.get('skip')
        return torch.from_numpy(R.rank_ref(scores.numpy(), target.numpy(), None if skip is None else skip.numpy()))


@pytest.fixture(scope='module')
def data():
    with contextlib.redirect_stdout(io.StringIO()):
        return LoadData(PATH, 'frappe', 'square_loss')


@pytest.fixture
def model(tmp_path, data, monkeypatch):
    monkeypatch.setattr(M.CFFM, 'engine_factory', _StubEngine)
    monkeypatch.delenv('CFFM_TABLES', raising=False)
    m = M.CFFM(data.features_M, 0, str(tmp_path / 'm'), 8, 8, 'square_loss', 1, 16, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer', 0, 0, 0,
               10, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'relu')
    m.build_graph()
    m._train_split = data.Train_data
    return m


def _calls(m):
    calls = list(m.engine.calls)
    del m.engine.calls[:]
    return calls


def X(split):
    return np.asarray(split['X'], dtype=np.int32)


def loop_mask(ctx, cand, cols, splits, by):
    """The seen mask as the docstrings state it, by a plain loop: cand [N] ids or [N, nf] tuples."""
    cand = np.asarray(cand).reshape(len(cand), -1)
    mask = np.zeros((len(ctx), len(cand)), dtype=np.uint8)
    for split in splits:
        for x, y in zip(split['X'], np.asarray(split['Y']).reshape(-1)):
            if not y > 0:
                continue
            for c in range(len(ctx)):
                if ctx[c][by] != x[by]:
                    continue
                for n in range(len(cand)):
                    if all(cand[n][a] == x[f] for a, f in enumerate(cols)):
                        mask[c, n] = 1
    return mask


def positives(split):
    return X(split)[np.asarray(split['Y']).reshape(-1) > 0]


# by = 0 is the user column of frappe; the slice is sparse there (one positive test row whose user has another positive train app),
# so the same checks also run with denser relations: the city column as the owner, and the evaluated split itself excluded too -
# then every target is in its own owner's seen set and must still be ranked
EXCLUDES = [(('Train_data',), USER), (('Train_data',), 9), (('Train_data', 'Test_data'), USER), (('Train_data', 'Validation_data', 'Test_data'), 8)]


@pytest.mark.parametrize('names,by', EXCLUDES)
def test_evaluate_ranking_equals_the_ranks_under_the_looped_mask(model, data, names, by):
    splits = [getattr(data, n) for n in names]
    test = data.Test_data
    ctx = positives(test)
    cand = np.union1d(X(data.Train_data)[:, FIELD], X(test)[:, FIELD]).astype(np.int32)
    mask = loop_mask(ctx, cand, [FIELD], splits, by)
    assert mask.any() and not mask.all()
    scores = _score(R.expand_ref(ctx, FIELD, cand, 0, ctx.shape[0] * cand.size)).reshape(ctx.shape[0], cand.size)
    target = np.searchsorted(cand, ctx[:, FIELD])
    if 'Test_data' in names:
        assert mask[np.arange(len(ctx)), target].all()                            # every target is seen, and is ranked all the same
    ranks, plain = R.rank_ref(scores, target, mask), R.rank_ref(scores, target)
    assert (ranks >= 0).all() and (ranks <= plain).all() and (ranks < plain).any()
    got = model.evaluate_ranking(test, FIELD, k=10, exclude=splits[0] if len(splits) == 1 else splits, by=by)
    assert got == pytest.approx(M.ranking_metrics(ranks, 10), abs=1e-12)
    calls = _calls(model)
    assert calls == [('score', len(ctx)), ('seen_mask', len(ctx), False), ('rank_of', ['skip'])]
    assert model.evaluate_ranking(test, FIELD, k=10) == pytest.approx(M.ranking_metrics(plain, 10), abs=1e-12)


@pytest.mark.parametrize('names,by', EXCLUDES[:3])
def test_evaluate_ranking_tuples_equals_the_ranks_under_the_looped_mask(model, data, names, by):
    splits = [getattr(data, n) for n in names]
    test = data.Test_data
    ctx = positives(test)
    cols = list(FIELDS)
    cand = np.unique(np.concatenate([X(data.Train_data)[:, cols], X(test)[:, cols]]), axis=0)
    mask = loop_mask(ctx, cand, cols, splits, by)
    assert mask.any()
    scores = _score(CR.expand_tuples(ctx, cols, cand)).reshape(ctx.shape[0], -1)
    target = np.array([int(np.nonzero((cand == t).all(axis=1))[0][0]) for t in ctx[:, cols]])
    ranks = R.rank_ref(scores, target, mask)
    got = model.evaluate_ranking_tuples(test, FIELDS, k=10, exclude=splits, by=by, score_rows=7 * len(cand))
    assert got == pytest.approx(M.ranking_metrics(ranks, 10), abs=1e-12)
    groups = -(-len(ctx) // 7)
    assert [c[0] for c in _calls(model)] == ['score', 'seen_mask', 'rank_of'] * groups


def test_recommend_leaves_out_seen_and_skipped(model, data):
    by, k = 9, 6
    ctx = X(data.Test_data)[:9]
    cand = np.unique(X(data.Train_data)[:, FIELD]).astype(np.int32)               # the default candidates
    N = cand.size
    seen = loop_mask(ctx, cand, [FIELD], [data.Train_data], by)
    assert seen.any(axis=1).sum() >= 5 and not seen.all()
    skip = np.random.default_rng(2).random((9, N)) < 0.3
    skip[4] = True                                                               # nothing left for context 4
    scores = _score(R.expand_ref(ctx, FIELD, cand, 0, 9 * N)).reshape(9, N)
    for sk, both in ((None, seen), (skip, seen | skip)):
        ids, val = model.recommend(ctx, FIELD, k=k, skip=sk, exclude=data.Train_data, by=by)
        idx, bits_, count = R.topk_ref(scores, k, both)
        assert np.array_equal(ids, np.where(idx >= 0, cand[np.maximum(idx, 0)], -1)) and np.array_equal(val.view(np.uint32), bits_)
        for c in range(9):
            assert not set(ids[c][ids[c] >= 0]) & set(cand[both[c] != 0])         # no seen and no skipped id comes back
        assert _calls(model) == [('score', 9), ('seen_mask', 9, sk is not None), ('topk', ['skip'], True)]
    assert (ids[4] == -1).all() and np.isnan(val[4]).all()
    # the plain call differs: the seen ids did matter
    plain, _ = model.recommend(ctx, FIELD, k=k)
    assert any(set(plain[c]) & set(cand[seen[c] != 0]) for c in range(9))
    # tuples: positions come back, under the same rule
    cols = list(FIELDS)
    tup = np.unique(X(data.Train_data)[:, cols], axis=0)
    seen2 = loop_mask(ctx, tup, cols, [data.Train_data], by)
    pos, val = model.recommend_tuples(ctx, FIELDS, tup, k=k, exclude=[data.Train_data], by=by, score_rows=4 * len(tup))
    idx, bits_, _ = R.topk_ref(_score(CR.expand_tuples(ctx, cols, tup)).reshape(9, -1), k, seen2)
    assert seen2.any() and np.array_equal(pos, idx) and np.array_equal(val.view(np.uint32), bits_)


def _everything(ctx, cand, by):
    """A split in which the owner of every context row has every candidate id at FIELD, with label 1."""
    rows = []
    for u in sorted(set(int(r[by]) for r in ctx)):
        for v in cand:
            row = [int(t) for t in ctx[0]]
            row[by], row[FIELD] = u, int(v)
            rows.append(row)
    return {'X': rows, 'Y': [1.0] * len(rows)}


def test_with_every_candidate_seen_only_the_target_is_left(model, data):
    test = data.Test_data
    ctx = positives(test)
    cand = np.union1d(X(data.Train_data)[:, FIELD], X(test)[:, FIELD]).astype(np.int32)
    everything = _everything(ctx, cand, USER)
    hr, ndcg = model.evaluate_ranking(test, FIELD, k=1, exclude=everything, by=USER)
    assert hr == 1.0 and ndcg == 1.0
    ids, val = model.recommend(ctx[:4], FIELD, candidates=cand, k=3, exclude=everything, by=USER)
    assert (ids == -1).all() and np.isnan(val).all()
    # an owner the relation does not know keeps every candidate
    stranger = ctx[:2].copy()
    stranger[:, USER] = 0 if 0 not in set(ctx[:, USER]) else int(ctx[:, USER].max()) + 1
    ids, _ = model.recommend(stranger, FIELD, candidates=cand, k=3, exclude=everything, by=USER)
    assert (ids >= 0).all()
    # a relation without a positive row, and one none of whose items is a candidate: nothing is seen
    nothing = {'X': everything['X'][:5], 'Y': [-1.0] * 5}
    other = {'X': [[int(t) for t in ctx[0]]], 'Y': [1.0]}
    other['X'][0][FIELD] = int(cand.max()) + 1
    plain = model.recommend(ctx[:4], FIELD, candidates=cand, k=3)
    for ex in (nothing, other, [nothing, other]):
        got = model.recommend(ctx[:4], FIELD, candidates=cand, k=3, exclude=ex, by=USER)
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1].view(np.uint32), plain[1].view(np.uint32))


def test_a_repeated_seen_id_loses_every_copy(model, data):
    ctx = positives(data.Train_data)[:3]
    seen_id = int(ctx[0, FIELD])                                                  # context 0's own user has it in the train split
    cand = np.array([5, seen_id, 9, seen_id, 12, 5, seen_id], dtype=np.int32)
    mask = loop_mask(ctx, cand, [FIELD], [data.Train_data], USER)
    assert mask[0].tolist() == [0, 1, 0, 1, 0, 0, 1]
    ids, val = model.recommend(ctx, FIELD, candidates=cand, k=7, exclude=data.Train_data, by=USER)
    idx, bits_, count = R.topk_ref(_score(R.expand_ref(ctx, FIELD, cand, 0, 3 * 7)).reshape(3, 7), 7, mask)
    assert count[0] == 4 and seen_id not in ids[0] and (ids[0] >= 0).sum() == 4
    assert np.array_equal(ids, np.where(idx >= 0, cand[np.maximum(idx, 0)], -1)) and np.array_equal(val.view(np.uint32), bits_)
    # the same through the tuple method, which returns positions
    pos, _ = model.recommend_tuples(ctx, [FIELD], cand, k=7, exclude=data.Train_data, by=USER)
    assert np.array_equal(pos, idx)
    # in evaluation the target's own copies stay out of its way too: the first copy is the target, the other copies are skipped
    rows = {'X': [[int(t) for t in ctx[0]]], 'Y': [1.0]}
    scores = _score(R.expand_ref(ctx[:1], FIELD, cand, 0, 7)).reshape(1, 7)
    want = M.ranking_metrics(R.rank_ref(scores, np.array([1]), mask[:1]), 2)
    assert model.evaluate_ranking(rows, FIELD, k=2, candidates=cand, exclude=data.Train_data, by=USER) == pytest.approx(want, abs=1e-12)


def test_groups_of_contexts_give_the_result_of_one_group(model, data):
    ctx = X(data.Test_data)[:11]
    cand = np.unique(X(data.Train_data)[:, FIELD]).astype(np.int32)
    kw = dict(k=5, exclude=[data.Train_data, data.Validation_data], by=9)
    one = model.recommend(ctx, FIELD, **kw)
    assert [c[:2] for c in _calls(model)] == [('score', 11), ('seen_mask', 11), ('topk', ['skip'])]
    cut = model.recommend(ctx, FIELD, score_rows=3 * cand.size, **kw)
    assert [c[:2] for c in _calls(model)] == [('score', 3), ('seen_mask', 3), ('topk', ['skip'])] * 3 + \
        [('score', 2), ('seen_mask', 2), ('topk', ['skip'])]
    assert np.array_equal(one[0], cut[0]) and np.array_equal(one[1].view(np.uint32), cut[1].view(np.uint32))
    ev = dict(k=10, exclude=data.Train_data, by=9)
    assert model.evaluate_ranking(data.Test_data, FIELD, **ev) == model.evaluate_ranking(data.Test_data, FIELD, score_rows=4 * 200, **ev)


def test_every_refusal_comes_ahead_of_any_engine_call(model, data):
    ctx = X(data.Test_data)[:3]
    tr, te = data.Train_data, data.Test_data
    tup = np.unique(X(tr)[:, list(FIELDS)], axis=0)
    calls = {
        'recommend': lambda **kw: model.recommend(ctx, FIELD, **kw),
        'recommend_tuples': lambda **kw: model.recommend_tuples(ctx, FIELDS, tup, **kw),
        'evaluate_ranking': lambda **kw: model.evaluate_ranking(te, FIELD, **kw),
        'evaluate_ranking_tuples': lambda **kw: model.evaluate_ranking_tuples(te, FIELDS, **kw),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match=r'%s\(\).*\bby\b' % name):           # one keyword names the other
            call(exclude=tr)
        with pytest.raises(ValueError, match=r'%s\(\).*\bexclude\b' % name):
            call(by=USER)
        for by in (-1, 10, 1.5, 'user', True):
            with pytest.raises(ValueError, match='by='):
                call(exclude=tr, by=by)
        with pytest.raises(ValueError, match='swept'):
            call(exclude=tr, by=FIELD)
        for ex in ([], 'train', [tr, None], {'X': []}):
            with pytest.raises(ValueError, match='exclude'):
                call(exclude=ex, by=USER)
    with pytest.raises(ValueError, match='swept'):
        calls['recommend_tuples'](exclude=tr, by=6)
    with pytest.raises(ValueError, match=r'exclude.*negatives|negatives.*exclude'):
        calls['evaluate_ranking_tuples'](exclude=tr, by=USER, negatives=5)
    with pytest.raises(ValueError, match=r'exclude.*per_context|per_context.*exclude'):
        model.recommend_tuples(ctx, FIELDS, np.stack([tup[:4]] * 3), per_context=True, exclude=tr, by=USER)
    assert _calls(model) == []


def test_without_the_keywords_the_calls_are_the_calls_of_before(model, data):
    ctx = X(data.Test_data)[:5]
    tup = np.unique(X(data.Train_data)[:, list(FIELDS)], axis=0)
    P = len(positives(data.Test_data))
    skip = np.zeros((5, len(tup)), dtype=bool)
    skip[0, 0] = True
    model.recommend(ctx, FIELD)
    assert _calls(model) == [('score', 5), ('topk', ['skip'], False)]             # topk(scores, k, skip=None), as it always was
    model.recommend_tuples(ctx, FIELDS, tup, skip=skip, exclude=None, by=None)
    assert _calls(model) == [('score', 5), ('topk', ['skip'], True)]
    model.evaluate_ranking(data.Test_data, FIELD)
    assert _calls(model) == [('score', P), ('rank_of', [])]                       # rank_of(scores, tpos): no skip argument at all
    model.evaluate_ranking_tuples(data.Test_data, FIELDS)
    assert _calls(model) == [('score', P), ('rank_of', [])]
    model.evaluate_ranking_tuples(data.Test_data, FIELDS, negatives=4)
    assert _calls(model) == [('score', P), ('rank_of', [])]
