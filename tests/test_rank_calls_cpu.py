"""The five public ranking methods of CFFM (recommend, evaluate_ranking, recommend_tuples, evaluate_ranking_tuples, train_ranking) on
one recording stub engine (no GPU), through a fixed matrix of calls on the committed frappe slice: for every call the sequence of
engine calls - method name, and per argument the shape, dtype and sha256 of a tensor's bytes or the scalar itself - and the sha256 of
the returned arrays or the bits of the returned floats, compared with tests/golden/rank_calls.json.  The fixture says what the class
asks of the engine and what it returns; a change of the host code that leaves both alone leaves this test alone.

The stub is composed from the stubs of the other ranking class tests: its scores are the _score of tests/test_rank_class_cpu.py, its
draws the numpy twins of cffm_amd.spec.  `python -m tests.test_rank_calls_cpu --record` writes the fixture; the test never writes."""
import contextlib
import hashlib
import io
import json
import os
import struct
import sys

import numpy as np
import pytest
import torch

from cffm_amd import CFFM as M
from cffm_amd.LoadData import LoadData
from tests.test_draw_weighted_class_cpu import _StubEngine as _DrawStub
from tests.test_sweep_tuples_class_cpu import _TupleStub

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'golden', 'frappe_slice') + '/'
GOLDEN = os.path.join(HERE, 'golden', 'rank_calls.json')
FIELD, FIELDS = 1, (1, 6)
RECORDED = ('score_candidates', 'score_candidates_shared', 'score_candidate_lists_shared', 'score_candidate_tuples',
            'score_candidate_tuples_shared', 'topk', 'rank_of', 'draw_lists', 'draw_lists_weighted', 'train_step_lists',
            'train_step_lists_fused')


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _describe(v):
    if isinstance(v, torch.Tensor):
        return [list(v.shape), str(v.dtype), _sha(v.contiguous().numpy())]
    if isinstance(v, (list, tuple)):
        return [_describe(x) for x in v]
    if v is None or isinstance(v, (bool, int, str)):
        return v
    raise TypeError('an engine argument of type %s' % type(v).__name__)


def _result(v):
    if isinstance(v, np.ndarray):
        return [list(v.shape), str(v.dtype), _sha(v)]
    if isinstance(v, float):
        return struct.pack('<d', v).hex()
    return [_result(x) for x in v]


class _Stub(_DrawStub, _TupleStub):
    """Every stub method of the ranking class tests in one engine, plus a fused list step that is the stage stub's and is served
    for B >= 24 rows."""

    def list_step_ok(self, B):
        return int(B) >= 24

    def train_step_lists_fused(self, ctx, fields, cand, target, kind):
        return _DrawStub.train_step_lists(self, ctx, fields, cand, target, kind)


def _recorded(name):
    def call(self, *args, **kwargs):
        self.log.append([name, _describe(args), {k: _describe(v) for k, v in sorted(kwargs.items())}])
        return getattr(_Stub, name)(self, *args, **kwargs)
    return call


class _Recorder(_Stub):
    """_Stub with every call of a RECORDED method logged with its arguments, in order."""

    def __init__(self, cfg, seed):
        _Stub.__init__(self, cfg, seed)
        self.log = []


for _name in RECORDED:
    setattr(_Recorder, _name, _recorded(_name))


def _load():
    with contextlib.redirect_stdout(io.StringIO()):
        return LoadData(PATH, 'frappe', 'square_loss')


def _model(save_dir, data):
    m = M.CFFM(data.features_M, 0, os.path.join(str(save_dir), 'm'), 8, 8, 'square_loss', 1, 16, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer',
               0, 0, 0, 10, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'relu')
    m.build_graph()
    m._train_split = data.Train_data
    m._all_reduce_sum = lambda t: t                                           # no group here: every rank's own sums
    return m


def _matrix(data):
    """(label, SWEEP_MIN_N, (world, rank), method name, args, kwargs) of every call, in a fixed order."""
    rng = np.random.default_rng(17)
    train, test = data.Train_data, data.Test_data
    ctx = np.asarray(test['X'][:5], dtype=np.int32)
    C, N = 5, 9
    cand30 = np.arange(20, 50, dtype=np.int32)
    skip30 = rng.random((C, 30)) < 0.3
    col = lambda split: {row[FIELD] for row in split['X']}
    n_eval = len(col(train) | col(test))                                      # evaluate_ranking's default N
    calls = []
    for sweep in ('expand', 'shared', 'auto'):
        for side in (0, 1):                                                   # N >= SWEEP_MIN_N, then N < SWEEP_MIN_N
            tag = '%s/min_n=N+%d' % (sweep, side)
            calls.append(('recommend ' + tag, 30 + side, (1, 0), 'recommend', (ctx, FIELD),
                          dict(candidates=cand30, k=4, skip=skip30 if side else None, score_rows=2 * 30, sweep=sweep)))
            calls.append(('evaluate_ranking ' + tag, n_eval + side, (1, 0), 'evaluate_ranking', (test, FIELD),
                          dict(k=10, score_rows=12 * n_eval, sweep=sweep)))
    calls.append(('recommend defaults', M.SWEEP_MIN_N, (1, 0), 'recommend', (ctx, FIELD), {}))
    calls.append(('evaluate_ranking explicit', M.SWEEP_MIN_N, (1, 0), 'evaluate_ranking', (test, FIELD),
                  dict(k=3, candidates=rng.permutation(np.array(sorted(col(train) | col(test)), dtype=np.int64)))))
    for rank in range(3):
        calls.append(('evaluate_ranking world=3 rank=%d' % rank, M.SWEEP_MIN_N, (3, rank), 'evaluate_ranking', (test, FIELD),
                      dict(k=10, score_rows=5 * n_eval)))
    one, two = rng.integers(0, 200, size=N).astype(np.int32), rng.integers(0, 200, size=(N, 2)).astype(np.int32)
    one_pc, two_pc = rng.integers(0, 200, size=(C, N)).astype(np.int32), rng.integers(0, 200, size=(C, N, 2)).astype(np.int32)
    skip, counts = rng.random((C, N)) < 0.3, np.array([9, 0, 3, 7, 1])
    for name, fields, cand, pc in (('[N]', 1, one, False), ('[N,2]', FIELDS, two, False), ('[C,N]', 1, one_pc, True),
                                   ('[C,N,2]', FIELDS, two_pc, True)):
        for sweep in ('expand', 'auto', 'tuples') + (('shared',) if fields == 1 else ()):
            kw = dict(per_context=pc, k=4, skip=skip, score_rows=2 * N, sweep=sweep)
            if pc:
                kw['counts'] = counts
            calls.append(('recommend_tuples %s %s' % (name, sweep), 1, (1, 0), 'recommend_tuples', (ctx, fields, cand), kw))
    calls.append(('recommend_tuples defaults', M.SWEEP_MIN_N, (1, 0), 'recommend_tuples', (ctx, FIELDS, two), {}))
    ev = 'evaluate_ranking_tuples '
    for sweep in ('expand', 'tuples'):
        calls.append((ev + 'shared list ' + sweep, M.SWEEP_MIN_N, (1, 0), 'evaluate_ranking_tuples', (test, FIELDS),
                      dict(k=10, score_rows=3 * 150, sweep=sweep)))
    calls.append((ev + 'one field auto', 1, (1, 0), 'evaluate_ranking_tuples', (test, FIELD), dict(k=5, sweep='auto')))
    for sampler in ('host', 'device'):
        calls.append((ev + 'negatives=3 ' + sampler, M.SWEEP_MIN_N, (1, 0), 'evaluate_ranking_tuples', (test, FIELDS),
                      dict(k=2, negatives=3, seed=11, score_rows=4 * 10, sampler=sampler)))
        for rank in range(3):
            calls.append((ev + 'negatives=3 %s world=3 rank=%d' % (sampler, rank), M.SWEEP_MIN_N, (3, rank), 'evaluate_ranking_tuples',
                          (test, FIELDS), dict(k=2, negatives=3, seed=11, sampler=sampler)))
    calls.append((ev + 'negatives=3 one field auto', 1, (1, 0), 'evaluate_ranking_tuples', (test, FIELD),
                  dict(k=2, negatives=3, seed=2, sweep='auto')))
    for rank in range(3):
        calls.append((ev + 'popularity world=3 rank=%d' % rank, M.SWEEP_MIN_N, (3, rank), 'evaluate_ranking_tuples', (test, FIELDS),
                      dict(k=2, negatives=3, seed=11, sampler='device', negative_weights='popularity')))
    distinct = np.unique(np.concatenate([np.asarray(s['X'], dtype=np.int32)[:, list(FIELDS)] for s in (train, test)]), axis=0)
    calls.append((ev + 'explicit candidates, weights', M.SWEEP_MIN_N, (1, 0), 'evaluate_ranking_tuples', (test, FIELDS),
                  dict(k=2, candidates=np.concatenate([distinct, distinct[:5]]), negatives=3, seed=3, sampler='device',
                       negative_weights=1.0 + np.arange(distinct.shape[0]) % 5)))
    for sampler in ('host', 'device'):
        for step in ('stages', 'auto'):                                       # 37 positives: 4 steps of 8 lists and one of 5
            calls.append(('train_ranking %s %s' % (sampler, step), M.SWEEP_MIN_N, (1, 0), 'train_ranking', (train, FIELDS),
                          dict(negatives=3, loss='softmax' if step == 'auto' else 'bpr', epochs=2, lists_per_step=8, seed=5, step=step,
                               sampler=sampler)))
    calls.append(('train_ranking popularity fused', M.SWEEP_MIN_N, (1, 0), 'train_ranking', (train, FIELDS),
                  dict(negatives=4, epochs=2, seed=5, step='fused', sampler='device', negative_weights='popularity', negative_power=0.5)))
    calls.append(('train_ranking defaults', M.SWEEP_MIN_N, (1, 0), 'train_ranking', (train, FIELD), {}))
    return calls


def _run(save_dir, data):
    """{label: {'engine': the engine calls, 'returns': what the method returned}} over the matrix, each call on a fresh model."""
    out = {}
    min_n = M.SWEEP_MIN_N
    try:
        for label, sweep_min_n, (world, rank), method, args, kwargs in _matrix(data):
            M.SWEEP_MIN_N = sweep_min_n                                       # the module attribute, read at call time
            m = _model(save_dir, data)
            m.world, m.rank = world, rank
            got = getattr(m, method)(*args, **kwargs)
            assert label not in out
            out[label] = {'engine': m.engine.log, 'returns': _result(got)}
    finally:
        M.SWEEP_MIN_N = min_n
    return out


@pytest.fixture(scope='module')
def got(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setattr(M.CFFM, 'engine_factory', _Recorder)
    mp.delenv('CFFM_TABLES', raising=False)
    try:
        return _run(tmp_path_factory.mktemp('rank_calls'), _load())
    finally:
        mp.undo()


def test_every_engine_call_and_every_result_is_the_recorded_one(got):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want['calls'])
    for label in want['calls']:
        g, w = json.loads(json.dumps(got[label])), want['calls'][label]
        assert [c[0] for c in g['engine']] == [c[0] for c in w['engine']], label
        for i, (a, b) in enumerate(zip(g['engine'], w['engine'])):
            assert a == b, '%s: engine call %d (%s)' % (label, i, b[0])
        assert g['returns'] == w['returns'], label


def test_the_matrix_reaches_every_engine_method(got):
    seen = {c[0] for rec in got.values() for c in rec['engine']}
    assert seen == set(RECORDED)
    kinds = lambda label: [c[0] for c in got[label]['engine']]
    assert len(kinds('evaluate_ranking expand/min_n=N+0')) > 2                # several groups of contexts
    steps = [k for k in kinds('train_ranking host auto') if k.startswith('train_step')]
    assert steps == (['train_step_lists_fused'] * 4 + ['train_step_lists']) * 2      # the ragged last step is not served


if __name__ == '__main__':
    if sys.argv[1:] != ['--record'] or len(sys.argv) != 2:
        sys.exit('usage: python -m tests.test_rank_calls_cpu --record')
    import tempfile
    M.CFFM.engine_factory = _Recorder
    os.environ.pop('CFFM_TABLES', None)
    with tempfile.TemporaryDirectory() as tmp:
        calls = _run(tmp, _load())
    with open(GOLDEN, 'w') as f:
        json.dump({'calls': calls}, f, sort_keys=True, separators=(',', ':'))
        f.write('\n')
    print('%d calls, %d engine calls -> %s' % (len(calls), sum(len(c['engine']) for c in calls.values()), GOLDEN))
