"""GPU: candidates that are tuples of ids and candidate lists per context - cffm_expand_candidates_ex through the C ABI bit for bit
against the loop-level numpy reading of tests/_cand_ref.py, the engine's score_candidate_tuples against predict on the numpy-expanded
rows, and the class's recommend_tuples / evaluate_ranking_tuples on the committed frappe slice and at world size 2.

The id rows are written into a Guard of tests/test_gpu_rows.py (canaries on both sides, a poison payload) that is 16 values longer
than rows * F: the tail must keep its poison.  Context ids are < 1000, candidate ids >= 10000 and distinct per (context, n, a), and
the gap behind a context's list holds ids <= -10000 - an index that is off by one in any direction shows as a wrong value.

Shapes: F in {2, 10, 64} (the slot map's two ends), nf in {1, 2, F}, C in {1, 3, 130}, N in {1, 63, 65} - more than one workgroup
of 256 values at all but the smallest - strides 0 (one shared list), N * nf and N * nf + 3; pieces (0, all), (60, 10) at N = 65 (it
crosses a context) and the last row alone.  Not the full product: the reference is a Python loop over every value, so C = 130 is
taken with N = 1 at every (F, nf) and with N = 65 at the two ends nf = 1 and nf = F."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cffm_amd.spec import CFFMConfig, init_params  # noqa: E402
from oracle import rows_check as rc  # noqa: E402
from tests import _cand_ref as CR  # noqa: E402
from tests import _rank_ref as R  # noqa: E402
from tests import test_dist_cpu as H  # noqa: E402   (the spawn / gloo harness)
from tests.test_gpu_rows import Guard, dev_of, stream  # noqa: E402

pytestmark = pytest.mark.gpu

TAIL = 16


@functools.lru_cache(maxsize=None)
def lib():
    from cffm_amd import hip
    hip.load()
    return hip.fast()


def expand_ex(shape, d_ctx, C, fields, d_cand, stride, N, first, rows, name):
    """cffm_expand_candidates_ex into a guarded buffer: the rows * F values, after the canaries and the tail were checked."""
    F = int(shape.F)
    host = (ctypes.c_int32 * len(fields))(*fields)
    out = Guard((rows * F + TAIL) * 4)
    rcode = lib().cffm_expand_candidates_ex(ctypes.addressof(shape), d_ctx.data_ptr(), C, ctypes.addressof(host), len(fields),
                                            d_cand.data_ptr(), stride, N, first, rows, out.ptr, stream())
    assert rcode == 0, '%s returned %d' % (name, rcode)
    got = out.read(name, np.int32)
    rc.check_untouched(name + ': beyond rows * F values', got[rows * F:].view(np.float32))
    return got[:rows * F].reshape(rows, F)


def fields_of(F, nf, rng):
    return [int(f) for f in rng.permutation(F)[:nf]]                          # any order: tuple id a goes to column fields[a]


@pytest.mark.parametrize('F', [2, 10, 64])
def test_expand_ex(F):
    from cffm_amd import hip
    shape = hip.make_shape(CFFMConfig(M=50, F=F, K=8, D=8))
    rng = np.random.default_rng(F)
    for nf in sorted({1, 2, F}):
        sizes = [(1, 1), (1, 65), (3, 63), (3, 65), (130, 1)] + ([(130, 65)] if nf in (1, F) else [])
        for C, N in sizes:
            fields = fields_of(F, nf, rng)
            ctx = rng.integers(0, 1000, size=(C, F)).astype(np.int32)
            lists = (10000 + np.arange(C * N * nf, dtype=np.int32)).reshape(C, N, nf)
            d_ctx = dev_of(ctx)
            for stride in (0, N * nf, N * nf + 3):
                flat = lists[0].reshape(-1) if stride == 0 else CR.flat_lists(lists, stride, -10000)
                if stride > N * nf:
                    flat = flat - (flat < 0) * np.arange(flat.size, dtype=np.int32)          # every gap value its own
                d_cand = dev_of(flat)
                total = C * N
                pieces = [(0, total), (total - 1, 1)] + ([(60, 10)] if N == 65 and total >= 70 else [])
                whole = CR.expand_ex_ref(ctx, fields, flat, stride, N, 0, total)
                for first, rows in pieces:
                    name = 'expand_ex F=%d nf=%d fields=%s C=%d N=%d stride=%d piece (%d, %d)' % (F, nf, fields, C, N, stride, first, rows)
                    got = expand_ex(shape, d_ctx, C, fields, d_cand, stride, N, first, rows, name)
                    ref = whole if rows == total else CR.expand_ex_ref(ctx, fields, flat, stride, N, first, rows)
                    rc.check_exact(name, got, ref)
                    assert np.array_equal(ref, whole[first:first + rows])
                if nf == 1 and stride == 0:                                   # the entry point it generalises, on the same inputs
                    for first, rows in pieces:
                        old = Guard((rows * F + TAIL) * 4)
                        assert lib().cffm_expand_candidates(ctypes.addressof(shape), d_ctx.data_ptr(), C, fields[0], d_cand.data_ptr(), N,
                                                            first, rows, old.ptr, stream()) == 0
                        rc.check_exact('cffm_expand_candidates F=%d C=%d N=%d piece (%d, %d)' % (F, C, N, first, rows),
                                       old.read('old', np.int32)[:rows * F].reshape(rows, F), whole[first:first + rows])


def test_expand_ex_writes_nothing_when_there_is_nothing_to_do():
    from cffm_amd import hip
    shape = hip.make_shape(CFFMConfig(M=50, F=4, K=8, D=8))
    host = (ctypes.c_int32 * 2)(1, 3)
    ctx, cand = dev_of(np.zeros((3, 4), dtype=np.int32)), dev_of(np.arange(10, dtype=np.int32))
    for C, first, rows, want in ((3, 7, 0, 0), (0, 0, 0, 0), (3, 0, 16, 10001), (3, 15, 1, 10001)):
        out = Guard(64)
        assert lib().cffm_expand_candidates_ex(ctypes.addressof(shape), ctx.data_ptr(), C, ctypes.addressof(host), 2, cand.data_ptr(), 0, 5,
                                               first, rows, out.ptr, stream()) == want
        rc.check_untouched('C=%d piece (%d, %d)' % (C, first, rows), out.read('out'))


# ---- HipEngine.score_candidate_tuples ----------------------------------------------------------------------------------------
FRAPPE = CFFMConfig(M=5382, F=10, K=32, D=32, activation='selu')


def ref_tuple_scores(eng, ctx, fields, cand, block):
    """engine.predict over the numpy-expanded id rows, cut into the pieces score_candidate_tuples cuts the flattened range into."""
    X = CR.expand_tuples(ctx, list(fields), cand)
    out = np.empty(X.shape[0], dtype=np.float32)
    for s0 in range(0, X.shape[0], block):
        out[s0:s0 + block] = eng.predict(dev_of(X[s0:s0 + block])).cpu().numpy()
    return out.reshape(ctx.shape[0], -1)


def test_score_candidate_tuples_equals_predict_on_the_expanded_rows():
    from cffm_amd.engine import HipEngine
    cfg, C, N, block = FRAPPE, 3, 65, 50                                      # ragged pieces that cut the contexts
    rng = np.random.default_rng(C + N)
    p = init_params(cfg, seed=3)
    p['feature_bias'] = (rng.standard_normal(p['feature_bias'].shape) * 0.3).astype(np.float32)
    eng = HipEngine(cfg, params=p)
    ctx = rng.integers(0, cfg.M, size=(C, cfg.F)).astype(np.int32)
    fields = (6, 1)
    shared = rng.integers(0, cfg.M, size=(N, 2)).astype(np.int32)
    shared[1], shared[N - 1] = (-1, cfg.M), (cfg.M + 5, -3)                   # clamped by the forward, as predict clamps them
    per_ctx = rng.integers(0, cfg.M, size=(C, N, 2)).astype(np.int32)
    for name, cand in (('shared', shared), ('per-context', per_ctx)):
        got = eng.score_candidate_tuples(dev_of(ctx), fields, dev_of(cand), block=block)
        assert got.shape == (C, N) and got.dtype == torch.float32
        want = ref_tuple_scores(eng, ctx, fields, cand, block)
        assert np.unique(want).size > N // 2, 'the scores do not depend on the candidate'
        rc.check_exact('score_candidate_tuples %s' % name, got.cpu().numpy().reshape(-1), want.reshape(-1))
    # one field, one list: the bits of score_candidates
    one = eng.score_candidate_tuples(dev_of(ctx), [6], dev_of(shared[:, :1].copy()), block=block)
    rc.check_exact('nf = 1 against score_candidates', one.cpu().numpy(),
                   eng.score_candidates(dev_of(ctx), 6, dev_of(shared[:, 0].copy()), block=block).cpu().numpy())
    for bad_fields, bad_cand in (((1, 1), shared), ((1, 10), shared), ((), shared), ((1,), shared), ((1, 6), per_ctx[:2]),
                                 ((1, 6), shared[:0])):
        with pytest.raises(ValueError):
            eng.score_candidate_tuples(dev_of(ctx), bad_fields, dev_of(bad_cand))


# ---- CFFM.recommend_tuples / CFFM.evaluate_ranking_tuples ----------------------------------------------------------------------
FIELDS = (1, 6)


def test_class_on_the_frappe_slice(tmp_path):
    from tests.test_gpu_rank import _frappe_model
    M, m, data = _frappe_model(tmp_path)
    eng = m.engine
    rows_of = lambda split: np.asarray(split['X'], dtype=np.int32)
    distinct = np.unique(rows_of(data.Train_data)[:, list(FIELDS)], axis=0)
    ctx = rows_of(data.Test_data)[:6]
    C, k = ctx.shape[0], 5
    # one shared list of tuples
    want = ref_tuple_scores(eng, ctx, FIELDS, distinct, 8192)
    skip = np.random.default_rng(1).random(want.shape) < 0.2
    for sk in (None, skip):
        pos, val = m.recommend_tuples(ctx, FIELDS, distinct, k=k, skip=sk)
        ridx, rval, _ = R.topk_ref(want, k, sk)
        rc.check_exact('recommend_tuples shared pos', pos, ridx)
        rc.check_exact('recommend_tuples shared scores', val.view(np.uint32), rval)
    # a list per context, padded behind counts[c] candidates with ids that must not matter
    rng = np.random.default_rng(2)
    N = 40
    lists = distinct[rng.integers(0, distinct.shape[0], size=(C, N))]
    counts = np.array([N, 0, 1, 17, 39, 8])
    pad = np.arange(N)[None, :] >= counts[:, None]
    want = ref_tuple_scores(eng, ctx, FIELDS, lists, 8192)
    padded = lists.copy()
    padded[pad] = -5
    pos, val = m.recommend_tuples(ctx, FIELDS, padded, per_context=True, counts=counts, k=k, score_rows=3 * N)
    ridx, rval, rcount = R.topk_ref(want, k, pad)
    assert rcount.tolist() == np.minimum(counts, k).tolist()
    rc.check_exact('recommend_tuples per-context pos', pos, ridx)
    rc.check_exact('recommend_tuples per-context scores', val.view(np.uint32), rval)
    # the sampled protocol: the lists the class drew are read off the engine call; the reference is predict on their expanded rows
    test = data.Test_data
    both = np.unique(np.concatenate([rows_of(data.Train_data), rows_of(test)])[:, list(FIELDS)], axis=0)
    rows = rows_of(test)[np.asarray(test['Y']).reshape(-1) > 0]
    neg = min(20, both.shape[0] - 1)
    seen = []
    inner = eng.score_candidate_tuples

    def recording(c, fields, cand, block=8192):
        seen.append((c.cpu().numpy(), cand.cpu().numpy()))
        return inner(c, fields, cand, block)
    eng.score_candidate_tuples = recording
    got = m.evaluate_ranking_tuples(test, FIELDS, k=3, negatives=neg, seed=5)
    again = m.evaluate_ranking_tuples(test, FIELDS, k=3, negatives=neg, seed=5)
    eng.score_candidate_tuples = inner
    assert np.array_equal(np.array(got).view(np.uint64), np.array(again).view(np.uint64))
    seen = seen[:len(seen) // 2]
    drawn = np.concatenate([s[1] for s in seen])
    assert np.array_equal(np.concatenate([s[0] for s in seen]), rows) and drawn.shape == (rows.shape[0], neg + 1, 2)
    is_target = (drawn == rows[:, None, list(FIELDS)]).all(axis=2)
    assert (is_target.sum(axis=1) == 1).all()
    ranks = R.rank_ref(ref_tuple_scores(eng, rows, FIELDS, drawn, 8192), is_target.argmax(axis=1))
    want = M.ranking_metrics(ranks, 3)
    print('frappe slice, fields %s: %d positive rows, %d distinct tuples, %d negatives, HR@3 %.6f NDCG@3 %.6f'
          % (FIELDS, rows.shape[0], both.shape[0], neg, got[0], got[1]))
    assert 0.0 < want[0] < 1.0, ranks                                         # the case separates hits from misses
    assert abs(got[0] - want[0]) <= 1e-12 and abs(got[1] - want[1]) <= 1e-12, (got, want)
    # one shared list of all distinct tuples
    scores = ref_tuple_scores(eng, rows, FIELDS, both, 8192)
    target = np.array([int(np.nonzero((both == t).all(axis=1))[0][0]) for t in rows[:, list(FIELDS)]])
    want = M.ranking_metrics(R.rank_ref(scores, target), 10)
    got = m.evaluate_ranking_tuples(test, FIELDS, k=10)
    assert abs(got[0] - want[0]) <= 1e-12 and abs(got[1] - want[1]) <= 1e-12, (got, want)
    # one field through the shared sweep, a list per context: the order is defined on those scores themselves
    ids = np.unique(rows_of(data.Train_data)[:, 1])
    lists1 = ids[rng.integers(0, ids.size, size=(C, N))]
    shared = eng.score_candidate_lists_shared(dev_of(ctx), 1, dev_of(lists1)).cpu().numpy()
    pos, val = m.recommend_tuples(ctx, 1, lists1, per_context=True, k=k, sweep='shared')
    ridx, rval, _ = R.topk_ref(shared, k)
    rc.check_exact('recommend_tuples sweep=shared pos', pos, ridx)
    rc.check_exact('recommend_tuples sweep=shared scores', val.view(np.uint32), rval)


def _tuples_worker(rank, world, tmp):
    """evaluate_ranking_tuples(negatives=m) of the SAME untrained model (one seed; under a group rank 0's parameters are broadcast)
    at any world size."""
    from cffm_amd import CFFM as M
    from cffm_amd import synth

    class Split(dict):
        pass
    rng = np.random.default_rng(11)
    Mf, F = 200, 4                                                           # 50 ids per field (cffm_amd.synth.field_ranges)
    test = Split(X=synth.sample_ids(rng, Mf, F, 91).tolist(), Y=synth.sample_labels(rng, 91).tolist())
    m = M.CFFM(Mf, 0, os.path.join(tmp, 't%d_w%d' % (rank, world)), 8, 8, 'square_loss', 1, 8, 0.05, 0, [1.0, 1.0],
               'AdagradOptimizer', 0, 0, 0, F, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'relu')
    m.build_graph()
    assert m.world == world
    return m.evaluate_ranking_tuples(test, (1, 2), k=3, negatives=12, seed=4), sum(1 for v in test['Y'] if v > 0)


def test_evaluate_ranking_tuples_world2_equals_world1(tmp_path):
    one, n_pos = H._run(_tuples_worker, 1, str(tmp_path))[0]
    two = H._run(_tuples_worker, 2, str(tmp_path))
    assert n_pos >= 16
    assert 0.0 < one[0] < 1.0, one                                             # the case separates hits from misses
    for rank in (0, 1):
        got = two[rank][0]
        assert abs(got[0] - one[0]) <= 1e-12 and abs(got[1] - one[1]) <= 1e-12, (rank, got, one)
