"""GPU: the candidate sweep with the fixed-field work done once per context (cffm_amd/csrc/sweep.hip) - cffm_score_sweep through
the C ABI against the float64 oracle on the numpy-expanded id rows, its independence of the candidate's position bit for bit,
the engine's score_candidates_shared against the path it replaces, and the class's sweep= keyword on the committed frappe slice.

The scores and the scratch of every ABI call are Guards of tests/test_gpu_rows.py: canaries on both sides, a NaN poison payload.
The scores lie in rows of N + 5 floats whose 5-float gap holds 3e38, which must survive.

Parity is oracle.parity.close(got, ref, 'out') at its default tolerance, the criterion of every predict check.  float32 numpy
stand-ins of both summation orders pass it at a worst err/bound of 0.01 - 0.07 on these shapes, and a dropped V term or a
transposed tap index of U fails it at err/bound 500 - 2,300: it sees the layer-0 algebra through `out`.

Shapes: the smallest at which the kernels can still go wrong - F = 2 (no fixed pair at all), Pp = 16 / 32 / 48 (the three kernel
instances), the swept field at both ends (U or V empty) and in the middle, N below, at and above the chunk of candidates one
workgroup unit takes, one context spread over several units, candidate ids outside [0, M)."""
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

from cffm_amd import hip  # noqa: E402
from cffm_amd.spec import CFFMConfig, init_params  # noqa: E402
from oracle import cffm_oracle as orc  # noqa: E402
from oracle import parity as T  # noqa: E402
from oracle import rows_check as rc  # noqa: E402
from tests import _rank_ref as R  # noqa: E402
from tests.test_gpu_rows import Guard, dev_of, stream  # noqa: E402

pytestmark = pytest.mark.gpu

GAP, SENTINEL = 5, np.float32(3e38)
CHUNK = hip.SWEEP_CHUNK

CASES = {
    'f2-relu': (CFFMConfig(M=60, F=2, K=8, D=32, activation='relu'), 3, 70),            # no fixed pair at all: Zctx == 0
    'f3-relu': (CFFMConfig(M=60, F=3, K=8, D=32, activation='relu'), 3, 70),
    'f7-gelu': (CFFMConfig(M=90, F=7, K=8, D=32, activation='gelu'), 2, 70),
    'f8-prelu-noatt': (CFFMConfig(M=90, F=8, K=16, D=32, activation='prelu', linear_att=0), 2, 70),
    'f6-elu': (CFFMConfig(M=90, F=6, K=8, D=32, activation='elu'), 2, 70),
    'frappe-selu': (CFFMConfig(M=5382, F=10, K=32, D=32, activation='selu'), 2, 300),
}
UNSERVED = {
    'f6-d64-elu': CFFMConfig(M=90, F=6, K=8, D=64, activation='elu'),
    'f11-relu': CFFMConfig(M=90, F=11, K=8, D=32, activation='relu'),
    'f4-d8': CFFMConfig(M=50, F=4, K=8, D=8),
}


@functools.lru_cache(maxsize=None)
def params_of(name):
    cfg = CASES[name][0] if name in CASES else UNSERVED[name]
    p = init_params(cfg, seed=3)
    rng = np.random.default_rng(17)
    p['feature_bias'] = (rng.standard_normal(p['feature_bias'].shape) * 0.3).astype(np.float32)
    return cfg, p


@functools.lru_cache(maxsize=2)
def engine_of(name):
    from cffm_amd.engine import HipEngine
    cfg, p = params_of(name)
    return HipEngine(cfg, params=p)


def inputs_of(name, C, N, seed=0):
    cfg, _ = params_of(name)
    rng = np.random.default_rng(1000 * C + N + seed)
    ctx = rng.integers(0, cfg.M, size=(C, cfg.F)).astype(np.int32)
    cand = rng.integers(0, cfg.M, size=N).astype(np.int32)
    if N <= cfg.M:
        cand = rng.permutation(cfg.M)[:N].astype(np.int32)
    return ctx, cand


def sweep_abi(eng, ctx, field, cand, label):
    """cffm_score_sweep into guarded, gapped rows; returns the [C, N] scores on the host after the canaries, the gap and the
    scratch's canaries have been checked."""
    C, N = ctx.shape[0], cand.size
    lib = eng.lib
    nbytes = int(lib.cffm_sweep_scratch_bytes(eng._s, C))
    assert nbytes > 0, label
    scores, scratch = Guard(C * (N + GAP) * 4), Guard(nbytes)
    scores.view().reshape(C, N + GAP)[:, N:] = float(SENTINEL)
    dctx, dcand = dev_of(ctx), dev_of(cand)
    rcode = lib.cffm_score_sweep(eng._s, eng._t, eng.theta.data_ptr(), dctx.data_ptr(), C, int(field), dcand.data_ptr(), N, scores.ptr,
                                 N + GAP, scratch.ptr, stream())
    assert rcode == 0, '%s returned %d' % (label, rcode)
    img = scores.read(label).reshape(C, N + GAP)
    scratch.read(label + ' scratch')
    rc.check_exact(label + ': the gap behind every row', img[:, N:], np.full((C, GAP), SENTINEL, dtype=np.float32))
    got = np.ascontiguousarray(img[:, :N])
    assert not (rc.bits(got) == rc.POISON).any(), '%s: scores left at poison' % label
    return got


def oracle_scores(name, ctx, field, cand):
    """cffm_oracle.forward in float64 on the numpy-expanded ids (clamped as the forward clamps them), in pieces of 100 rows."""
    cfg, p = params_of(name)
    p64 = {k: np.asarray(v, dtype=np.float64) for k, v in p.items()}
    C, N = ctx.shape[0], cand.size
    X = np.clip(R.expand_ref(ctx, field, cand, 0, C * N), 0, cfg.M - 1)
    out = np.concatenate([orc.forward(p64, X[s:s + 100], cfg, keep_cache=False)[0] for s in range(0, C * N, 100)])
    return out.reshape(C, N)


# ---- parity against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_sweep_matches_the_oracle(name):
    cfg, C, N = CASES[name]
    eng = engine_of(name)
    assert eng.sweep_ok() and eng.lib.cffm_sweep_ok(eng._s) == 1
    ctx, cand = inputs_of(name, C, N)
    cand[1], cand[N - 1] = -1, cfg.M                                          # clamped: < 0 -> 0, >= M -> M - 1
    for field in (0, cfg.F // 2, cfg.F - 1):
        label = '%s field %d' % (name, field)
        got = sweep_abi(eng, ctx, field, cand, label)
        ref = oracle_scores(name, ctx, field, cand)
        assert np.unique(ref).size > N / 3, '%s: the reference scores hardly depend on the candidate' % label
        rms = float(np.sqrt(np.mean(ref * ref)))
        print('%s: worst err/bound %.3f' % (label, float((np.abs(got - ref) / (T.TOL * (np.abs(ref) + rms))).max())))
        T.close(got.reshape(-1), ref.reshape(-1), 'out')


@pytest.mark.parametrize('name', ['f6-d64-elu', 'f11-relu'])
def test_unserved_shapes_are_refused(name):
    cfg, _ = params_of(name)
    eng = engine_of(name)
    assert not eng.sweep_ok()
    assert eng.lib.cffm_sweep_scratch_bytes(eng._s, 2) < 0
    ctx = dev_of(np.zeros((2, cfg.F), dtype=np.int32))
    cand = dev_of(np.arange(5, dtype=np.int32))
    out, scratch = Guard(2 * 5 * 4), Guard(1024)
    assert eng.lib.cffm_score_sweep(eng._s, eng._t, eng.theta.data_ptr(), ctx.data_ptr(), 2, 0, cand.data_ptr(), 5, out.ptr, 5, scratch.ptr,
                                    stream()) == 10002
    rc.check_untouched(name + ' scores', out.read(name))
    rc.check_untouched(name + ' scratch', scratch.read(name))
    with pytest.raises(ValueError):
        eng.score_candidates_shared(ctx, 0, cand)


# ---- a candidate's score does not depend on where it stands -----------------------------------------------------------------
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('N', [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_scores_do_not_depend_on_the_position(N, C):
    name = 'f3-relu'
    cfg = CASES[name][0]
    eng = engine_of(name)
    ctx, cand = inputs_of(name, C, N, seed=5)
    same = sorted({p for p in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, N - 1) if 0 <= p < N})
    cand[same] = 41
    field = 1
    got = sweep_abi(eng, ctx, field, cand, 'position N=%d C=%d' % (N, C))
    for p in same[1:]:
        rc.check_exact('the same id at positions %d and %d' % (same[0], p), got[:, p], got[:, same[0]])
    again = sweep_abi(eng, ctx, field, cand, 'second call')
    rc.check_exact('second call N=%d C=%d' % (N, C), again, got)
    rev = sweep_abi(eng, ctx, field, cand[::-1].copy(), 'reversed')
    rc.check_exact('reversed candidates N=%d C=%d' % (N, C), rev[:, ::-1], got)
    T.close(got.reshape(-1), oracle_scores(name, ctx, field, cand).reshape(-1), 'out')


# ---- the engine: the shared sweep against the path it replaces ------------------------------------------------------------------
@pytest.mark.parametrize('name', ['f3-relu', 'frappe-selu'])
def test_shared_agrees_with_expand(name):
    cfg, C, N = CASES[name]
    eng = engine_of(name)
    ctx, cand = inputs_of(name, C, N, seed=9)
    cand[0], cand[N // 2] = cfg.M + 7, -3
    for field in (0, cfg.F - 1):
        d_ctx, d_cand = dev_of(ctx), dev_of(cand)
        ref = eng.score_candidates(d_ctx, field, d_cand).cpu().numpy()
        got = eng.score_candidates_shared(d_ctx, field, d_cand)
        assert got.shape == (C, N) and got.dtype == torch.float32
        T.close(got.cpu().numpy().reshape(-1), ref.reshape(-1).astype(np.float64), 'out')
    assert eng.score_candidates_shared(dev_of(ctx[:0]), 0, dev_of(cand)).shape == (0, N)
    for bad in (dict(field=-1), dict(field=cfg.F)):
        with pytest.raises(ValueError):
            eng.score_candidates_shared(dev_of(ctx), bad['field'], dev_of(cand))
    with pytest.raises(ValueError):
        eng.score_candidates_shared(dev_of(ctx[:, :-1]), 0, dev_of(cand))
    with pytest.raises(ValueError):
        eng.score_candidates_shared(dev_of(ctx), 0, dev_of(cand[:0]))


# ---- the class ---------------------------------------------------------------------------------------------------------------------
FIELD = 1


def test_class_sweep_keyword_on_the_frappe_slice(tmp_path, monkeypatch):
    from tests.test_gpu_rank import _frappe_model
    M, m, data = _frappe_model(tmp_path)
    column = lambda split: np.array([r[FIELD] for r in split['X']], dtype=np.int32)
    cand = np.unique(column(data.Train_data))
    ctx = np.asarray(data.Test_data['X'][:6], dtype=np.int32)
    assert m.engine.sweep_ok()
    shared = m.engine.score_candidates_shared(dev_of(ctx), FIELD, dev_of(cand)).cpu().numpy()
    skip = np.random.default_rng(1).random(shared.shape) < 0.2
    for sk in (None, skip):
        ids, val = m.recommend(ctx, FIELD, k=5, skip=sk, sweep='shared')
        ridx, rval, _ = R.topk_ref(shared, 5, sk)                              # the order is defined on the shared scores themselves
        rc.check_exact('recommend ids', ids, cand[ridx])
        rc.check_exact('recommend scores', val.view(np.uint32), rval)
    test = data.Test_data
    got = m.evaluate_ranking(test, FIELD, k=10, sweep='shared')
    assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in got), got
    monkeypatch.setattr(M, 'SWEEP_MIN_N', 1)                                    # every N is above it: 'auto' is 'shared'
    auto = m.evaluate_ranking(test, FIELD, k=10, sweep='auto')
    assert np.array_equal(np.array(got).view(np.uint64), np.array(auto).view(np.uint64)), (got, auto)
    ids_a, val_a = m.recommend(ctx, FIELD, k=5, sweep='auto')
    ids_s, val_s = m.recommend(ctx, FIELD, k=5, sweep='shared')
    rc.check_exact('auto ids', ids_a, ids_s)
    rc.check_exact('auto scores', val_a.view(np.uint32), val_s.view(np.uint32))
    monkeypatch.setattr(M, 'SWEEP_MIN_N', cand.size + 1)                        # below it: 'auto' is the default path, bit for bit
    ids_d, val_d = m.recommend(ctx, FIELD, k=5)
    ids_a, val_a = m.recommend(ctx, FIELD, k=5, sweep='auto')
    rc.check_exact('auto below SWEEP_MIN_N ids', ids_a, ids_d)
    rc.check_exact('auto below SWEEP_MIN_N scores', val_a.view(np.uint32), val_d.view(np.uint32))
    with pytest.raises(ValueError):
        m.recommend(ctx, FIELD, k=5, sweep='fast')


def test_class_auto_is_the_default_at_an_unserved_shape(tmp_path, monkeypatch):
    from cffm_amd import CFFM as M
    monkeypatch.setattr(M, 'SWEEP_MIN_N', 1)
    cfg = UNSERVED['f4-d8']
    m = M.CFFM(cfg.M, 0, str(tmp_path / 'm'), cfg.K, cfg.D, 'square_loss', 1, 8, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer', 0, 0, 0,
               cfg.F, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'relu')
    m.build_graph()
    assert not m.engine.sweep_ok()
    rng = np.random.default_rng(2)
    ctx = rng.integers(0, cfg.M, size=(5, cfg.F)).astype(np.int32)
    cand = np.arange(10, 40, dtype=np.int32)
    ids_d, val_d = m.recommend(ctx, 2, candidates=cand, k=7)
    ids_a, val_a = m.recommend(ctx, 2, candidates=cand, k=7, sweep='auto')
    rc.check_exact('auto ids', ids_a, ids_d)
    rc.check_exact('auto scores', val_a.view(np.uint32), val_d.view(np.uint32))
    with pytest.raises(ValueError, match='shared'):
        m.recommend(ctx, 2, candidates=cand, k=7, sweep='shared')
