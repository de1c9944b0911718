"""GPU: the shared sweep for candidates that are tuples of nf ids (cffm_score_sweep_tuples, cffm_amd/csrc/sweep.hip).

  1. the scores against the float64 oracle on the numpy-expanded id rows and against the expand path (score_candidate_tuples), both
     under oracle.parity.close(got, ref, 'out') at its default tolerance - the criterion tests/test_sweep_tuples_ref.py shows to fail
     on a dropped swept-swept pair, swapped slots, a swept row left in U_a and A_a summed over a swept field, on these inputs;
  2. bit for bit: nf = 1 against cffm_score_sweep_lists; the caller's field order; a tuple at every position, in every chunk, under
     a shared list and under its own, on a second call; more (context, chunk) units than the grid;
  3. the per-context block, read through cffm_sweep_tuples_block_layout, against tests/_sweep_tuples_ref.py: Ei / fb exact, pad
     channels exactly 0, Zctx / U_a / V_a under the hard tier of oracle/layer_check with the chain lengths the kernel runs, the
     floats the call leaves unwritten;
  4. the same bits on a scratch dirtied with NaN, with 3.39e38 and by a call at another nf and another C;
  5. an unserved (shape, nf): CFFM_ERR_UNSUPPORTED with the guarded outputs untouched;
  6. the class on the committed frappe slice with sweep='tuples'.

Harness of tests/test_gpu_sweep.py: the scores and the scratch of every ABI call are Guards (canaries on both sides, a NaN poison
payload); the scores lie in rows of N + 5 floats whose gap holds 3e38, which must survive.  Cases: tests/_sweep_tuples_cases.py."""
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
from oracle import layer_check as lc  # noqa: E402
from oracle import parity as T  # noqa: E402
from oracle import rows_check as rc  # noqa: E402
from tests import _rank_ref as R  # noqa: E402
from tests import _sweep_tuples_cases as CS  # noqa: E402
from tests import _sweep_tuples_ref as TR  # noqa: E402
from tests.test_gpu_rows import Guard, dev_of, stream  # noqa: E402

pytestmark = pytest.mark.gpu

GAP, SENTINEL = 5, np.float32(3e38)
CHUNK = hip.SWEEP_CHUNK
UNSUPPORTED = 10002


@functools.lru_cache(maxsize=2)
def engine_of(name):
    from cffm_amd.engine import HipEngine
    cfg, p = CS.shape_of(name)
    return HipEngine(cfg, params=p)


def host_fields(fields):
    return (ctypes.c_int32 * len(fields))(*fields)


def run_tuples(eng, ctx, fields, cand, label, scratch=None, want=0):
    """cffm_score_sweep_tuples for cand [N][nf] (one list, stride 0) or [C][N][nf] (stride N * nf) into guarded, gapped rows and a
    guarded scratch (a fresh poisoned one unless given) -> (scores [C][N], the scratch's floats), canaries and gaps checked."""
    C, N, nf = ctx.shape[0], cand.shape[-2], len(fields)
    assert cand.shape[-1] == nf
    lib = eng.lib
    nbytes = int(lib.cffm_sweep_tuples_scratch_bytes(eng._s, nf, C))
    assert nbytes > 0, label
    scores = Guard(C * (N + GAP) * 4)
    scratch = Guard(nbytes) if scratch is None else scratch
    assert scratch.nbytes >= nbytes
    scores.view().reshape(C, N + GAP)[:, N:] = float(SENTINEL)
    dctx, dcand, hf = dev_of(ctx), dev_of(cand), host_fields(fields)
    rcode = lib.cffm_score_sweep_tuples(eng._s, eng._t, eng.theta.data_ptr(), dctx.data_ptr(), C, ctypes.addressof(hf), nf, dcand.data_ptr(),
                                        N * nf if cand.ndim == 3 else 0, N, scores.ptr, N + GAP, scratch.ptr, stream())
    assert rcode == want, '%s returned %d' % (label, rcode)
    img = scores.read(label).reshape(C, N + GAP)
    raw = scratch.read(label + ' scratch')
    rc.check_exact(label + ': the gap behind every row', img[:, N:], np.full((C, GAP), SENTINEL, dtype=np.float32))
    got = np.ascontiguousarray(img[:, :N])
    if want == 0:
        assert not (rc.bits(got) == rc.POISON).any(), '%s: scores left at poison' % label
    return got, raw


def ratio(got, ref):
    ref = np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (T.TOL * (np.abs(ref) + float(np.sqrt(np.mean(ref * ref)))))).max())


@functools.lru_cache(maxsize=None)
def reference(name, fields):
    """(ctx, cand, the float64 oracle's scores) of a case: computed once, shared, read-only."""
    cfg, p = CS.shape_of(name)
    ctx, cand = CS.inputs_of(name, fields)
    ref = TR.oracle_scores(cfg, p, ctx, fields, cand)
    ref.setflags(write=False)
    return ctx, cand, ref


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,fields', CS.CASES, ids=CS.CASE_IDS)
def test_scores_match_the_oracle_and_the_expand_path(name, fields):
    cfg, p = CS.shape_of(name)
    eng = engine_of(name)
    nf = len(fields)
    assert eng.sweep_tuples_ok(nf) and eng.lib.cffm_sweep_tuples_ok(eng._s, nf) == 1
    ctx, cand, ref = reference(name, fields)
    N = cand.shape[0]
    label = '%s fields %s' % (name, fields)
    got, _ = run_tuples(eng, ctx, fields, cand, label)
    for c in range(ctx.shape[0]):
        assert np.unique(ref[c]).size > N / 3, '%s: the reference scores hardly depend on the tuple' % label
    expand = eng.score_candidate_tuples(dev_of(ctx), list(fields), dev_of(cand)).cpu().numpy()
    print('%s: worst err/bound %.3f against the oracle, %.3f against the expand path' % (label, ratio(got, ref), ratio(got, expand)))
    T.close(got.reshape(-1), ref.reshape(-1), 'out')
    T.close(got.reshape(-1), expand.reshape(-1).astype(np.float64), 'out')
    # the engine method: the same call, the same bits; a list per context
    shared = eng.score_candidate_tuples_shared(dev_of(ctx), list(fields), dev_of(cand))
    assert shared.shape == got.shape and shared.dtype == torch.float32
    rc.check_exact(label + ': score_candidate_tuples_shared', shared.cpu().numpy(), got)
    ctx2, lists = CS.inputs_of(name, fields, N=9, per_context=True, seed=3)
    gl = eng.score_candidate_tuples_shared(dev_of(ctx2), list(fields), dev_of(lists)).cpu().numpy()
    T.close(gl.reshape(-1), TR.oracle_scores(cfg, p, ctx2, fields, lists).reshape(-1), 'out')
    assert eng.score_candidate_tuples_shared(dev_of(ctx[:0]), list(fields), dev_of(cand)).shape == (0, N)


# ---- 2. bit for bit -------------------------------------------------------------------------------------------------------------------
def test_one_field_is_the_single_field_sweep():
    name = 'F7-gelu'
    cfg, _ = CS.shape_of(name)
    eng = engine_of(name)
    ctx, lists = CS.inputs_of(name, (3,), N=CHUNK + 6, per_context=True, seed=2)
    C, N = lists.shape[:2]
    for f in (0, 3, cfg.F - 1):
        got, raw = run_tuples(eng, ctx, (f,), lists, 'nf = 1 field %d' % f)
        out, scratch = Guard(C * N * 4), Guard(int(eng.lib.cffm_sweep_scratch_bytes(eng._s, C)))
        assert eng.lib.cffm_score_sweep_lists(eng._s, eng._t, eng.theta.data_ptr(), dev_of(ctx).data_ptr(), C, f, dev_of(lists).data_ptr(), N, N,
                                              out.ptr, N, scratch.ptr, stream()) == 0
        rc.check_exact('nf = 1 against cffm_score_sweep_lists, field %d' % f, got, out.read('lists').reshape(C, N))
        rc.check_exact('nf = 1: the scratch of cffm_score_sweep_lists', rc.bits(raw), rc.bits(scratch.read('lists scratch')))
        one, _ = run_tuples(eng, ctx, (f,), lists[0], 'nf = 1 shared list')
        single = eng.score_candidates_shared(dev_of(ctx), f, dev_of(lists[0, :, 0])).cpu().numpy()
        rc.check_exact('nf = 1 against cffm_score_sweep, field %d' % f, one, single)


@pytest.mark.parametrize('name,fields', [('frappe', (6, 1)), ('F8-K16-prelu-noatt', (7, 0, 3)), ('F6-K8-elu', (3, 1, 4, 2))], ids=['frappe', 'F8', 'F6'])
def test_the_callers_field_order_never_reaches_the_arithmetic(name, fields):
    eng = engine_of(name)
    ctx, cand = CS.inputs_of(name, fields, N=CHUNK + 3, seed=4)
    got, raw = run_tuples(eng, ctx, fields, cand, 'fields %s' % (fields,))
    order = sorted(range(len(fields)), key=lambda a: fields[a])
    srt = tuple(fields[a] for a in order)
    again, raw2 = run_tuples(eng, ctx, srt, np.ascontiguousarray(cand[:, order]), 'fields %s' % (srt,))
    rc.check_exact('fields %s with the columns permuted against %s' % (fields, srt), got, again)
    rc.check_exact('the scratch of both', rc.bits(raw), rc.bits(raw2))


@pytest.mark.parametrize('N', [1, CHUNK - 1, CHUNK, CHUNK + 1, 70, 300])
def test_a_tuple_scores_the_same_everywhere(N):
    name, fields = 'F3', (0, 2)
    cfg, p = CS.shape_of(name)
    eng = engine_of(name)
    C = 3
    ctx, cand = CS.inputs_of(name, fields, N=N, C=C, seed=5)
    same = sorted({q for q in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 4 * CHUNK + 5, N - 1) if 0 <= q < N})
    cand[same] = (41, 17)
    got, _ = run_tuples(eng, ctx, fields, cand, 'N=%d' % N)
    for q in same[1:]:
        rc.check_exact('the same tuple at positions %d and %d' % (same[0], q), got[:, q], got[:, same[0]])
    again, _ = run_tuples(eng, ctx, fields, cand, 'second call')
    rc.check_exact('second call N=%d' % N, again, got)
    rev, _ = run_tuples(eng, ctx, fields, cand[::-1].copy(), 'reversed')
    rc.check_exact('reversed candidates N=%d' % N, rev[:, ::-1], got)
    # under a list of its own: context c's list is the shared one rotated by c
    lists = np.stack([np.roll(cand, c, axis=0) for c in range(C)])
    own, _ = run_tuples(eng, ctx, fields, lists, 'own lists')
    rc.check_exact('own lists against the shared list N=%d' % N, np.stack([np.roll(own[c], -c) for c in range(C)]), got)
    T.close(got.reshape(-1), TR.oracle_scores(cfg, p, ctx, fields, cand).reshape(-1), 'out')


def test_more_units_than_workgroups():
    name, fields = 'F3', (2, 0)
    cfg, p = CS.shape_of(name)
    eng = engine_of(name)
    C, N = 260, CHUNK + 1                                                        # two chunks per context, the second ragged: 520 units
    assert C * ((N + CHUNK - 1) // CHUNK) > 512
    ctx, lists = CS.inputs_of(name, fields, N=N, C=C, per_context=True, seed=6)
    got, _ = run_tuples(eng, ctx, fields, lists, 'C = 260')
    parts = np.concatenate([run_tuples(eng, ctx[s:s + 100], fields, lists[s:s + 100], 'contexts %d..' % s)[0] for s in range(0, C, 100)])
    rc.check_exact('520 units on 512 workgroups against calls of at most 200 units', got, parts)
    T.close(got[:4].reshape(-1), TR.oracle_scores(cfg, p, ctx[:4], fields, lists[:4]).reshape(-1), 'out')


# ---- 3. the block ---------------------------------------------------------------------------------------------------------------------
def cut_blocks(raw, bl, cfg, C, nf):
    """The C blocks of a scratch image -> (list of dicts, a bool mask over raw of the floats the context kernel is specified to write)."""
    F, K = cfg.F, cfg.K
    H, n, Pp = int(bl.header_floats), int(bl.block_floats), int(bl.UV_stride) // 32
    assert raw.size == H + C * n and Pp % 16 == 0 and Pp >= cfg.P and int(bl.A_stride) == 32
    written = np.zeros(raw.size, bool)
    out = []
    parts = {'Z': (bl.Z, (16, 16, Pp)), 'U': (bl.U, (nf, 2, 16, Pp)), 'V': (bl.V, (nf, 2, 16, Pp)), 'Ei': (bl.Ei, (F, K)), 's0fix': (bl.s0fix, (32,)),
             'A': (bl.A, (nf, 32)), 'fb': (bl.fb, (16,)), 'fixed': (bl.scal, ()), 'R': (bl.scal + 1, (nf,))}
    for c in range(C):
        b, w, d = raw[H + c * n:H + (c + 1) * n], written[H + c * n:H + (c + 1) * n], {}
        for k, (off, shp) in parts.items():
            cnt = int(np.prod(shp)) if shp else 1
            d[k] = b[int(off):int(off) + cnt].reshape(shp).copy()
            w[int(off):int(off) + cnt] = True
        out.append(d)
    return out, written


@pytest.mark.parametrize('name,fields', CS.CASES, ids=CS.CASE_IDS)
def test_the_block_matches_float64_of_its_inputs(name, fields):
    from oracle import branch_check as bc
    cfg, p = CS.shape_of(name)
    eng = engine_of(name)
    nf, P = len(fields), cfg.P
    ctx, cand, _ = reference(name, fields)
    srt, order = TR.split_columns(fields)
    C = ctx.shape[0]
    label = '%s fields %s' % (name, fields)
    got, raw = run_tuples(eng, ctx, fields, cand[:3], label)
    bl = hip.sweep_tuples_block_layout(eng.shape, nf)
    blocks, written = cut_blocks(raw, bl, cfg, C, nf)
    left = rc.bits(raw) == rc.POISON
    assert np.array_equal(left, ~written), '%s: %d floats that must be written are poison, %d that must stay poison are not' % (
        label, int((left & written).sum()), int((~left & ~written).sum()))
    n = TR.chain_lengths(cfg, srt)
    worst = {}
    for c in range(C):
        ref, S = TR.block_ref(cfg, p, ctx[c], srt, Pp=blocks[c]['Z'].shape[-1])
        for k in ('Ei', 'fb'):
            rc.check_exact('%s context %d %s' % (label, c, k), rc.bits(blocks[c][k]), rc.bits(ref[k]))
        for k in ('Z', 'U', 'V'):
            assert (blocks[c][k][..., P:] == 0).all(), '%s %s: non-zero pad channels' % (label, k)
            for a in range(nf if k != 'Z' else 1):
                g, r, s = (blocks[c][k], ref[k], S[k]) if k == 'Z' else (blocks[c][k][a], ref[k][a], S[k][a])
                nk = n[k] if k != 'U' else n[k][a]
                st = lc.check_tiers('%s %s[%d]' % (label, k, a), torch.from_numpy(g[..., :P].copy()), torch.from_numpy(r[..., :P].copy()),
                                    torch.from_numpy(s[..., :P].copy()), nk, bias=False)
                bound = (nk + 2) * lc.U * s[..., :P]
                err = np.abs(g[..., :P].astype(np.float64) - r[..., :P])
                worst[k] = max(worst.get(k, 0.0), float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf)).max()))
        for k in ('s0fix', 'A', 'R'):
            worst[k] = max(worst.get(k, 0.0), bc.check('%s %s' % (label, k), blocks[c][k], ref[k], S[k], n[k], 1)['hard'])
        # the scores from the device's own block
        anchored = TR.score_from_block(cfg, p, blocks[c], TR.tuple_rows(cfg, p, cand[:3], srt, order), srt)
        T.close(got[c], anchored, 'sweep out from its own block')
    print('%s: worst |err| / bound  %s' % (label, '  '.join('%s %.3f' % kv for kv in sorted(worst.items()))))


# ---- 4. a dirty scratch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,fields,other', [('frappe', (1, 6), (4,)), ('F8-K16-prelu-noatt', (0, 3, 7), (2, 5))], ids=['frappe', 'F8'])
def test_a_dirty_scratch_changes_no_bit(name, fields, other):
    eng = engine_of(name)
    nf = len(fields)
    ctx, cand, _ = reference(name, fields)
    C = ctx.shape[0]
    clean, _ = run_tuples(eng, ctx, fields, cand, 'clean')
    big = max(int(eng.lib.cffm_sweep_tuples_scratch_bytes(eng._s, nf, C)), int(eng.lib.cffm_sweep_tuples_scratch_bytes(eng._s, len(other), C + 3)))
    for what, fill in (('NaN', float('nan')), ('3.39e38', 3.39e38)):
        scratch = Guard(big)
        scratch.view().fill_(fill)
        got, _ = run_tuples(eng, ctx, fields, cand, 'scratch full of %s' % what, scratch=scratch)
        rc.check_exact('scores on a scratch full of %s' % what, got, clean)
    scratch = Guard(big)                                                         # the leftovers of a call at another nf and another C
    ctx2, cand2 = CS.inputs_of(name, other, N=9, C=C + 3, seed=8)
    run_tuples(eng, ctx2, other, cand2, 'the call before', scratch=scratch)
    got, _ = run_tuples(eng, ctx, fields, cand, 'after a call at nf = %d, C = %d' % (len(other), C + 3), scratch=scratch)
    rc.check_exact('scores on the leftovers of another call', got, clean)


# ---- 5. what is not served --------------------------------------------------------------------------------------------------------------
def test_unserved_is_refused_with_the_outputs_untouched():
    eng = engine_of('frappe')
    ctx, _ = CS.inputs_of('frappe', (1, 6), N=5)
    C = ctx.shape[0]
    for fields in ((1, 6, 8, 9), (0, 1, 2, 3, 4), (1, 6, 8)):
        nf = len(fields)
        served = eng.lib.cffm_sweep_tuples_ok(eng._s, nf) == 1
        assert served == eng.sweep_tuples_ok(nf) and (int(eng.lib.cffm_sweep_tuples_scratch_bytes(eng._s, nf, C)) > 0) == served
        cand = np.arange(5 * nf, dtype=np.int32).reshape(5, nf)
        if served:                                                               # the call agrees with the query, whichever way it answers
            got, _ = run_tuples(eng, ctx, fields, cand, 'nf = %d' % nf)
            cfg, p = CS.shape_of('frappe')
            T.close(got.reshape(-1), TR.oracle_scores(cfg, p, ctx, fields, cand).reshape(-1), 'out')
            continue
        out, scratch, hf = Guard(C * 5 * 4), Guard(4096), host_fields(fields)
        assert eng.lib.cffm_score_sweep_tuples(eng._s, eng._t, eng.theta.data_ptr(), dev_of(ctx).data_ptr(), C, ctypes.addressof(hf), nf,
                                               dev_of(cand).data_ptr(), 0, 5, out.ptr, 5, scratch.ptr, stream()) == UNSUPPORTED
        rc.check_untouched('nf = %d scores' % nf, out.read('scores'))
        rc.check_untouched('nf = %d scratch' % nf, scratch.read('scratch'))
        with pytest.raises(ValueError):
            eng.score_candidate_tuples_shared(dev_of(ctx), list(fields), dev_of(cand))
    assert not eng.sweep_tuples_ok(4) and not eng.sweep_tuples_ok(5)


# ---- 6. the class -----------------------------------------------------------------------------------------------------------------------
def test_class_sweep_tuples_on_the_frappe_slice(tmp_path):
    from tests.test_gpu_rank import _frappe_model
    M, m, data = _frappe_model(tmp_path)
    fields = (1, 6)
    rows = lambda split: np.asarray(split['X'], dtype=np.int32)[:, list(fields)]
    cand = np.unique(np.concatenate([rows(data.Train_data), rows(data.Test_data)]), axis=0)
    ctx = np.asarray(data.Test_data['X'][:6], dtype=np.int32)
    assert m.engine.sweep_tuples_ok(2)
    scores = m.engine.score_candidate_tuples_shared(dev_of(ctx), list(fields), dev_of(cand)).cpu().numpy()
    skip = np.random.default_rng(1).random(scores.shape) < 0.2
    for sk in (None, skip):
        pos, val = m.recommend_tuples(ctx, fields, cand, k=5, skip=sk, sweep='tuples')
        ridx, rval, _ = R.topk_ref(scores, 5, sk)                                # the order is defined on the engine's scores themselves
        rc.check_exact('recommend_tuples positions', pos, ridx)
        rc.check_exact('recommend_tuples scores', val.view(np.uint32), rval)
    # the sampled protocol: the host formula on the ranks of the scores the engine method returns for the same lists
    test = data.Test_data
    seen = []
    inner = m.engine.score_candidate_tuples_shared

    def spy(c, f, l):
        out = inner(c, f, l)
        seen.append((c.cpu().numpy(), l.cpu().numpy(), out.cpu().numpy()))
        return out
    m.engine.score_candidate_tuples_shared = spy
    try:
        got = m.evaluate_ranking_tuples(test, fields, k=10, negatives=20, seed=3, sweep='tuples')
    finally:
        del m.engine.score_candidate_tuples_shared
    ctx_all = np.concatenate([s[0] for s in seen])
    lists, sc_all = np.concatenate([s[1] for s in seen]), np.concatenate([s[2] for s in seen])
    assert lists.ndim == 3 and lists.shape[1:] == (21, 2)
    place = (lists == ctx_all[:, None, list(fields)]).all(axis=2).argmax(axis=1)
    want = M.ranking_metrics(R.rank_ref(sc_all, place), 10)
    assert got == pytest.approx(want, abs=1e-12), (got, want)
    with pytest.raises(ValueError, match="'tuples'"):
        m.recommend_tuples(ctx, (1, 6, 8, 9), np.zeros((3, 4), dtype=np.int32), sweep='tuples')
