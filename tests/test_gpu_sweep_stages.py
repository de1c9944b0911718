"""GPU: the shared candidate sweep (cffm_amd/csrc/sweep.hip) stage by stage, at parameters where every term and every relu is live
(oracle/sweep_check.py; tests/test_sweep_check.py keeps the evidence that these checks see what `out` under close() alone does not).

  a. the per-context block, read from the guarded scratch through cffm_sweep_block_layout, against float64 of its own inputs: Ei and
     fb bit for bit, Zctx / U / V under layer_check.check_tiers with n = the chain the kernel runs, pads exactly 0, s0fix / A / R under
     branch_check.check, the fixed inner sum under branch_check.check_inner; clamped context ids; the unused id of the swept column;
     the exact set of floats the call leaves unwritten;
  b. the scores against score_from_block(the device's own block), against the oracle from the ids, and against the expand path;
  c. the LDS-only intermediates (s0 and the four pools) one t1 row at a time through probe parameters;
  d. more (context, chunk) units than workgroups: 520 units on a grid of 512, bit for bit the rows of calls with at most 200 units.

The cases and their parameters are sweep_check.CASES / make_case (outer rows x 20, inner rows x 4, signed conv biases, every bias
non-zero, beta_outer = 0.7, lamda_att = 1.3); C = 3 contexts and N = 70 candidates (one full chunk and a ragged one) unless said."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cffm_amd import hip  # noqa: E402
from oracle import parity as T  # noqa: E402
from oracle import rows_check as rc  # noqa: E402
from oracle import sweep_check as sc  # noqa: E402
from tests.test_gpu_rows import Guard, dev_of, stream  # noqa: E402

pytestmark = pytest.mark.gpu

GAP, SENTINEL = 5, np.float32(3e38)
WORST = {}                                   # (case, tensor) -> worst |err| / bound of part a., printed by every case


@functools.lru_cache(maxsize=2)
def engine_of(name):
    from cffm_amd.engine import HipEngine
    cfg, p, _, _ = sc.make_case(name)
    return HipEngine(cfg, params=p)


def run_sweep(eng, ctx, field, cand, label, stride=None):
    """cffm_score_sweep (stride None) or cffm_score_sweep_lists (cand [C][stride] flattened) into guarded, gapped rows and a guarded
    scratch -> (scores [C][N], the scratch's floats), after the canaries and the gap behind every row have been checked."""
    C = ctx.shape[0]
    N = cand.size if stride is None else int(stride)
    lib = eng.lib
    nbytes = int(lib.cffm_sweep_scratch_bytes(eng._s, C))
    assert nbytes > 0, label
    scores, scratch = Guard(C * (N + GAP) * 4), Guard(nbytes)
    scores.view().reshape(C, N + GAP)[:, N:] = float(SENTINEL)
    dctx, dcand = dev_of(ctx), dev_of(cand)
    if stride is None:
        rcode = lib.cffm_score_sweep(eng._s, eng._t, eng.theta.data_ptr(), dctx.data_ptr(), C, int(field), dcand.data_ptr(), N, scores.ptr,
                                     N + GAP, scratch.ptr, stream())
    else:
        rcode = lib.cffm_score_sweep_lists(eng._s, eng._t, eng.theta.data_ptr(), dctx.data_ptr(), C, int(field), dcand.data_ptr(), N, N,
                                           scores.ptr, N + GAP, scratch.ptr, stream())
    assert rcode == 0, '%s returned %d' % (label, rcode)
    img = scores.read(label).reshape(C, N + GAP)
    raw = scratch.read(label + ' scratch')
    rc.check_exact(label + ': the gap behind every row', img[:, N:], np.full((C, GAP), SENTINEL, dtype=np.float32))
    got = np.ascontiguousarray(img[:, :N])
    assert not (rc.bits(got) == rc.POISON).any(), '%s: scores left at poison' % label
    return got, raw


def blocks_of(eng, raw, C):
    return sc.cut_blocks(raw, hip.sweep_block_layout(eng.shape), eng.cfg, C)


# ---- a. the block against float64 of its own inputs -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(sc.CASES))
def test_the_block_matches_float64_of_its_inputs(name):
    cfg, p, ctx, cand = sc.make_case(name)
    eng = engine_of(name)
    C = ctx.shape[0]
    for f in sc.fields_of(cfg):
        label = '%s field %d' % (name, f)
        _, raw = run_sweep(eng, ctx, f, cand[:2], label)
        blocks, written = blocks_of(eng, raw, C)
        # every float of every block is written; the header, the unused slots of scal and the tail up to block_floats are not
        left = rc.bits(raw) == rc.POISON
        assert np.array_equal(left, ~written), '%s: %d floats that must be written are poison, %d that must stay poison are not' % (
            label, int((left & written).sum()), int((~left & ~written).sum()))
        sink = {}
        for c in range(C):
            sc.check_block('%s sweep' % name, blocks[c], cfg, p, ctx[c], f, sink=sink)
        for k, v in sink.items():
            WORST[(name, k)] = max(v, WORST.get((name, k), 0.0))
    print('%s: worst |err| / bound  %s' % (name, '  '.join('%s %.3f' % (k, WORST[(name, k)]) for k in ('Z', 'U', 'V', 's0fix', 'A', 'R', 'fixed'))))


def test_context_ids_outside_the_table_are_clamped():
    name = 'F6-K8-selu'
    cfg, p, ctx, cand = sc.make_case(name)
    eng = engine_of(name)
    f = 2
    bad = ctx.copy()
    bad[0, 0], bad[1, 5], bad[2, 3] = -3, cfg.M, cfg.M + 77                      # none in the swept column
    got, raw = run_sweep(eng, bad, f, cand, 'bad ids')
    ref, rraw = run_sweep(eng, sc.clamp_ids(bad, cfg.M).astype(np.int32), f, cand, 'clamped ids')
    rc.check_exact('the scratch under ids outside [0, M) and under the clamped ids', rc.bits(raw), rc.bits(rraw))
    rc.check_exact('the scores under ids outside [0, M) and under the clamped ids', got, ref)
    blocks, _ = blocks_of(eng, raw, 3)
    for c in range(3):
        sc.check_block('%s bad ids' % name, blocks[c], cfg, p, bad[c], f)
        assert np.array_equal(blocks[c]['Ei'], sc.block_ref(cfg, p, sc.clamp_ids(bad[c], cfg.M), f)[0]['Ei'])


def test_the_id_in_the_swept_column_is_never_used():
    name = 'F6-K8-selu'
    cfg, p, ctx, cand = sc.make_case(name)
    eng = engine_of(name)
    f = 3
    first = None
    for v in (0, cfg.M - 1, 2 ** 31 - 1):
        c2 = ctx.copy()
        c2[:, f] = v
        got, raw = run_sweep(eng, c2, f, cand, 'swept column = %d' % v)
        if first is None:
            first = (got, raw)
        rc.check_exact('the scratch with %d in the swept column' % v, rc.bits(raw), rc.bits(first[1]))
        rc.check_exact('the scores with %d in the swept column' % v, got, first[0])


# ---- b. the scores, re-anchored -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(sc.CASES))
def test_the_scores_match_their_block_the_oracle_and_the_expand_path(name):
    cfg, p, ctx, cand = sc.make_case(name)
    eng = engine_of(name)
    C, N = ctx.shape[0], cand.size
    cand = cand.copy()
    cand[1], cand[N - 1] = -1, cfg.M                                             # clamped: < 0 -> 0, >= M -> M - 1
    rows = sc.cand_rows(cfg, p, cand)
    for f in sc.fields_of(cfg):
        label = '%s field %d' % (name, f)
        got, raw = run_sweep(eng, ctx, f, cand, label)
        blocks, _ = blocks_of(eng, raw, C)
        anchored = np.stack([sc.score_from_block(cfg, p, blocks[c], rows, f)[0] for c in range(C)])
        ref = sc.oracle_scores(cfg, p, ctx, f, cand)
        assert np.unique(ref).size > N / 3, '%s: the reference scores hardly depend on the candidate' % label
        rms = float(np.sqrt(np.mean(ref * ref)))
        print('%s: worst err/bound %.3f from its block, %.3f from the ids' % (
            label, float((np.abs(got - anchored) / (T.TOL * (np.abs(anchored) + float(np.sqrt(np.mean(anchored ** 2)))))).max()),
            float((np.abs(got - ref) / (T.TOL * (np.abs(ref) + rms))).max())))
        T.close(got.reshape(-1), anchored.reshape(-1), 'sweep out from its own block')
        T.close(got.reshape(-1), ref.reshape(-1), 'out')
        expand = eng.score_candidates(dev_of(ctx), f, dev_of(cand)).cpu().numpy()
        T.close(got.reshape(-1), expand.reshape(-1).astype(np.float64), 'sweep out against the expand path')


# ---- c. the LDS-only intermediates through probe parameters -------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['F3-K8-relu', 'F10-K32-selu'])
def test_probes_of_s0_and_the_pools(name):
    from cffm_amd.engine import HipEngine
    cfg, p, ctx, cand = sc.make_case(name)
    C, N = ctx.shape[0], cand.size
    f = cfg.F // 2
    pcfg, q = sc.probe_params(cfg, p, 0)
    rows = sc.cand_rows(pcfg, q, cand)
    eng = HipEngine(pcfg, params=q)
    first, t1 = None, None
    for k in sc.PROBE_ROWS:
        pcfg, q = sc.probe_params(cfg, p, k)
        eng.load_params(q)
        label = '%s probe of t1[%d]' % (name, k)
        got, raw = run_sweep(eng, ctx, f, cand, label)
        if first is None:                        # the block does not depend on the dense parameters the probes differ in
            first = raw
            blocks, _ = blocks_of(eng, raw, C)
            t1 = np.stack([sc.score_from_block(pcfg, q, blocks[c], rows, f)[1]['t1'] for c in range(C)])
        rc.check_exact(label + ': the scratch of the first probe', rc.bits(raw), rc.bits(first))
        ref = t1[:, :, k]
        for c in range(C):
            assert np.unique(ref[c]).size >= N / 3, '%s: a broken probe, its column hardly depends on the candidate' % label
        print('%s: worst err/bound %.3f' % (label, float((np.abs(got - ref) / (T.TOL * (np.abs(ref) + float(np.sqrt(np.mean(ref * ref)))))).max())))
        T.close(got.reshape(-1), ref.reshape(-1), 'sweep t1 probe')


# ---- d. more units than workgroups -------------------------------------------------------------------------------------------------
def test_more_units_than_workgroups():
    name = 'F3-K8-relu'
    cfg, p, _, _ = sc.make_case(name)
    eng = engine_of(name)
    C, N, f = 260, 65, 1                                                         # two chunks per context, the second ragged: 520 units
    assert C * ((N + hip.SWEEP_CHUNK - 1) // hip.SWEEP_CHUNK) > 512
    rng = np.random.default_rng(5)
    ctx = rng.integers(0, cfg.M, size=(C, cfg.F)).astype(np.int32)
    cand = rng.integers(0, cfg.M, size=N).astype(np.int32)
    got, _ = run_sweep(eng, ctx, f, cand, 'C = 260')
    parts = np.concatenate([run_sweep(eng, ctx[s:s + 100], f, cand, 'contexts %d..' % s)[0] for s in range(0, C, 100)])
    rc.check_exact('520 units on 512 workgroups against calls of at most 200 units', got, parts)
    T.close(got.reshape(-1), sc.oracle_scores(cfg, p, ctx, f, cand).reshape(-1), 'out')
    lists = rng.integers(0, cfg.M, size=(C, N)).astype(np.int32)                 # a list of its own for every context
    assert np.unique(lists, axis=0).shape[0] == C
    gl, _ = run_sweep(eng, ctx, f, lists.reshape(-1), 'lists, C = 260', stride=N)
    single = np.concatenate([run_sweep(eng, ctx[c:c + 1], f, lists[c], 'context %d alone' % c)[0] for c in range(C)])
    rc.check_exact('per-context lists, 520 units, against single-context calls', gl, single)
