"""The evidence behind oracle/sweep_check.py (CPU only), as tests/test_layer_check.py keeps it for the conv tiers:

  * the reference is the model: score_from_block(block_ref(...)) is cffm_oracle.forward on the numpy-expanded rows to 1e-12;
  * every GPU case of tests/test_gpu_sweep_stages.py meets, from the float64 reference alone, the conditions that keep it from hiding a
    failure (every relu switches, no dead or always-on channels beyond a tenth, an unsaturated sigmoid);
  * the bounds of the block check pass a float32 numpy stand-in of the block in the kernel's factorised order and fail every mutant of
    block_ref; every mutant of score_from_block fails parity.close() against the unmutated scores at the named cases."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cffm_amd.spec import ACTIVATIONS, CFFMConfig  # noqa: E402
from oracle import parity as T  # noqa: E402
from oracle import sweep_check as sc  # noqa: E402


# ---- the reference is the model ---------------------------------------------------------------------------------------------------
def _model_case(F):
    """One configuration per F in 2..10; together: the five activations, linear_att 0 and 1, K in {4, 32, 64}, both score forms."""
    return dict(F=F, act=ACTIVATIONS[(F - 2) % 5], att=F % 2, K=(4, 32, 64)[F % 3], loss='log_loss' if F % 4 == 1 else 'square_loss')


def test_the_model_cases_cover_the_domain():
    cs = [_model_case(F) for F in range(2, 11)]
    assert {c['act'] for c in cs} == set(ACTIVATIONS) and {c['att'] for c in cs} == {0, 1} and {c['K'] for c in cs} == {4, 32, 64}
    assert {c['loss'] for c in cs} == {'log_loss', 'square_loss'}


@pytest.mark.parametrize('F', range(2, 11))
def test_the_reference_is_the_model(F):
    c = _model_case(F)
    cfg = CFFMConfig(M=40, F=F, K=c['K'], D=32, activation=c['act'], linear_att=c['att'], loss_type=c['loss'], beta_outer=0.7, lamda_att=1.3)
    p = sc.make_params(cfg, seed=F, log_scale=(1.0, 0.01) if c['loss'] == 'log_loss' else None)
    rng = np.random.default_rng(F)
    ctx = rng.integers(-2, cfg.M + 2, size=(2, F)).astype(np.int32)                 # a few ids outside [0, M): clamped
    cand = rng.integers(-2, cfg.M + 2, size=5).astype(np.int32)
    rows = sc.cand_rows(cfg, p, cand)
    for f in sc.fields_of(cfg):
        ref = sc.oracle_scores(cfg, p, ctx, f, cand)
        for ci in range(2):
            blk, _ = sc.block_ref(cfg, p, ctx[ci], f)
            got, d = sc.score_from_block(cfg, p, blk, rows, f)
            scale = np.abs(ref[ci]) + np.sqrt(np.mean(ref[ci] ** 2))
            assert (np.abs(got - ref[ci]) <= 1e-12 * scale).all(), (F, f, ci, float((np.abs(got - ref[ci]) / scale).max()))
            assert d['t1'].shape == (5, 62) and [r.shape[1] for r in d['relu']] == [16, 8, 4, 2]


# ---- the conditions ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_scores(name, fault=None):
    """Every (field, context) of a named case through block_ref and score_from_block -> scores [fields][C][N] and, unmutated, the
    relu outputs per layer and the raw scores over all rows."""
    cfg, p, ctx, cand = sc.make_case(name)
    rows = sc.cand_rows(cfg, p, cand)
    outs, relus, raws = [], [[] for _ in range(4)], []
    for f in sc.fields_of(cfg):
        for ci in range(ctx.shape[0]):
            blk, _ = sc.block_ref(cfg, p, ctx[ci], f)
            out, d = sc.score_from_block(cfg, p, blk, rows, f, fault=fault)
            outs.append(out)
            if fault is None:
                raws.append(d['raw'])
                for l in range(4):
                    relus[l].append(d['relu'][l])
    if fault is not None:
        return np.concatenate(outs), None, None
    return np.concatenate(outs), [np.concatenate(r) for r in relus], np.concatenate(raws)


@pytest.mark.parametrize('name', list(sc.CASES))
def test_the_gpu_cases_meet_the_conditions(name):
    cfg = sc.make_case(name)[0]
    _, relus, raw = case_scores(name)
    figs = sc.conditions(relus, raw, cfg.loss_type == 'log_loss')
    print(name, figs)


def test_the_cases_are_the_ones_the_gpu_file_runs():
    shapes = {(c['F'], c['K'], c['act'], c.get('loss', 'square_loss')) for c in sc.CASES.values()}
    want = {(2, 4, 'relu'), (3, 8, 'relu'), (4, 8, 'prelu'), (5, 16, 'elu'), (6, 8, 'selu'), (9, 8, 'gelu'), (10, 32, 'selu'), (10, 64, 'relu')}
    assert {s[:3] for s in shapes if s[3] == 'square_loss'} == want
    assert {s[:3] for s in shapes if s[3] == 'log_loss'} == {(3, 8, 'relu'), (6, 8, 'selu'), (10, 32, 'selu')}
    assert sc.CASES['F4-K8-prelu-noatt']['linear_att'] == 0 and sc.CASES['F10-K32-selu']['M'] == 5382
    for name in sc.CASES:
        cfg, p, _, _ = sc.make_case(name)
        assert cfg.beta_outer == 0.7 and cfg.lamda_att == 1.3
        for k in ('dense_bias', 'dense_1_bias', 'dense_2_bias', 'dense_3_bias', 'bias'):
            assert np.all(np.asarray(p[k]) != 0), (name, k)
        signs = {float(np.sign(np.asarray(p[k]).reshape(-1)[0])) for k in ('dense_bias', 'dense_2_bias', 'dense_3_bias', 'bias')}
        assert signs == {-1.0, 1.0} and (p['dense_1_bias'] > 0).any() and (p['dense_1_bias'] < 0).any()


# ---- the block bounds: a float32 stand-in passes, every mutant fails -----------------------------------------------------------------
BLOCK_CASES = ('F3-K8-relu', 'F9-K8-gelu', 'F10-K32-selu')              # the three kernel instances (Pp = 16, 48, 48), f in the middle


def _as_device(blk):
    return {k: np.asarray(v, np.float32) for k, v in blk.items()}


@pytest.mark.parametrize('name', BLOCK_CASES)
def test_block_bounds_pass_a_float32_standin(name):
    cfg, p, ctx, _ = sc.make_case(name)
    Pp = (cfg.P + 15) // 16 * 16
    for f in sc.fields_of(cfg):
        worst = sc.check_block('%s f=%d float32 stand-in' % (name, f), sc.block_f32(cfg, p, ctx[0], f, Pp=Pp), cfg, p, ctx[0], f)
        assert max(worst.values()) <= 1.0
        sc.check_block('%s f=%d rounded reference' % (name, f), _as_device(sc.block_ref(cfg, p, ctx[0], f, Pp=Pp)[0]), cfg, p, ctx[0], f)


@pytest.mark.parametrize('fault', sc.BLOCK_FAULTS)
@pytest.mark.parametrize('name', BLOCK_CASES)
def test_block_bounds_fail_every_mutant(name, fault):
    cfg, p, ctx, _ = sc.make_case(name)
    Pp = (cfg.P + 15) // 16 * 16
    f = cfg.F // 2
    mutant = _as_device(sc.block_ref(cfg, p, ctx[0], f, fault=fault, Pp=Pp)[0])
    with pytest.raises(AssertionError) as e:
        sc.check_block('%s %s' % (name, fault), mutant, cfg, p, ctx[0], f)
    print(str(e.value)[:300])


def test_block_bounds_see_bits_of_the_copies():
    cfg, p, ctx, _ = sc.make_case('F3-K8-relu')
    blk = _as_device(sc.block_ref(cfg, p, ctx[0], 1, Pp=16)[0])
    for k, at in (('Ei', (0, 3)), ('fb', (2,))):
        bad = dict(blk)
        bad[k] = blk[k].copy()
        bad[k][at] = np.nextafter(bad[k][at], np.float32(9))
        with pytest.raises(AssertionError, match='bits'):
            sc.check_block('one ulp in ' + k, bad, cfg, p, ctx[0], 1)


# ---- the score mutants: close() sees each at the new parameters ---------------------------------------------------------------------
# fault -> the named cases at which it must fail close() against the unmutated scores
SEEN_AT = {f: ('F3-K8-relu', 'F6-K8-selu-log') for f in sc.SCORE_FAULTS}
SEEN_AT['no_relu0'] = ('F6-K8-selu', 'F10-K32-selu', 'F6-K8-selu-log')       # act(relu(z)) == act(z) only where act is relu itself
SEEN_AT['no_sigmoid'] = ('F3-K8-relu-log', 'F6-K8-selu-log', 'F10-K32-selu-log')


@pytest.mark.parametrize('fault', sc.SCORE_FAULTS)
def test_close_sees_every_score_mutant(fault):
    for name in SEEN_AT[fault]:
        base = case_scores(name)[0]
        mut = case_scores(name, fault)[0]
        with pytest.raises(AssertionError):
            T.close(mut, base, 'mutant ' + fault)
        rms = float(np.sqrt(np.mean(base * base)))
        print('%s at %s: worst err/bound %.3g' % (fault, name, float((np.abs(mut - base) / (T.TOL * (np.abs(base) + rms))).max())))


def test_unmutated_scores_pass_close_against_the_oracle():
    for name in ('F3-K8-relu', 'F6-K8-selu-log'):
        cfg, p, ctx, cand = sc.make_case(name)
        ref = np.concatenate([sc.oracle_scores(cfg, p, ctx, f, cand).reshape(-1) for f in sc.fields_of(cfg)])
        T.close(case_scores(name)[0], ref, 'reference scores')


# ---- the probes and the scratch reader -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['F3-K8-relu', 'F10-K32-selu'])
def test_a_probe_isolates_one_row_of_t1(name):
    cfg, p, ctx, cand = sc.make_case(name)
    f = cfg.F // 2
    rows = sc.cand_rows(cfg, p, cand)
    _, d0 = sc.score_from_block(cfg, p, sc.block_ref(cfg, p, ctx[0], f)[0], rows, f)
    for k in sc.PROBE_ROWS:
        pcfg, q = sc.probe_params(cfg, p, k)
        assert pcfg.beta_outer == 1.0 and pcfg.lamda_att == cfg.lamda_att
        out, d = sc.score_from_block(pcfg, q, sc.block_ref(pcfg, q, ctx[0], f)[0], sc.cand_rows(pcfg, q, cand), f)
        assert np.array_equal(d['t1'], d0['t1'])                                   # the tables and the conv stack are the case's
        assert np.abs(out - d0['t1'][:, k]).max() <= 1e-13 * np.abs(d0['t1'][:, k]).max(), k
        assert np.unique(out).size >= cand.size / 3, k
    assert sc.PROBE_ROWS == (0, 31, 32, 47, 48, 55, 56, 59, 60, 61)


def test_cut_blocks_reads_the_scratch_through_the_layout():
    from cffm_amd import hip
    cfg, p, ctx, _ = sc.make_case('F9-K8-gelu')
    bl = hip.sweep_block_layout(hip.make_shape(cfg))
    C = 2
    raw = np.arange(bl.header_floats + C * bl.block_floats, dtype=np.float32)
    blocks, written = sc.cut_blocks(raw, bl, cfg, C)
    Pp = 48
    assert blocks[0]['Z'].shape == (16, 16, Pp) and blocks[0]['U'].shape == (2, 16, Pp) and blocks[0]['Ei'].shape == (cfg.F, cfg.K)
    per = 256 * Pp + 2 * 32 * Pp + cfg.F * cfg.K + 32 + 32 + 16 + 2
    assert int(written.sum()) == C * per and not written[:bl.header_floats].any()
    seen = np.concatenate([np.asarray(v).reshape(-1) for b in blocks for v in b.values()])
    assert np.array_equal(np.sort(seen), raw[written])                             # every written float is in exactly one tensor
    assert blocks[1]['Z'][0, 0, 0] == bl.header_floats + bl.block_floats + bl.Z and float(blocks[1]['R']) == float(blocks[1]['fixed']) + 1
