"""CPU: the float64 reading of the tuple sweep's identity (tests/_sweep_tuples_ref.py) against cffm_oracle.forward on the
numpy-expanded id rows, and the evidence that the criterion of the GPU tests (oracle.parity.close(..., 'out') at its default
tolerance) sees the ways this split can go wrong, on the GPU cases' own inputs.

1e-10 is the agreement the two float64 restatements of oracle/sweep_check.py already have (tests/test_sweep_check.py): both are
float64 sums of the same terms in another order."""
import numpy as np
import pytest

from oracle import parity as T
from tests import _sweep_tuples_cases as CS
from tests import _sweep_tuples_ref as TR


_REF = {}


def reference(name, fields):
    """The oracle's scores of a case, computed once and shared (read-only)."""
    key = (name, fields)
    if key not in _REF:
        cfg, p = CS.shape_of(name)
        ctx, cand = CS.inputs_of(name, fields)
        ref = TR.oracle_scores(cfg, p, ctx, fields, cand)
        ref.setflags(write=False)
        _REF[key] = (cfg, p, ctx, cand, ref)
    return _REF[key]


@pytest.mark.parametrize('nf', [1, 2, 3, 4])
def test_block_plus_tuple_equals_the_oracle(nf):
    """nf = 1 .. 4 at F = 6 (fields in a scrambled caller's order, a list per context for the last) and at F = nf (nothing fixed)."""
    name = 'F6-K8-elu'
    cfg, p = CS.shape_of(name)
    for fields, pc in (((4, 1, 3, 2)[:nf], False), ((5, 0, 2, 3)[:nf], True)):
        ctx, cand = CS.inputs_of(name, fields, N=12, per_context=pc, seed=nf)
        got = TR.sweep_scores(cfg, p, ctx, fields, cand)
        ref = TR.oracle_scores(cfg, p, ctx, fields, cand)
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        print('nf %d fields %s: max |err| / max |ref| %.2e' % (nf, fields, err))
        assert err < 1e-10
    if nf >= 2:
        from cffm_amd.spec import CFFMConfig
        from oracle import sweep_check as sc
        cfg = CFFMConfig(M=60, F=nf, K=8, D=32, activation='selu', beta_outer=0.7, lamda_att=1.3)
        p = sc.make_params(cfg, 1)
        rng = np.random.default_rng(nf)
        ctx = rng.integers(0, 60, size=(2, nf)).astype(np.int32)
        cand = rng.integers(-1, 62, size=(9, nf)).astype(np.int32)
        fields = tuple(range(nf))[::-1]
        got, ref = TR.sweep_scores(cfg, p, ctx, fields, cand), TR.oracle_scores(cfg, p, ctx, fields, cand)
        assert float(np.abs(got - ref).max() / np.abs(ref).max()) < 1e-10


@pytest.mark.parametrize('name,fields', CS.CASES, ids=CS.CASE_IDS)
def test_the_cases_are_not_vacuous_and_the_criterion_sees_planted_faults(name, fields):
    cfg, p, ctx, cand, ref = reference(name, fields)
    N, nf = cand.shape[0], len(fields)
    good = TR.sweep_scores(cfg, p, ctx, fields, cand)
    assert float(np.abs(good - ref).max() / np.abs(ref).max()) < 1e-10
    T.close(good.reshape(-1), ref.reshape(-1), 'out')
    # non-vacuity, from the reference alone
    for c in range(ctx.shape[0]):
        assert np.unique(ref[c]).size > N / 3, 'context %d: the reference scores hardly depend on the tuple' % c
    for a in range(nf):
        other = cand.copy()
        other[:, a] = (np.clip(cand[:, a], 0, cfg.M - 1) + 1 + 3 * a) % cfg.M      # another valid id in that column alone
        moved = TR.oracle_scores(cfg, p, ctx, fields, other) != ref
        assert moved.mean() >= 0.9, 'slot %d: only %.0f %% of the scores depend on it' % (a, 100 * moved.mean())
    # the planted faults: each must FAIL the GPU tests' criterion
    rms = float(np.sqrt(np.mean(ref * ref)))
    for fault in TR.FAULTS:
        bad = TR.sweep_scores(cfg, p, ctx, fields, cand, fault=fault)
        ratio = float((np.abs(bad - ref) / (T.TOL * (np.abs(ref) + rms))).max())
        print('%s %s %s: worst err/bound %.1f' % (name, fields, fault, ratio))
        with pytest.raises(AssertionError):
            T.close(bad.reshape(-1), ref.reshape(-1), 'out: planted %s' % fault)
