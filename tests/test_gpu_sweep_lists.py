"""GPU: cffm_score_sweep_lists - the shared candidate sweep with a candidate list per context - tied bit for bit to cffm_score_sweep,
whose agreement with the float64 oracle tests/test_gpu_sweep.py holds: the new entry point changes where a candidate id is read
from and nothing else, so no tolerance appears here.

  * every list equal to one shared list: the scores cffm_score_sweep gives for that list;
  * distinct lists: row c is cffm_score_sweep of context c alone with list c;
  * stride 0 through the new entry point: cffm_score_sweep itself.

Shapes: F 10 / K 32 (Pp = 48) and F 3 / K 8 (Pp = 16), D = 32; C = 3; N in {1, 64, 65, 130} - below, at and above the chunk of
candidates one workgroup unit takes, and one context spread over three units; list strides N and N + 5, the gap holding an id
that differs from every candidate.  The scores lie in guarded rows of N + 5 floats whose gap holds 3e38 and must keep it."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cffm_amd import hip  # noqa: E402
from oracle import rows_check as rc  # noqa: E402
from tests import _cand_ref as CR  # noqa: E402
from tests.test_gpu_rows import Guard, dev_of, stream  # noqa: E402
from tests.test_gpu_sweep import CASES, GAP, SENTINEL, engine_of, sweep_abi  # noqa: E402

pytestmark = pytest.mark.gpu

assert hip.SWEEP_CHUNK == 64


def lists_abi(eng, ctx, field, flat, stride, N, label):
    """cffm_score_sweep_lists into guarded, gapped rows; the [C, N] scores after the canaries, the gap and the scratch's canaries
    have been checked."""
    C = ctx.shape[0]
    lib = eng.lib
    nbytes = int(lib.cffm_sweep_scratch_bytes(eng._s, C))
    assert nbytes > 0, label
    scores, scratch = Guard(C * (N + GAP) * 4), Guard(nbytes)
    scores.view().reshape(C, N + GAP)[:, N:] = float(SENTINEL)
    dctx, dcand = dev_of(ctx), dev_of(flat)
    rcode = lib.cffm_score_sweep_lists(eng._s, eng._t, eng.theta.data_ptr(), dctx.data_ptr(), C, int(field), dcand.data_ptr(), stride, N,
                                       scores.ptr, N + GAP, scratch.ptr, stream())
    assert rcode == 0, '%s returned %d' % (label, rcode)
    img = scores.read(label).reshape(C, N + GAP)
    scratch.read(label + ' scratch')
    rc.check_exact(label + ': the gap behind every row', img[:, N:], np.full((C, GAP), SENTINEL, dtype=np.float32))
    got = np.ascontiguousarray(img[:, :N])
    assert not (rc.bits(got) == rc.POISON).any(), '%s: scores left at poison' % label
    return got


@pytest.mark.parametrize('N', [1, 64, 65, 130])
@pytest.mark.parametrize('name', ['frappe-selu', 'f3-relu'])
def test_lists_equal_the_shared_sweep(name, N):
    cfg = CASES[name][0]
    eng = engine_of(name)
    C, field = 3, 1
    rng = np.random.default_rng(N)
    ctx = rng.integers(0, cfg.M, size=(C, cfg.F)).astype(np.int32)
    # ids of [1, M): 0 is kept for the gap, so a read behind a list scores a row no candidate has
    lists = rng.integers(1, cfg.M, size=(C, N)).astype(np.int32)
    lists[0, 0], lists[C - 1, N - 1] = -1, cfg.M                              # clamped: < 0 -> 0, >= M -> M - 1
    one = lists[1]
    ref_one = sweep_abi(eng, ctx, field, one, '%s N=%d: cffm_score_sweep' % (name, N))
    assert N < 8 or np.unique(ref_one).size > N // 2, 'the scores hardly depend on the candidate'
    ref_own = np.concatenate([sweep_abi(eng, ctx[c:c + 1], field, lists[c], '%s N=%d: context %d alone' % (name, N, c)) for c in range(C)])
    for stride in (N, N + 5):
        label = '%s N=%d stride %d' % (name, N, stride)
        same = CR.flat_lists(np.repeat(one[None, :, None], C, axis=0), stride, 0)
        rc.check_exact(label + ': every list the shared list', lists_abi(eng, ctx, field, same, stride, N, label), ref_one)
        own = CR.flat_lists(lists[:, :, None], stride, 0)
        rc.check_exact(label + ': a list per context', lists_abi(eng, ctx, field, own, stride, N, label), ref_own)
    rc.check_exact('%s N=%d stride 0' % (name, N), lists_abi(eng, ctx, field, one, 0, N, 'stride 0'), ref_one)


def test_engine_lists_shared():
    name = 'f3-relu'
    cfg = CASES[name][0]
    eng = engine_of(name)
    rng = np.random.default_rng(8)
    C, N = 4, 70
    ctx = rng.integers(0, cfg.M, size=(C, cfg.F)).astype(np.int32)
    lists = rng.integers(0, cfg.M, size=(C, N)).astype(np.int32)
    got = eng.score_candidate_lists_shared(dev_of(ctx), 2, dev_of(lists))
    assert got.shape == (C, N)
    for c in range(C):
        rc.check_exact('context %d' % c, got[c].cpu().numpy(),
                       eng.score_candidates_shared(dev_of(ctx[c:c + 1]), 2, dev_of(lists[c])).cpu().numpy().reshape(-1))
    assert eng.score_candidate_lists_shared(dev_of(ctx[:0]), 0, dev_of(lists[:0])).shape == (0, N)
    for bad_ctx, field, bad_lists in ((ctx, -1, lists), (ctx, cfg.F, lists), (ctx, 0, lists[:3]), (ctx, 0, lists[0]), (ctx, 0, lists[:, :0]),
                                      (ctx[:, :-1], 0, lists)):
        with pytest.raises(ValueError):
            eng.score_candidate_lists_shared(dev_of(bad_ctx), field, dev_of(bad_lists))
