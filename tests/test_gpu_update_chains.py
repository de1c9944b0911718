"""The chains of the update launch and the single-pass instances of the backward, against replays written here.

* Dense sums (reduce_slabs_body): cffm_reduce_slabs on a workspace of seeded slabs, bit-equal to sequential float32 adds in the
  documented order - per range quarters of ceil(nslab / 4) slabs, k ascending, then ((q0 + q1) + q2) + q3.  The slab plan is
  rebuilt here from the theta layout (slab_plan below mirrors make_slab_plan of common.hpp) and tied to the library by the
  workspace layout's slab floats.
* Table-row sums (segment_walk): the dense-image route of the data-parallel step stores the sums (StoreSink); bit-equal to float32
  adds in slot order.  That route runs where the single-launch forward does (D = 32 or 64): W = 65 and W = 129.  W = 33
  (K = D = 16) is outside it and goes through cffm_sparse_adagrad with synthetic rows under the float64 bound of
  oracle/update_check.py, like tests/test_gpu_update.py.
* The backward with both single-pass call sites (conv01_bwd_kernel's layer 0, bwd_top_kernel's inner role): two engines
  bit-identical after three steps, one step within step_check of tests/test_gpu_parity.py, and workgroups without an example
  still write zero slabs."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cffm_amd import hip  # noqa: E402
from cffm_amd.spec import CFFMConfig, init_params  # noqa: E402
from oracle import update_check as uc  # noqa: E402

pytestmark = pytest.mark.gpu

NSLAB = 64            # CFFM_NSLAB
TOP_SLAB_ROWS = 32    # CFFM_TOP_SLAB_ROWS


# ---- the slab plan (common.hpp: small_slabs, conv_slabs, make_slab_plan) ---------------------------------------------------------
def small_slabs(B):
    return 256 if B <= 256 else (1024 if B >= 1024 else (B + 255) // 256 * 256)


def slab_plan(cfg, tl, B):
    """[(off, len, base, nslab)] in theta order, and the total floats."""
    F, D = cfg.F, cfg.D
    Pp = (F * (F - 1) // 2 + 15) // 16 * 16
    live = int(tl.live)
    top_ok = Pp <= 64 and B <= 256 and cfg.inner_conv and cfg.outer_conv and live >= 2
    first = max(live - 2, 1)
    fused01 = top_ok and D == 32 and Pp <= 48 and B >= 64

    def plain(l):
        S = D >> (l + 1)
        return 256 if (Pp <= 64 and B * S * S >= 256 * 64) else NSLAB

    def pair_ok(l):
        S = D >> (l + 1)
        n = plain(l)
        return l >= 1 and Pp <= 64 and (B * S * S + n - 1) // n < 128

    deferred = top_ok and not fused01 and pair_ok(first - 1)

    def conv_slabs(l):
        S = D >> (l + 1)
        if fused01:
            return 256 if l <= 1 else max(1, (B * S * S + TOP_SLAB_ROWS - 1) // TOP_SLAB_ROWS)
        if top_ok and l >= first:
            return min(256, max(1, (B * S * S + 63) // 64)) if deferred else 256
        return plain(l)

    conv_w = [int(tl.conv_w[l]) for l in range(live)]
    d1_w, n = int(tl.d1_w), int(tl.n)
    convs = conv_w[0] if live > 0 else d1_w
    cuts = [(0, int(tl.inner_cw), small_slabs(B)), (int(tl.inner_cw), convs, small_slabs(B))]
    cuts += [(conv_w[l], conv_w[l + 1] if l + 1 < live else d1_w, conv_slabs(l)) for l in range(live)]
    cuts.append((d1_w, n, small_slabs(B)))
    plan, base = [], 0
    for off, end, ns in cuts:
        plan.append((off, end - off, base, ns))
        base += (end - off) * ns
    return plan, base


def quarter_sums(slabs):
    """slabs [nslab][len] float32 -> [len]: the documented add order."""
    ns = slabs.shape[0]
    per = (ns + 3) // 4
    q = np.zeros((4, slabs.shape[1]), np.float32)
    for w in range(4):
        for k in range(w * per, min(ns, w * per + per)):
            q[w] = q[w] + slabs[k]
    return ((q[0] + q[1]) + q[2]) + q[3]


def slab_values(rng, n):
    """Exact zeros (also negative zeros), tiny and large elements."""
    g = (rng.standard_normal(n) * 0.03).astype(np.float32)
    u = rng.random(n)
    g[u < 0.1] = 0.0
    g[(u >= 0.1) & (u < 0.12)] = -0.0
    g[(u >= 0.12) & (u < 0.2)] *= np.float32(1e-3)
    g[(u >= 0.2) & (u < 0.25)] *= np.float32(300.0)
    g[(u >= 0.25) & (u < 0.26)] *= np.float32(1e-30)
    return g


_POOL = {}


def slab_pool(n):
    """One seeded buffer shared by the cases (each takes a prefix)."""
    if _POOL.get('n', 0) < n:
        _POOL['v'] = slab_values(np.random.default_rng(2024), max(n, 8_500_000))
        _POOL['n'] = _POOL['v'].shape[0]
    return _POOL['v'][:n]


def engine(cfg, seed=1, scale=True):
    from cffm_amd.engine import HipEngine
    p = init_params(cfg, seed=seed)
    if scale:
        rng = np.random.default_rng(seed + 11)
        p['feature_bias'] = (rng.standard_normal(p['feature_bias'].shape) * 0.3).astype(np.float32)
        p['outer_embeddings'] = (p['outer_embeddings'] * 20.0).astype(np.float32)
    return HipEngine(cfg, params=p)


DENSE = [(10, 32, 32, 200, B) for B in (1, 3, 65, 100, 256, 300)] + [(5, 16, 16, 200, 64)]


@pytest.mark.parametrize('F,K,D,M,B', DENSE, ids=['f%d-k%d-b%d' % (c[0], c[1], c[4]) for c in DENSE])
def test_dense_sums_are_the_documented_float32_adds(F, K, D, M, B):
    cfg = CFFMConfig(M=M, F=F, K=K, D=D, activation='selu')
    eng = engine(cfg, scale=False)
    buf, wl = eng.workspace(B)
    plan, total = slab_plan(cfg, eng.tl, B)
    assert total == int(wl.gpart_floats), 'slab_plan() no longer mirrors make_slab_plan'
    ns = {p[3] for p in plan}
    if (F, B) == (10, 65):
        assert plan[5][3] == 9                      # layer 3: quarters 3 / 3 / 3 / 0
    if (F, B) == (10, 100):
        assert (plan[4][3], plan[5][3]) == (50, 13)
    if (F, B) == (10, 300):
        assert 512 in ns and 256 in ns              # outside the fused backward: small ranges of 512 slabs
    vals = slab_pool(total)
    eng.ws_tensor(B, 'gpart', (total,)).copy_(torch.from_numpy(vals))
    n = int(eng.tl.n)
    flat = torch.full((n,), float('nan'), dtype=torch.float32, device=eng.device)
    hip.check(eng.lib.cffm_reduce_slabs(eng._s, buf.data_ptr(), B, flat.data_ptr(), eng._stream()))
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    want = np.empty(n, np.float32)
    for off, ln, base, nslab in plan:
        want[off:off + ln] = quarter_sums(vals[base:base + nslab * ln].reshape(nslab, ln))
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, '%d of %d sums differ in their bits, first at %d: %r vs %r' % (bad.size, n, bad[0], got[bad[0]], want[bad[0]])


# ---- table-row sums -------------------------------------------------------------------------------------------------------------------
def id_patterns(name, M, F, rng):
    """[B][F] ids at M = 200 (ids below 20 are reserved for the runs)."""
    if name == 'b1':
        return rng.integers(20, M, size=(1, F)).astype(np.int32)
    if name == 'distinct':
        B = (M - 20) // F
        return (20 + rng.permutation(B * F)).reshape(B, F).astype(np.int32)
    B = 100
    X = rng.integers(20, M - 1, size=(B, F)).astype(np.int32)
    X[:, 0] = 7                                    # one id 100 times: a run longer than a chunk of 64 keys
    X[:64, 1] = 11                                 # a run of exactly 64
    X[:65, 2] = 13                                 # ... and of 65
    X[[4, 50, 99], 3] = M - 1                      # the largest id: its run ends at the last sorted position
    if name == 'bad-ids':
        X[[2, 60], 4] = -1
        X[[3, 61, 62], 4] = M
    return X


def row_sums(ids, rows, M):
    """float32 sums of rows [n][C] per id in slot order; ids outside [0, M) are skipped."""
    G = np.zeros((M, rows.shape[1]), np.float32)
    for s, i in enumerate(ids):
        if 0 <= i < M:
            G[i] = G[i] + rows[s]
    return G


ROWS = [(K, p) for K in (32, 64) for p in ('distinct', 'runs', 'bad-ids', 'b1')]


@pytest.mark.parametrize('K,pattern', ROWS, ids=['w%d-%s' % (2 * k + 1, p) for k, p in ROWS])
def test_table_row_sums_are_float32_adds_in_slot_order(K, pattern):
    M, F, D = 200, 10, K
    cfg = CFFMConfig(M=M, F=F, K=K, D=D, activation='selu')
    eng = engine(cfg)
    rng = np.random.default_rng(K + len(pattern))
    X = id_patterns(pattern, M, F, rng)
    B = X.shape[0]
    if not eng.lib.cffm_dp_runs_ok(eng._s, B):
        assert K == 64, 'W = 65 must take the route that stores the sums'
        sparse_route(cfg, eng, X.reshape(-1), rng)
        return
    y = rng.choice([-1.0, 1.0], size=B).astype(np.float32)
    flat = eng.dp_local_dense(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda(), B, B)
    torch.cuda.synchronize()
    n = int(eng.tl.n)
    toff = (n + 4 + 3) // 4 * 4
    img = flat.cpu().numpy()[toff:]
    dEi, dEo, dfb = (t.cpu().numpy() for t in eng.row_grads(B))
    ids = X.reshape(-1)
    parts = ((dEi.reshape(B * F, K), 'Gi'), (dEo.reshape(B * F, D), 'Go'), (dfb.reshape(B * F, 1), 'Gfb'))
    at = 0
    for rows, label in parts:
        C = rows.shape[1]
        got = img[at:at + M * C].reshape(M, C)
        at += M * C
        want = row_sums(ids, rows, M)
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, '%s: %d elements differ in their bits, first at %s' % (label, len(bad), bad[0])
        assert np.any(want != 0)
    assert at == img.shape[0]


def sparse_route(cfg, eng, ids, rng):
    """cffm_sparse_adagrad on synthetic rows with these ids, under the float64 bound of oracle/update_check.py."""
    from tests.test_gpu_update import grads, spread_slots, state
    n, F = ids.shape[0], cfg.F
    spread_slots(eng, rng)
    rows = {'dEi': grads(rng, n, cfg.K), 'dEo': grads(rng, n, cfg.D), 'dfb': grads(rng, n)}
    dev = {k: torch.from_numpy(v).cuda() for k, v in rows.items()}
    pre = state(eng)
    eng.apply_sparse(torch.from_numpy(ids).cuda(), dev['dEi'], dev['dEo'], dev['dfb'], -(-n // F))
    post = state(eng)
    rep = uc.replay('AdagradOptimizer', pre, None, ids, rows, cfg.M, cfg.lr)
    uc.check_update('sparse chains', pre, post, rep)
    uc.check_exact('theta', post['theta'], pre['theta'])


@pytest.mark.parametrize('pattern', ['distinct', 'runs', 'bad-ids', 'b1'])
def test_table_rows_w33_through_sparse_adagrad(pattern):
    """K = D = 16: the route that stores the sums does not take D = 16, so W = 33 is checked on the applied update."""
    M, F, K = 200, 10, 16
    cfg = CFFMConfig(M=M, F=F, K=K, D=K, activation='relu')
    eng = engine(cfg)
    assert not eng.lib.cffm_dp_runs_ok(eng._s, 100)
    rng = np.random.default_rng(33 + len(pattern))
    sparse_route(cfg, eng, id_patterns(pattern, M, F, rng).reshape(-1), rng)


# ---- the backward with both single-pass call sites ------------------------------------------------------------------------------------------
BWD = {
    'chains-f10-b64-selu': dict(M=900, F=10, K=32, D=32, act='selu', B=64),
    'chains-f10-b256-selu': dict(M=900, F=10, K=32, D=32, act='selu', B=256),
    'chains-f9-b64-selu': dict(M=900, F=9, K=32, D=32, act='selu', B=64),          # a generic instance at Pp = 48
    'chains-f10-b100-elu': dict(M=900, F=10, K=16, D=32, act='elu', B=100),        # 156 workgroups without an example
}


def bwd_case(name):
    from tests import test_gpu_parity as par
    par.CASES[name] = BWD[name]
    return par, par.make_case(name)


@pytest.mark.parametrize('name', list(BWD))
def test_single_pass_backward_is_reproducible(name):
    par, (cfg, p32, X, y) = bwd_case(name)
    rng = np.random.default_rng(5)
    batches = [X, np.ascontiguousarray(X[::-1]), rng.integers(0, cfg.M, size=X.shape).astype(np.int32)]
    outs = []
    for _ in range(2):
        eng = par.engine_for(cfg, p32)
        losses = [float(eng.train_step(torch.from_numpy(Xs).cuda(), torch.from_numpy(y).cuda())) for Xs in batches]
        torch.cuda.synchronize()
        outs.append((eng.export_params(), eng.export_accumulators(), losses))
    assert outs[0][2] == outs[1][2] and all(np.isfinite(outs[0][2]))
    for which in (0, 1):
        for k, v in outs[0][which].items():
            np.testing.assert_array_equal(v, outs[1][which][k], err_msg=k)


@pytest.mark.parametrize('name', list(BWD))
def test_single_pass_backward_step_matches_the_oracle(name):
    par, (cfg, p32, X, y) = bwd_case(name)
    par.step_check(cfg, par.engine_for(cfg, p32), p32, None, X, y, name)


def test_workgroups_without_an_example_write_zero_slabs():
    name = 'chains-f10-b100-elu'
    par, (cfg, p32, X, y) = bwd_case(name)
    B = X.shape[0]
    eng = par.engine_for(cfg, p32)
    plan, total = slab_plan(cfg, eng.tl, B)
    _, wl = eng.workspace(B)
    assert total == int(wl.gpart_floats)
    assert plan[2][3] == 256 and plan[1][3] == 256 and B < 256          # layer 0 and the inner branch: one slab per workgroup
    gpart = eng.ws_tensor(B, 'gpart', (total,))
    for r in (1, 2):                                                     # inner branch (bwd_top_kernel), layer 0 (conv01_bwd_kernel)
        off, ln, base, nslab = plan[r]
        gpart[base + B * ln:base + nslab * ln].fill_(float('nan'))        # what the workgroups without an example must overwrite
    eng.train_step(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda())
    torch.cuda.synchronize()
    gp = gpart.cpu().numpy()
    for r in (1, 2):
        off, ln, base, nslab = plan[r]
        slabs = gp[base:base + nslab * ln].reshape(nslab, ln)
        assert not np.any(slabs[B:]), 'range %d: a slab past the batch is not zero' % r
        assert np.any(slabs[:B])
