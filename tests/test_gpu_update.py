"""Every update launch of optim.hip against oracle/update_check.py: the device's state is read, the route runs, the state is
read again, and the update is replayed in float64 from the inputs the kernel consumed (the dense gradient, the row gradients
in the workspace or the synthetic rows handed in, the loss-term sum) and the device's own pre-step state.  Each element of
every parameter and optimizer slot within a rigorous fp32 error bound; rows nobody looked up, channel pads and disabled
branches bit-identical.  A train step here is replayed from the device's own state, so no trajectory drifts."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cffm_amd.spec import CFFMConfig, init_params  # noqa: E402
from oracle import update_check as uc  # noqa: E402

pytestmark = pytest.mark.gpu

NONE_ROWS = {'dEi': None, 'dEo': None, 'dfb': None}


def engine(cfg, seed=1, scale_tables=True):
    from cffm_amd.engine import HipEngine
    p = init_params(cfg, seed=seed)
    if scale_tables:                   # feature_bias is exactly 0 at init: give every column a non-trivial value
        rng = np.random.default_rng(seed + 11)
        p['feature_bias'] = (rng.standard_normal(p['feature_bias'].shape) * 0.3).astype(np.float32)
        p['outer_embeddings'] = (p['outer_embeddings'] * 20.0).astype(np.float32)
    return HipEngine(cfg, params=p)


def host(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def state(eng):
    torch.cuda.synchronize()
    st = {'theta': host(eng.theta), 'inner': host(eng.inner), 'outer': host(eng.outer), 'fbias': host(eng.fbias),
          's1': {'theta': host(eng.theta_acc), 'inner': host(eng.inner_acc), 'outer': host(eng.outer_acc),
                 'fbias': host(eng.fbias_acc)}}
    if eng.theta_acc2 is not None:
        st['s2'] = {'theta': host(eng.theta_acc2), 'inner': host(eng.inner_acc2), 'outer': host(eng.outer_acc2),
                    'fbias': host(eng.fbias_acc2)}
    return st


def spread_slots(eng, rng, lo=1e-4, hi=1.0):
    """Accumulators away from 1e-8 (a quarter of the rows stay at the initial value)."""
    for t in (eng.theta_acc, eng.inner_acc, eng.outer_acc, eng.fbias_acc):
        a = np.exp(rng.uniform(np.log(lo), np.log(hi), size=tuple(t.shape))).astype(np.float32)
        a.reshape(a.shape[0], -1)[::4] = np.float32(1e-8)
        t.copy_(torch.from_numpy(a))


def grads(rng, *shape):
    """Row / dense gradients with exact zeros, tiny (< 1e-4) and large elements."""
    g = rng.standard_normal(shape) * 0.03
    u = rng.random(shape)
    g[u < 0.1] = 0.0
    g[(u >= 0.1) & (u < 0.2)] *= 1e-3
    g[(u >= 0.2) & (u < 0.25)] *= 300.0
    return g.astype(np.float32)


def id_bits(M):
    b = 1
    while (1 << b) <= M and b < 31:
        b += 1
    return b


def synthetic_ids(rng, M, n, bad=True):
    """Duplicates, ids 0 and M-1, and (bad) negative ids, M, and an id whose low id bits alias a valid id."""
    ids = rng.integers(0, M, size=n).astype(np.int64)
    if n >= 64:
        ids[rng.integers(0, n, size=n // 4)] = ids[: n // 4]          # duplicates
        ids[5], ids[6] = 0, M - 1
        if bad:
            ids[10:14] = [-1, -(1 << 31), M, ids[20] + (1 << id_bits(M))]
    return ids.astype(np.int32)


def pads_unchanged(label, eng, pre, post):
    mask = uc.theta_pad_mask(eng.tl)
    uc.check_exact(label + ' theta pads', post['theta'][mask], pre['theta'][mask])
    uc.check_exact(label + ' theta pad slots', post['s1']['theta'][mask], pre['s1']['theta'][mask])


# ---- the two building blocks of the C ABI ---------------------------------------------------------------------------------
def test_apply_dense():
    cfg = CFFMConfig(M=5382, F=10, K=32, D=32, activation='selu')
    eng = engine(cfg)
    rng = np.random.default_rng(3)
    spread_slots(eng, rng)
    n = int(eng.tl.n)
    g = grads(rng, n)
    eng.grad.copy_(torch.from_numpy(g))
    pre = state(eng)
    eng.apply_dense()
    post = state(eng)
    rep = uc.replay('AdagradOptimizer', pre, g, np.zeros(0, np.int32), NONE_ROWS, cfg.M, cfg.lr)
    uc.check_update('apply_dense', pre, post, rep)


SPARSE = {   # name: M, K, D, n_rows, inner_conv, outer_conv
    'w17-n1': (3000, 8, 8, 1, 1, 1),
    'w17-n4096-M4095': (4095, 8, 8, 4096, 1, 1),
    'w65-n4097-M4096': (4096, 32, 32, 4097, 1, 1),
    'w129-n4097-M4097': (4097, 64, 64, 4097, 1, 1),
    'w129-n4096-M8191': (8191, 64, 64, 4096, 1, 1),
    'w65-n4096-one-id': (300, 32, 32, 4096, 1, 1),
    'w65-n12000-M16385': (16385, 32, 32, 12000, 1, 1),
    'no-inner-n4097': (2049, 32, 32, 4097, 0, 1),
    'no-outer-n500': (2048, 32, 32, 500, 1, 0),
}


@pytest.mark.parametrize('name', list(SPARSE))
def test_apply_sparse(name):
    M, K, D, n, ic, oc = SPARSE[name]
    F = 8
    cfg = CFFMConfig(M=M, F=F, K=K, D=D, activation='relu', inner_conv=ic, outer_conv=oc)
    eng = engine(cfg)
    rng = np.random.default_rng(n + M)
    spread_slots(eng, rng)
    ids = synthetic_ids(rng, M, n)
    if 'one-id' in name:
        ids[:] = 7                                                   # one segment of n slots
    rows = {'dEi': grads(rng, n, K) if ic else None, 'dEo': grads(rng, n, D) if oc else None, 'dfb': grads(rng, n)}
    dev = {k: (torch.from_numpy(v).cuda() if v is not None else None) for k, v in rows.items()}
    pre = state(eng)
    eng.apply_sparse(torch.from_numpy(ids).cuda(), dev['dEi'], dev['dEo'], dev['dfb'], -(-n // F))
    post = state(eng)
    rep = uc.replay('AdagradOptimizer', pre, None, ids, rows, M, cfg.lr)
    uc.check_update('apply_sparse ' + name, pre, post, rep)
    uc.check_exact(name + ' theta', post['theta'], pre['theta'])


# ---- train_step, Adagrad: the fused update_all launch, the generic path, B*F > 4096, the regularised loss ------------------
TRAIN = {    # name: M, F, K, D, B, id_range, lamda
    'frappe-b256-fused': (5382, 10, 32, 32, 256, None, 0.0),
    'f16-k32-d32-generic': (3000, 16, 32, 32, 70, None, 0.0),
    'frappe-b1024-dups': (5382, 10, 32, 32, 1024, 150, 0.0),      # 10,240 row gradients: rocPRIM sort, generic path
    'l2-f6-d32': (2000, 6, 32, 32, 128, None, 0.02),
}


def batch(rng, M, F, B, id_range=None):
    X = rng.integers(0, id_range or M, size=(B, F)).astype(np.int64)
    if id_range:
        X = X * (M // id_range)
    X[1] = X[0]
    X[2, 0] = M - 1
    y = rng.choice([-1.0, 1.0], size=B).astype(np.float32)
    return X.astype(np.int32), y


def row_inputs(eng, B):
    dEi, dEo, dfb = eng.row_grads(B)
    F = eng.cfg.F
    return {'dEi': host(dEi).reshape(B * F, -1) if dEi is not None else None,
            'dEo': host(dEo).reshape(B * F, -1) if dEo is not None else None, 'dfb': host(dfb).reshape(-1)}


def dense_table_buffers_zero_off_rows(label, eng, B, ids, which):
    touched = np.zeros(eng.cfg.M, dtype=bool)
    touched[ids.reshape(-1)] = True
    for member, C in which:
        G = host(eng.ws_tensor(B, member, (eng.cfg.M, C))).reshape(eng.cfg.M, C)
        assert not np.any(G[~touched]), '%s: ws.%s is not 0 on rows nobody looked up' % (label, member)


@pytest.mark.parametrize('name', list(TRAIN))
def test_train_step_adagrad(name):
    M, F, K, D, B, id_range, lam = TRAIN[name]
    cfg = CFFMConfig(M=M, F=F, K=K, D=D, activation='selu', lamda_att=1.3, lamda_bilinear=lam)
    eng = engine(cfg)
    rng = np.random.default_rng(B + F)
    fused = bool(eng.lib.cffm_dp_runs_ok(eng._s, B)) and lam == 0
    for step in range(5):
        X, y = batch(rng, M, F, B, id_range)
        pre = state(eng)
        eng.train_step(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda())
        post = state(eng)
        g = host(eng.grad)
        rows = row_inputs(eng, B)
        label = '%s step %d' % (name, step)
        rep = uc.replay('AdagradOptimizer', pre, g, X.reshape(-1), rows, M, cfg.lr, lamda=lam, lamda_att=cfg.lamda_att)
        uc.check_update(label, pre, post, rep)
        pads_unchanged(label, eng, pre, post)
        if lam > 0:
            dense_table_buffers_zero_off_rows(label, eng, B, X, (('Gi', K), ('Go', D)))
            for member, key, C in (('Gi', 'dEi', K), ('Go', 'dEo', D)):
                G, A, n = uc.seg_sums(X.reshape(-1), rows[key], M)
                got = host(eng.ws_tensor(B, member, (M, C))).reshape(M, C)
                uc.check_close(label + ' ws.' + member, got, G, uc.gamma(np.maximum(n - 1, 0))[:, None] * A)
        if fused and step == 0:
            # the slab reduction alone, on the same workspace, reproduces the gradient the fused update consumed bit for bit
            buf, _ = eng.workspace(B)
            again = torch.zeros_like(eng.grad)
            from cffm_amd import hip
            hip.check(eng.lib.cffm_reduce_slabs(eng._s, buf.data_ptr(), B, again.data_ptr(), eng._stream()))
            uc.check_exact(label + ' reduce_slabs', host(again), g)
    assert fused == (name == 'frappe-b256-fused'), 'the case no longer takes the route it is named for'


# ---- train_step, SGD / Momentum / Adam (cffm_apply_opt) -------------------------------------------------------------------
# the regularised loss's data term is l2_loss = sum / 2 over the batch (not a mean): SGD on it stays finite for 12 steps only
# with a far smaller lr and unscaled tables (the float64 oracle diverges alike at lr = 1e-4)
OPT_CASES = {'plain': dict(lr=0.01), 'l2': dict(lamda_bilinear=0.05, lr=1e-5), 'no-inner': dict(inner_conv=0, lr=0.01),
             'no-outer': dict(outer_conv=0, lr=0.01)}


@pytest.mark.parametrize('variant', list(OPT_CASES))
@pytest.mark.parametrize('opt', ['GradientDescentOptimizer', 'MomentumOptimizer', 'AdamOptimizer'])
def test_train_step_other_optimizers(opt, variant):
    M, F, K, D, B = 600, 6, 16, 16, 40
    cfg = CFFMConfig(M=M, F=F, K=K, D=D, activation='elu', lamda_att=1.3, optimizer=opt, **OPT_CASES[variant])
    lam = cfg.lamda_bilinear
    eng = engine(cfg, scale_tables=lam == 0)
    rng = np.random.default_rng(len(opt) + len(variant))
    for step in range(12):
        X, y = batch(rng, M, F, B)
        pre = state(eng)
        eng.train_step(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda())
        post = state(eng)
        rows = row_inputs(eng, B)
        label = '%s %s step %d' % (opt, variant, step + 1)
        assert np.isfinite(host(eng.grad)).all() and np.isfinite(post['theta']).all(), label + ': the run diverged'
        rep = uc.replay(opt, pre, host(eng.grad), X.reshape(-1), rows, M, cfg.lr, lamda=lam, lamda_att=cfg.lamda_att,
                        t=eng.opt_step)
        uc.check_update(label, pre, post, rep)
        pads_unchanged(label, eng, pre, post)
        which = []
        if opt == 'AdamOptimizer' or lam > 0:
            which = [('Gi', K), ('Go', D)]
        if opt == 'AdamOptimizer':
            which.append(('Gfb', 1))
        dense_table_buffers_zero_off_rows(label, eng, B, X, which)
    assert eng.opt_step == 12


# ---- data-parallel apply: synthetic all-reduced gradient and gathered rows -------------------------------------------------
def dp_inputs(eng, rng, n_rows, lsum, ids=None):
    cfg = eng.cfg
    n = int(eng.tl.n)
    W = 1 + cfg.K + cfg.D + 1
    g = grads(rng, n)
    full = np.zeros(n + 4, dtype=np.float32)
    full[:n] = g
    full[n] = lsum
    if ids is None:
        ids = synthetic_ids(rng, cfg.M, n_rows)
    rows = {'dEi': grads(rng, n_rows, cfg.K), 'dEo': grads(rng, n_rows, cfg.D), 'dfb': grads(rng, n_rows)}
    packed = np.concatenate([ids.reshape(-1, 1).view(np.float32), rows['dEi'], rows['dEo'], rows['dfb'].reshape(-1, 1)], axis=1)
    assert packed.shape[1] == W
    return g, full, ids, rows, np.ascontiguousarray(packed)


DP = {   # name: n_rows, loss, loss sum
    'n100-rmse': (100, 'square_loss', 41.7),
    'n5000-rmse': (5000, 'square_loss', 913.2),
    'n8192-mse': (8192, 'mse', 913.2),
    'n8192-rmse-sum0': (8192, 'square_loss', 0.0),
    'n9000-rmse': (9000, 'square_loss', 2710.5),
    'n9000-mse': (9000, 'mse', 2710.5),
}


@pytest.mark.parametrize('name', list(DP))
def test_dp_apply(name):
    n_rows, loss, lsum = DP[name]
    cfg = CFFMConfig(M=5382, F=10, K=32, D=32, activation='selu', loss_type=loss)
    eng = engine(cfg)
    rng = np.random.default_rng(n_rows)
    spread_slots(eng, rng)
    Bg = 1000
    g, full, ids, rows, packed = dp_inputs(eng, rng, n_rows, lsum)
    pre = state(eng)
    L = eng.dp_apply(torch.from_numpy(full).cuda(), torch.from_numpy(packed).cuda(), Bg)
    post = state(eng)
    rep = uc.replay('AdagradOptimizer', pre, g, ids, rows, cfg.M, cfg.lr, late=(full[int(eng.tl.n)], Bg, loss == 'square_loss'))
    uc.check_update('dp_apply ' + name, pre, post, rep, loss=float(host(L)[0]))


def test_dp_apply_merges_eight_sorted_runs():
    """n_runs = 8: eight blocks [m rows | m sorted keys] as cffm_dp_local leaves them, ids drawn from a small range so that
    segments cross ranks; the merged order feeds the same segment walk."""
    cfg = CFFMConfig(M=5382, F=10, K=32, D=32, activation='selu')
    eng = engine(cfg)
    rng = np.random.default_rng(8)
    spread_slots(eng, rng)
    R, B = 8, 64
    m = B * cfg.F
    assert eng.lib.cffm_dp_runs_ok(eng._s, B)
    ids = (rng.integers(0, 60, size=R * m) * 89).astype(np.int32)
    ids[3] = cfg.M - 1
    g, full, ids, rows, packed = dp_inputs(eng, rng, R * m, 517.0, ids=ids)
    blocks = []
    for r in range(R):
        loc = ids[r * m:(r + 1) * m].astype(np.uint64)
        keys = np.sort((loc << np.uint64(32)) | np.arange(m, dtype=np.uint64))
        blocks += [packed[r * m:(r + 1) * m].reshape(-1), keys.view(np.float32)]
    flat = np.ascontiguousarray(np.concatenate(blocks))
    pre = state(eng)
    L = eng.dp_apply(torch.from_numpy(full).cuda(), torch.from_numpy(flat).cuda(), R * B, R)
    post = state(eng)
    rep = uc.replay('AdagradOptimizer', pre, g, ids, rows, cfg.M, cfg.lr, late=(full[int(eng.tl.n)], R * B, True))
    uc.check_update('dp_apply runs', pre, post, rep, loss=float(host(L)[0]))


def test_dp_apply_dense():
    """The dense-image route: update of every table row from the summed image (rows nobody looked up carry 0 and stay
    bit-identical), and the image is all zeros on exit."""
    cfg = CFFMConfig(M=2000, F=10, K=32, D=32, activation='selu')
    eng = engine(cfg)
    rng = np.random.default_rng(9)
    spread_slots(eng, rng)
    n, M, K, D = int(eng.tl.n), cfg.M, cfg.K, cfg.D
    nf = int(eng.lib.cffm_dp_dense_floats(eng._s))
    toff = (n + 4 + 3) // 4 * 4
    assert nf == toff + M * (K + D + 1)
    looked = np.unique(rng.integers(0, M, size=700)).astype(np.int32)
    img = {'dEi': grads(rng, len(looked), K), 'dEo': grads(rng, len(looked), D), 'dfb': grads(rng, len(looked))}
    flat = np.zeros(nf, dtype=np.float32)
    g = grads(rng, n)
    flat[:n], flat[n] = g, 377.5
    Gi = np.zeros((M, K), np.float32); Gi[looked] = img['dEi']
    Go = np.zeros((M, D), np.float32); Go[looked] = img['dEo']
    Gf = np.zeros(M, np.float32); Gf[looked] = img['dfb']
    flat[toff:] = np.concatenate([Gi.reshape(-1), Go.reshape(-1), Gf])
    dflat = torch.from_numpy(flat).cuda()
    pre = state(eng)
    L = eng.dp_apply_dense(dflat, 512)
    post = state(eng)
    rep = uc.replay('AdagradOptimizer', pre, g, looked, img, M, cfg.lr, late=(flat[n], 512, True))
    uc.check_update('dp_apply_dense', pre, post, rep, loss=float(host(L)[0]))
    left = host(dflat)[toff:]
    assert not np.any(left), 'the table image is not zero on exit (%d elements)' % int(np.count_nonzero(left))


def test_row_sharded_owner_update():
    """The owner's half of ShardedStep: two senders' gradient messages, each with the duplicates of a local row already
    summed (one record per distinct row, cffm_pack_rows_dedup's format), overlapping across senders; the owner's dp_apply sums
    the cross-sender duplicates, applies 1/L and updates its rows and accumulators."""
    cfg = CFFMConfig(M=5000, F=6, K=32, D=32, activation='relu')
    eng = engine(cfg)
    rng = np.random.default_rng(12)
    spread_slots(eng, rng)
    parts = [np.unique(rng.integers(0, 1500, size=900)).astype(np.int32) for _ in range(2)]
    ids = np.concatenate(parts)
    g, full, ids, rows, packed = dp_inputs(eng, rng, len(ids), 96.0, ids=ids)
    Bg = 2 * 128
    pre = state(eng)
    L = eng.dp_apply(torch.from_numpy(full).cuda(), torch.from_numpy(packed).cuda(), Bg)
    post = state(eng)
    rep = uc.replay('AdagradOptimizer', pre, g, ids, rows, cfg.M, cfg.lr, late=(full[int(eng.tl.n)], Bg, True))
    uc.check_update('row-sharded owner', pre, post, rep, loss=float(host(L)[0]))
