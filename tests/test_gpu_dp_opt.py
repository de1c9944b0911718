"""cffm_dp_apply_opt on the GPU: the SGD / Momentum apply of the data-parallel and row-sharded steps.

By element.  The device's parameters and slots are read, the local half of a step runs (dp_local, or forward + backward_unscaled),
the exact fp32 gradient, packed rows and loss-term sum the apply will consume are read back, dp_apply runs, and every element of
every parameter and slot is held to the float64 replay of tests/_dp_opt_check.py through update_check.check_update: moved elements
within a rigorous fp32 bound, rows nobody looked up and their slots bit-identical.  Each route of the apply appears at the
smallest shape that reaches it (ROUTES).  The Momentum slots start from random values, so a decayed accumulator of an untouched
row, or 0.95 on the wrong operand, cannot hide behind a zero; a second apply with disjoint ids must leave the rows of the first
and their slots bit-identical.

End to end at world 2: two ranks on cuda:0 over gloo (the harness of tests/test_gpu_dist.py: the children are started before the
parent touches the GPU in the test, two processes with the GPU open, the harness' queue timeout), DataParallelStep and
ShardedStep for two steps against ONE HipEngine.train_step (cffm_train_step_opt) on the whole batch.  Criterion: that of
tests/test_gpu_dist.py::_same's first step, 1e-4 relative / 2e-6 absolute, with at most 0.2 % of a tensor's elements left out of
it; the worst error / bound ratio of every tensor is printed.

HIP-graph capture cannot be rehearsed over gloo (its collectives go through the host, which a capture refuses): as
tests/test_gpu_fullsize.py does for Adagrad, the captured step runs at world size 1 over RCCL loopback against an eager twin."""
import copy
import ctypes as C
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
from tests import _dp_opt_check as dc  # noqa: E402
from tests import test_dist_cpu as H  # noqa: E402   (the spawn / gloo harness)
from tests import test_gpu_dist as G  # noqa: E402   (its cases)
from tests.test_gpu_update import engine, host, state  # noqa: E402

pytestmark = pytest.mark.gpu
TABLES = G.TABLES
OPTS = ['GradientDescentOptimizer', 'MomentumOptimizer']
LOSSES = ['square_loss', 'mse']                       # late scale != 1, late scale exactly 1

# route: F, K, D, M, examples per block, blocks (n_runs of the apply; 0: one block without a sorted run), id values per batch
ROUTES = {
    'place': (3, 8, 8, 40, 8, 0, 12),                 # n_rows = 24 <= 8192: dense rule ∥ key placement; W = 17, one column pass
    'merge': (10, 32, 32, 800, 64, 2, 40),            # two dp_local blocks as world 2 gathers them; W = 65, two column passes
    'radix': (10, 32, 32, 800, 1024, 0, 400),         # n_rows = 10,240 > 8192: dense rule, radix sort, sparse rule
}


# SGD and Momentum have no per-element normaliser, and at F10 K32 D32 an untrained model answers ~25 where the labels are +-1: with
# ids drawn from 40 values (a row gradient is the sum of ~30 duplicates) lr = 0.05 overflows fp32 in the second apply, on one GPU
# as in the float64 oracle (loss 20 -> 1e7 -> 1e24).  The check is element-wise against the apply's own inputs, so any lr serves;
# these keep two applies finite in the oracle (the mse gradient is 2 L ~ 40 times the RMSE-style one).
LR = {'place': {'square_loss': 0.05, 'mse': 0.05}, 'merge': {'square_loss': 2e-5, 'mse': 5e-7}, 'radix': {'square_loss': 2e-5, 'mse': 5e-7}}


def _config(route, opt, loss, **kw):
    F, K, D, M = ROUTES[route][:4]
    return CFFMConfig(M=M, F=F, K=K, D=D, activation='selu', lamda_att=1.3, optimizer=opt, loss_type=loss, lr=LR[route][loss], **kw)


def _engine(route, cfg):
    eng = engine(cfg, scale_tables=route == 'place')
    if route != 'place':                               # feature_bias is exactly 0 at init: give it values to round against
        eng.fbias.copy_(torch.from_numpy((np.random.default_rng(2).standard_normal(cfg.M) * 0.3).astype(np.float32)))
    return eng


def _random_slots(eng, rng):
    """Momentum accumulators away from 0 (SGD never reads them: they must come back bit-identical)."""
    for t in (eng.theta_acc, eng.inner_acc, eng.outer_acc, eng.fbias_acc):
        t.copy_(torch.from_numpy((rng.standard_normal(tuple(t.shape)) * 0.02).astype(np.float32)))


def _batches(route, rng, second):
    """The id blocks of one apply: values k * step (+ 1 for the second apply, so the two applies share no id), duplicates inside
    a block and across blocks; the first apply also looks up the last row of the vocabulary."""
    F, K, D, M, B, blocks, nval = ROUTES[route]
    step = M // nval
    assert step >= 2
    out = []
    for b in range(max(blocks, 1)):
        X = (rng.integers(0, nval - 1 if second else nval, size=(B, F)) * step + (1 if second else 0)).astype(np.int32)   # never M - 1 twice
        X[1] = X[0]
        if not second and b == 0:
            X[2, 0] = M - 1
        out.append((X, rng.choice([-1.0, 1.0], size=B).astype(np.float32)))
    return out


def _local_half(eng, route, batches):
    """Runs the local half of every block; returns (grad_sum [n + 4], rows tensor for dp_apply, n_runs, Bg, host ids, host rows)."""
    F, K, D, M, B, blocks, _ = ROUTES[route]
    W = 1 + K + D + 1
    Bg = B * len(batches)
    grads, blocks_dev, packed = [], [], []
    for X, y in batches:
        ids, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
        if blocks:
            assert eng.lib.cffm_dp_runs_ok(eng._s, B)
            g, blk = eng.dp_local(ids, yt, B, Bg)
            packed.append(host(blk)[:B * F * W].reshape(B * F, W))
        else:
            eng.forward(ids, yt)
            g, blk = eng.backward_unscaled(ids, yt, B, Bg)
            packed.append(host(blk))
        grads.append(g.clone())
        blocks_dev.append(blk.clone())
    grad = grads[0]
    for g in grads[1:]:
        grad = grad + g                                # what the all-reduce hands every rank (fp32, this order)
    rows_dev = torch.cat([b.reshape(-1) for b in blocks_dev]) if blocks else blocks_dev[0]
    return grad.contiguous(), rows_dev.contiguous(), blocks, Bg, np.concatenate(packed)


def _unpack(cfg, packed):
    K, D = cfg.K, cfg.D
    ids = np.ascontiguousarray(packed[:, 0]).view(np.int32).copy()
    dEi, dEo = packed[:, 1:1 + K], packed[:, 1 + K:1 + K + D]
    if not cfg.inner_conv:
        assert not np.any(dEi), 'a disabled branch travels as zeros'
    if not cfg.outer_conv:
        assert not np.any(dEo), 'a disabled branch travels as zeros'
    return ids, {'dEi': dEi if cfg.inner_conv else None, 'dEo': dEo if cfg.outer_conv else None, 'dfb': packed[:, 1 + K + D]}


def _apply_and_check(label, eng, route, batches):
    cfg = eng.cfg
    n = int(eng.tl.n)
    grad, rows_dev, n_runs, Bg, packed = _local_half(eng, route, batches)
    ids, rows = _unpack(cfg, packed)
    g_host = host(grad)
    pre = state(eng)
    L = eng.dp_apply(grad, rows_dev, Bg, n_runs)
    post = state(eng)
    assert np.isfinite(g_host).all() and np.isfinite(post['theta']).all(), label
    rep = dc.replay_late(cfg.optimizer, pre, g_host[:n], ids, rows, cfg.M, cfg.lr, g_host[n], Bg, cfg.loss_type == 'square_loss')
    uc.check_update(label, pre, post, rep, loss=float(host(L)[0]))
    print('\nworst error / bound, %s: %s' % (label, ', '.join(
        '%s %.2f' % (k[len(label) + 1:], v) for k, v in sorted(uc.WORST.items(), key=lambda kv: -kv[1]) if k.startswith(label + ' '))))
    if cfg.optimizer == 'GradientDescentOptimizer':
        for k in pre['s1']:
            uc.check_exact('%s: SGD keeps no slot (%s)' % (label, k), post['s1'][k], pre['s1'][k])
    return ids, pre, post


@pytest.mark.parametrize('loss', LOSSES)
@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('route', list(ROUTES))
def test_every_route_of_the_apply_by_element(route, opt, loss):
    cfg = _config(route, opt, loss)
    eng = _engine(route, cfg)
    rng = np.random.default_rng(len(route) + len(opt) + len(loss))
    _random_slots(eng, rng)
    label = '%s %s %s' % (route, opt, loss)
    ids1, _, post1 = _apply_and_check(label + ' apply 1', eng, route, _batches(route, rng, False))
    assert np.unique(ids1).size < ids1.size                   # there were duplicates to sum
    if ROUTES[route][5]:
        m = ids1.size // ROUTES[route][5]
        assert np.intersect1d(ids1[:m], ids1[m:]).size > 0    # and ids that appear in both runs
    # a second apply on ids the first never looked up: the first apply's rows and slots stay as they are, bit for bit
    ids2, pre2, post2 = _apply_and_check(label + ' apply 2', eng, route, _batches(route, rng, True))
    assert np.intersect1d(ids1, ids2).size == 0
    rows1 = np.unique(ids1)
    for k in ('inner', 'outer', 'fbias'):
        uc.check_exact(label + ': rows of apply 1 after apply 2, ' + k, post2[k][rows1], post1[k][rows1])
        uc.check_exact(label + ': slots of apply 1 after apply 2, ' + k, post2['s1'][k][rows1], post1['s1'][k][rows1])
        if opt == 'MomentumOptimizer':
            assert np.any(post1['s1'][k][rows1] != 0)


@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('branch', ['inner_conv', 'outer_conv'])
def test_a_disabled_branch_keeps_its_table_and_slot(opt, branch):
    cfg = _config('place', opt, 'square_loss', **{branch: 0})
    eng = engine(cfg)
    rng = np.random.default_rng(5)
    _random_slots(eng, rng)
    _, pre, post = _apply_and_check('no %s %s' % (branch, opt), eng, 'place', _batches('place', rng, False))
    k = 'inner' if branch == 'inner_conv' else 'outer'
    uc.check_exact('disabled table', post[k], pre[k])
    uc.check_exact('disabled table slot', post['s1'][k], pre['s1'][k])
    other = 'outer' if k == 'inner' else 'inner'
    assert np.any(post[other] != pre[other])


@pytest.mark.parametrize('opt', OPTS)
def test_ids_outside_the_vocabulary_are_skipped(opt):
    """Ids >= M and a negative id planted in the rows: their rows are skipped and nothing outside [0, M) is written.  The tables and
    their slots lie between canaries (tests/test_gpu_rows.py: Guard); the planted ids are close enough to the vocabulary that an
    unguarded write would land in a canary, not in foreign memory."""
    from tests.test_gpu_rows import Guard
    cfg = _config('place', opt, 'square_loss')
    eng = engine(cfg)
    rng = np.random.default_rng(6)
    _random_slots(eng, rng)
    M, K, D, F = cfg.M, cfg.K, cfg.D, cfg.F
    n = int(eng.tl.n)
    grad, rows_dev, n_runs, Bg, packed = _local_half(eng, 'place', _batches('place', rng, False))
    bad = {5: M, 9: M + 3, 13: -1, 17: M + 100}
    assert max(bad.values()) - M + 1 <= 4096 // (4 * max(K, D))                   # inside the rear canary
    for slot, v in bad.items():
        rows_dev[slot, 0:1].view(torch.int32).fill_(v)
        packed[slot, 0:1].view(np.int32)[:] = v
    ids, rows = _unpack(cfg, packed)
    assert set(bad.values()) <= set(ids.tolist())
    pre = state(eng)
    names = (('inner', eng.inner, eng.inner_acc), ('outer', eng.outer, eng.outer_acc), ('fbias', eng.fbias, eng.fbias_acc))
    guards = {}
    for k, w, a in names:
        for tag, t in (('w', w), ('s', a)):
            gd = Guard(t.numel() * 4)
            gd.view()[:] = t.reshape(-1)
            guards[tag + k] = gd
    tab = hip.Tables(guards['winner'].ptr, guards['wouter'].ptr, guards['wfbias'].ptr)
    slot = hip.Tables(guards['sinner'].ptr, guards['souter'].ptr, guards['sfbias'].ptr)
    n_rows = packed.shape[0]
    B_ws = -(-n_rows // F)
    buf, _ = eng.workspace(B_ws)
    hip.check(eng.lib.cffm_dp_apply_opt(eng._s, C.addressof(tab), C.addressof(slot), eng.theta.data_ptr(), eng.theta_acc.data_ptr(),
                                        grad.data_ptr(), Bg, rows_dev.data_ptr(), n_rows, buf.data_ptr(), B_ws,
                                        eng.loss_buf.data_ptr(), 0, eng._stream()))
    post = state(eng)                                                              # theta and its slot
    for k, w, a in names:
        uc.check_exact('the engine\'s own table was not the target: ' + k, post[k], pre[k])
        post[k] = guards['w' + k].read('table ' + k).reshape(pre[k].shape)         # canaries checked
        post['s1'][k] = guards['s' + k].read('slot ' + k).reshape(pre[k].shape)
    g_host = host(grad)
    rep = dc.replay_late(opt, pre, g_host[:n], ids, rows, M, cfg.lr, g_host[n], Bg, True)
    uc.check_update('bad ids ' + opt, pre, post, rep, loss=float(host(eng.loss_buf)[0]))


# ---- end to end at world 2 -----------------------------------------------------------------------------------------------------
def _case(opt, wide=False):
    """The cases of tests/test_gpu_dist.py with the optimizer set.  Their untrained models answer ~100 (narrow) and ~1500 (wide)
    where the labels are +-1, and neither rule normalises a gradient: lr = 0.05 diverges within two steps on ONE engine as in the
    float64 oracle (narrow: loss 107 -> 1.3e7 -> 3.9e26).  lr is the largest power of ten at which the oracle's loss falls over
    three steps (narrow 107 -> 53 -> 28, wide 1480 -> 658 -> 397).  At such an lr most parameters move by about the absolute
    tolerance, so for them the comparison is loose; the Momentum slots (after step 1 the summed, late-scaled gradient itself, held
    to 1e-4 relative) and the by-element tests above carry the sensitivity to a wrong scale, a lost rank or a mis-routed row."""
    cfg, X, y = G._case(wide)
    cfg.optimizer = opt
    cfg.lr = 1e-6 if wide else 1e-5
    return cfg, X, y


def _dp_worker(rank, world, mode, opt):
    from cffm_amd.dist import DataParallelStep, replicas_agree
    from cffm_amd.engine import HipEngine
    cfg, X, y = _case(opt)
    eng = HipEngine(cfg, params=init_params(cfg, seed=7 + rank), device='cuda:0')   # different draws: rank 0's must win
    dense_calls, local_dense = [], eng.dp_local_dense
    eng.dp_local_dense = lambda *a: (dense_calls.append(1), local_dense(*a))[1]
    dp = DataParallelStep(eng, mode=mode)
    per = X.shape[1] // world
    sl = slice(rank * per, rank * per + per)
    out = []
    for s in range(X.shape[0]):
        loss = dp.train_step(torch.from_numpy(X[s, sl].copy()).cuda(), torch.from_numpy(y[s, sl].copy()).cuda())
        torch.cuda.synchronize()
        assert replicas_agree(eng, tables=True)
        out.append((float(loss.cpu().reshape(-1)[0]), eng.export_params(), eng.export_accumulators()))
    assert not dense_calls, 'the dense-image route is Adagrad only'
    return out


def _sharded_worker(rank, world, opt, wide):
    from cffm_amd.dist import ShardedStep, local_rows_count, replicas_agree, shard_params
    from cffm_amd.engine import HipEngine
    cfg, X, y = _case(opt, wide)
    lcfg = copy.copy(cfg)
    lcfg.M = local_rows_count(cfg.M, rank, world)
    eng = HipEngine(lcfg, params=shard_params(init_params(cfg, seed=7), rank, world), device='cuda:0')
    sh = ShardedStep(eng)
    assert eng.packed_ok() == wide
    per = X.shape[1] // world
    sl = slice(rank * per, rank * per + per)
    ids = [torch.from_numpy(X[s, sl].copy()).cuda() for s in range(X.shape[0])]
    ys = [torch.from_numpy(y[s, sl].copy()).cuda() for s in range(X.shape[0])]
    out = []
    for s in range(len(ids)):
        loss = sh.train_step(ids[s], ys[s], next_ids=ids[s + 1] if s + 1 < len(ids) else None)
        torch.cuda.synchronize()
        assert replicas_agree(eng, tables=False)
        out.append((float(loss.cpu().reshape(-1)[0]), eng.export_params(), eng.export_accumulators()))
    return out


def _single(opt, wide=False):
    from cffm_amd.engine import HipEngine
    cfg, X, y = _case(opt, wide)
    eng = HipEngine(cfg, params=init_params(cfg, seed=7), device='cuda:0')
    out = []
    for s in range(X.shape[0]):
        loss = eng.train_step(torch.from_numpy(X[s]).cuda(), torch.from_numpy(y[s]).cuda())
        torch.cuda.synchronize()
        out.append((float(loss.cpu().reshape(-1)[0]), eng.export_params(), eng.export_accumulators()))
    return out


def _within(a, b, what, worst):
    """1e-4 relative / 2e-6 absolute; at most 0.2 % of the elements of a tensor may lie outside.  Records the worst error / bound."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.isfinite(a).all(), what
    ratio = np.abs(a - b) / (2e-6 + 1e-4 * np.abs(b))
    worst[what] = max(worst.get(what, 0.0), float(ratio.max()) if ratio.size else 0.0)
    inside = float((ratio <= 1.0).mean()) if ratio.size else 1.0
    assert inside >= 0.998, '%s: %.4f %% of the elements within 1e-4 / 2e-6, worst error / bound %.3g' % (what, 100 * inside, ratio.max())


def _against_single(res, ref, opt, sharded, label):
    worst = {}
    for step, (L, p, acc) in enumerate(ref):
        for rank in (0, 1):
            loss, got, gacc = res[rank][step]
            _within(loss, L, 'loss', worst)
            for k in acc:                                  # the trained variables, as tests/test_gpu_dist.py
                cut = (lambda v: np.asarray(v)[rank::2]) if (sharded and k in TABLES) else np.asarray
                _within(got[k], cut(p[k]), k, worst)
                if opt == 'MomentumOptimizer':
                    _within(gacc[k], cut(acc[k]), 'slot of ' + k, worst)
        for k in acc:                                      # the replicas stay bit-identical
            if not (sharded and k in TABLES):
                np.testing.assert_array_equal(np.asarray(res[0][step][1][k]), np.asarray(res[1][step][1][k]), err_msg=k)
                np.testing.assert_array_equal(np.asarray(res[0][step][2][k]), np.asarray(res[1][step][2][k]), err_msg='slot of ' + k)
    moved = [k for k in ref[0][2] if np.any(np.asarray(ref[1][1][k]) != np.asarray(ref[0][1][k]))]
    assert len(moved) > 3                                  # the second step did train
    print('\nworst error / bound, %s: %s' % (label, ', '.join('%s %.3g' % kv for kv in sorted(worst.items(), key=lambda kv: -kv[1]))))


@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('mode', ['gather', 'dense'])
def test_data_parallel_world2_equals_one_engine(mode, opt):
    """mode='dense' must take the all-gather route for these optimizers (the worker checks that the dense-image half never
    runs) and give the same result."""
    res = H._run(_dp_worker, 2, mode, opt)
    _against_single(res, _single(opt), opt, False, 'DataParallelStep %s %s' % (mode, opt))


@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('wide', [False, True])
def test_row_sharded_world2_equals_one_engine(wide, opt):
    res = H._run(_sharded_worker, 2, opt, wide)
    _against_single(res, _single(opt, wide), opt, True, 'ShardedStep %s %s' % ('wide' if wide else 'narrow', opt))


def _class_worker(rank, world, tmp, tables):
    """tests/test_gpu_dist.py::_cffm_class_worker with MomentumOptimizer, replicated or row-sharded tables."""
    from cffm_amd import CFFM as M
    from tests.test_sharded_class_cpu import _data, _model
    if tables == 'sharded':
        os.environ['CFFM_TABLES'] = 'sharded'
    try:
        data, Mf, F = _data()
        m = _model(os.path.join(tmp, 'g%d_w%d' % (rank, world)), Mf, F, optimizer='MomentumOptimizer', rng=np.random.RandomState(77))
        m.train(data)
        assert m.world == world and ((m._dp is not None) or (m._sh is not None)) == (world > 1)
        refused = None
        if world > 1:
            try:
                _model(os.path.join(tmp, 'adam'), Mf, F, optimizer='AdamOptimizer').build_graph()
            except ValueError as e:
                refused = str(e)
        return (m.train_rmse, m.valid_rmse, m.test_rmse), m.engine.export_params(), refused
    finally:
        os.environ.pop('CFFM_TABLES', None)


@pytest.mark.parametrize('tables', ['replicated', 'sharded'])
def test_cffm_class_trains_momentum_at_world2(tables, tmp_path):
    """The drop-in class with its real HipEngine and --optimizer MomentumOptimizer under a world-2 group; AdamOptimizer is still
    refused by name before the first step."""
    one = H._run(_class_worker, 1, str(tmp_path), tables)[0]
    two = H._run(_class_worker, 2, str(tmp_path), tables)
    for rank in (0, 1):
        assert two[rank][2] is not None and 'AdamOptimizer' in two[rank][2]
    for a, b in zip(two[0][0], two[1][0]):                   # per-epoch metrics: the SAME numbers on both ranks
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    for a, b in zip(one[0], two[0][0]):                      # and the single-process run's, up to fp32 summation order over two
        np.testing.assert_allclose(np.asarray(a), np.asarray(b), rtol=2e-2, atol=2e-3)   # free-running epochs
        assert np.isfinite(np.asarray(b)).all()
    if tables == 'replicated':
        for k in two[0][1]:
            np.testing.assert_array_equal(np.asarray(two[0][1][k]), np.asarray(two[1][1][k]), err_msg=k)


# ---- HIP-graph capture ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def nccl_world1():
    import torch.distributed as dist
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29547')
    created = not dist.is_initialized()
    if created:
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    yield
    if created:
        dist.destroy_process_group()


@pytest.mark.parametrize('opt', OPTS)
def test_captured_step_equals_an_eager_twin(nccl_world1, opt):
    """use_graph=True: two eager warm-up calls, the capture on the third (replayed at once), one more replay; after every call
    the state equals an eager twin's bit for bit - the new apply launches the same way on capture and on replay, with no host
    reads."""
    from cffm_amd.dist import DataParallelStep
    from cffm_amd.engine import HipEngine
    cfg, X, y = _case(opt)
    p = init_params(cfg, seed=7)
    eng_g, eng_e = HipEngine(cfg, params=p), HipEngine(cfg, params=p)
    dp_g, dp_e = DataParallelStep(eng_g, use_graph=True), DataParallelStep(eng_e, use_graph=False)
    rng = np.random.default_rng(3)
    B = 128
    yt = torch.from_numpy(y[0, :B].copy()).cuda()
    for call in range(4):
        ids = torch.from_numpy(rng.integers(0, cfg.M, size=(B, cfg.F)).astype(np.int32)).cuda()
        lg, le = dp_g.train_step(ids, yt), dp_e.train_step(ids, yt)
        torch.cuda.synchronize()
        st = next(iter(dp_g._graphs.values()))
        assert (st['graph'] is not None) == (call >= 2), call
        assert float(lg) == float(le), call
        for a, b in ((eng_g.export_params(), eng_e.export_params()), (eng_g.export_accumulators(), eng_e.export_accumulators())):
            for k in a:
                np.testing.assert_array_equal(a[k], b[k], err_msg='call %d %s' % (call, k))
    assert np.any(eng_g.export_accumulators()['bias_W'] != 0) == (opt == 'MomentumOptimizer')
