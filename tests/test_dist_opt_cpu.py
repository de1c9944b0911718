"""SGD and Momentum under a process group, on the CPU: world-2 / world-4 gloo runs of cffm_amd.dist with the float64 oracle as the
per-rank compute (the stand-ins of tests/test_dist_cpu.py and tests/test_sharded_class_cpu.py, with a dp_apply that runs
oracle.apply_optimizer on the late-scaled gradients), against the single-process oracle step on the whole batch.

Two steps: the first has cross-rank duplicate ids (H._case()), the second only ids the first did not look up - so the rows of
step 1 and their Momentum slots must come out of step 2 bit-identical (TF does not decay the accumulator of a row nobody looked
up).  Tolerances are those of test_data_parallel_step_equals_single_process_step: loss 1e-12, parameters rtol 1e-10 / atol 1e-12,
replicas bit-identical."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import cffm_oracle as orc
from tests import test_dist_cpu as H
from tests import test_sharded_class_cpu as S

TABLES = S.TABLES
OPTS = ['GradientDescentOptimizer', 'MomentumOptimizer']


class _OptRule(object):
    """dp_apply / train_step of the stand-ins for the optimizers of oracle.apply_optimizer; self.acc is the first slot (zeros at
    the start for SGD and Momentum, as HipEngine's theta_acc / tables_acc)."""

    def _zero_slots(self):
        if self.cfg.optimizer != 'AdagradOptimizer':
            self.acc = {k: np.zeros_like(v) for k, v in self.p.items()}

    def dp_apply(self, grad, rows_all, Bg):
        g = grad.numpy()
        n = sum(self.sizes)
        L = np.sqrt(g[n] / Bg + 1e-10)
        gd, o = {}, 0
        for k, sz in zip(self.names, self.sizes):
            gd[k] = (g[o:o + sz] / L).reshape(np.shape(self.p[k]))
            o += sz
        r = rows_all.numpy()
        K, D = self.cfg.K, self.cfg.D
        gd['d_inner_rows'], gd['d_outer_rows'], gd['d_bias_rows'] = r[:, 1:1 + K] / L, r[:, 1 + K:1 + K + D] / L, r[:, 1 + K + D:] / L
        orc.apply_optimizer(self.p, {'acc': self.acc}, gd, r[:, 0].astype(np.int64), self.cfg)
        return torch.tensor([L])

    def train_step(self, ids, y):
        L, _ = orc.train_step_opt(self.p, {'acc': self.acc}, ids.numpy(), y.numpy().astype(np.float64), self.cfg)
        return torch.tensor([L])


class OptCompute(_OptRule, H.OracleCompute):
    def __init__(self, cfg, p):
        H.OracleCompute.__init__(self, cfg, p)
        self._zero_slots()


class DenseOptCompute(_OptRule, H.DenseOracleCompute):
    """A compute that offers the dense-image route; HipEngine.dp_dense_ok answers False for these optimizers, and so does this."""

    def __init__(self, cfg, p):
        H.DenseOracleCompute.__init__(self, cfg, p)
        self._zero_slots()

    def dp_dense_ok(self, B, world):
        return self.cfg.optimizer == 'AdagradOptimizer'


class ShardedOptCompute(_OptRule, H.ShardedOracleCompute):
    def __init__(self, cfg, p):
        H.ShardedOracleCompute.__init__(self, cfg, p)
        self._zero_slots()


def _case(opt):
    """H._case() with the optimizer set and a second batch drawn from the ids the first never looks up."""
    cfg, p, X, y = H._case()
    cfg.optimizer = opt
    free = np.setdiff1d(np.arange(cfg.M), X.reshape(-1))
    assert free.size >= 8
    X2 = np.random.default_rng(9).choice(free, size=X.shape)
    X2[6] = X2[1]                                # cross-rank duplicates in step 2 as well
    return cfg, p, X, X2, y


def _snap(comp):
    return {k: np.array(v, dtype=np.float64) for k, v in comp.p.items()}, {k: np.array(v, dtype=np.float64) for k, v in comp.acc.items()}


def _two_steps(step, comp, X, X2, y, rank, world):
    per = X.shape[0] // world
    sl = slice(rank * per, rank * per + per)
    yt = torch.from_numpy(y[sl])
    l1 = step.train_step(torch.from_numpy(X[sl].copy()), yt)
    s1 = _snap(comp)
    l2 = step.train_step(torch.from_numpy(X2[sl].copy()), yt)
    return (float(l1[0]), float(l2[0])), s1, _snap(comp)


def _dp_worker(rank, world, opt, dense):
    from cffm_amd.dist import DataParallelStep, replicas_agree
    cfg, p, X, X2, y = _case(opt)
    comp = (DenseOptCompute if dense else OptCompute)(cfg, p)
    step = DataParallelStep(comp, mode='dense' if dense else 'auto')
    out = _two_steps(step, comp, X, X2, y, rank, world)
    assert replicas_agree(comp, tables=True)
    return out


def _sharded_worker(rank, world, opt):
    from cffm_amd.dist import ShardedStep, local_rows_count, replicas_agree, shard_params
    cfg, p, X, X2, y = _case(opt)
    lcfg = copy.copy(cfg)
    lcfg.M = local_rows_count(cfg.M, rank, world)
    comp = ShardedOptCompute(lcfg, shard_params(p, rank, world))
    out = _two_steps(ShardedStep(comp), comp, X, X2, y, rank, world)
    assert replicas_agree(comp, tables=False)
    return out


def _reference(opt):
    cfg, p, X, X2, y = _case(opt)
    st = orc.init_opt_state(p, opt)
    L1, _ = orc.train_step_opt(p, st, X, y, cfg)
    L2, _ = orc.train_step_opt(p, st, X2, y, cfg)
    acc = st.get('acc', {k: np.zeros_like(v) for k, v in p.items()})
    return (L1, L2), p, acc, np.unique(X)


def _check(res, world, opt, sharded):
    (L1, L2), p, acc, touched = _reference(opt)
    for rank in range(world):
        (l1, l2), (p1, a1), (p2, a2) = res[rank]
        assert abs(l1 - L1) < 1e-12 and abs(l2 - L2) < 1e-12, (rank, l1 - L1, l2 - L2)
        for k in p2:
            shard = sharded and k in TABLES
            rp, ra = (p[k][rank::world], acc[k][rank::world]) if shard else (p[k], acc[k])
            np.testing.assert_allclose(p2[k], rp, rtol=1e-10, atol=1e-12, err_msg='rank %d %s' % (rank, k))
            np.testing.assert_allclose(a2[k], ra, rtol=1e-10, atol=1e-12, err_msg='rank %d slot %s' % (rank, k))
            if k in TABLES:
                # the rows of step 1 (local rows of this rank's shard when sharded): untouched by step 2, slot included
                rows = touched[touched % world == rank] // world if sharded else touched
                assert rows.size > 0
                np.testing.assert_array_equal(p2[k][rows], p1[k][rows], err_msg='rank %d %s moved in step 2' % (rank, k))
                np.testing.assert_array_equal(a2[k][rows], a1[k][rows], err_msg='rank %d slot %s moved in step 2' % (rank, k))
                if opt == 'MomentumOptimizer':
                    assert np.any(a1[k][rows] != 0)          # there was an accumulator to decay
                assert np.any(p2[k] != p1[k])                # and step 2 did move other rows
    for rank in range(1, world):                             # replicas stay bit-identical
        for k in res[0][2][0]:
            if not (sharded and k in TABLES):
                np.testing.assert_array_equal(res[0][2][0][k], res[rank][2][0][k], err_msg=k)
                np.testing.assert_array_equal(res[0][2][1][k], res[rank][2][1][k], err_msg='slot ' + k)


@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('world', [2, 4])
def test_data_parallel_two_steps_equal_the_single_process_steps(world, opt):
    _check(H._run(_dp_worker, world, opt, False), world, opt, sharded=False)


@pytest.mark.parametrize('opt', OPTS)
def test_mode_dense_falls_through_to_the_gather_route(opt):
    """mode='dense' with a compute whose dp_dense_ok refuses the optimizer: the all-gather route runs and gives the same result."""
    _check(H._run(_dp_worker, 2, opt, True), 2, opt, sharded=False)


@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('world', [2, 4])
def test_row_sharded_two_steps_equal_the_single_process_steps(world, opt):
    _check(H._run(_sharded_worker, world, opt), world, opt, sharded=True)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _refuse_worker(rank, world):
    from cffm_amd.dist import DataParallelStep, ShardedStep, shard_params
    out = {}
    for opt in ('AdamOptimizer', 'FtrlOptimizer'):
        cfg, p, _, _, _ = _case(opt)
        for cls, comp in ((DataParallelStep, OptCompute(cfg, p)), (ShardedStep, ShardedOptCompute(cfg, shard_params(p, rank, world)))):
            try:
                cls(comp)
            except ValueError as e:
                out[(opt, cls.__name__)] = str(e)
            else:
                out[(opt, cls.__name__)] = None
    return out


def test_adam_and_unknown_optimizers_are_still_refused_by_name():
    res = H._run(_refuse_worker, 2)
    for rank in range(2):
        assert len(res[rank]) == 4
        for (opt, who), msg in res[rank].items():
            assert msg is not None and opt in msg and who in msg, (rank, opt, who, msg)


# ---- the drop-in class -------------------------------------------------------------------------------------------------------
class OptOracleEngine(_OptRule, H.OracleEngine):
    def __init__(self, cfg, seed):
        H.OracleEngine.__init__(self, cfg, seed)
        self._zero_slots()


class ShardedOptOracleEngine(_OptRule, S.ShardedOracleEngine):
    def __init__(self, cfg, seed, rank, world, M_global):
        S.ShardedOracleEngine.__init__(self, cfg, seed, rank, world, M_global)
        self._zero_slots()


def _class_worker(rank, world, tmp):
    """tests/test_dist_cpu.py::_cffm_class_worker with MomentumOptimizer: replicated tables."""
    from cffm_amd import CFFM as M
    data, Mf, F = S._data()
    M.CFFM.engine_factory = OptOracleEngine
    try:
        m = S._model(os.path.join(tmp, 'r%d_w%d' % (rank, world)), Mf, F, optimizer='MomentumOptimizer', rng=np.random.RandomState(77))
        m.train(data)
    finally:
        M.CFFM.engine_factory = None
    assert m.world == world and (m._dp is not None) == (world > 1) and m.engine.cfg.optimizer == 'MomentumOptimizer'
    return (m.train_rmse, m.valid_rmse, m.test_rmse, m.train_r2), m.engine.export_params(), {k: np.array(v) for k, v in m.engine.acc.items()}


def test_cffm_class_trains_momentum_data_parallel_like_world1(tmp_path):
    one = H._run(_class_worker, 1, str(tmp_path))[0]
    two = H._run(_class_worker, 2, str(tmp_path))
    assert any(np.any(v != 0) for v in one[2].values()) and np.isfinite(np.asarray(one[0])).all()
    for rank in (0, 1):
        for a, b in zip(one[0], two[rank][0]):
            np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12)
        for k, v in one[1].items():
            np.testing.assert_allclose(two[rank][1][k], v, rtol=1e-8, atol=1e-11, err_msg='rank %d %s' % (rank, k))
            np.testing.assert_allclose(two[rank][2][k], one[2][k], rtol=1e-8, atol=1e-11, err_msg='rank %d slot %s' % (rank, k))
    for k in two[0][1]:
        np.testing.assert_array_equal(two[0][1][k], two[1][1][k], err_msg=k)
        np.testing.assert_array_equal(two[0][2][k], two[1][2][k], err_msg='slot ' + k)


def _with_stand_in(fn):
    from cffm_amd import CFFM as M
    os.environ['CFFM_TABLES'] = 'sharded'
    M.CFFM.sharded_engine_factory = ShardedOptOracleEngine
    try:
        return fn()
    finally:
        M.CFFM.sharded_engine_factory = None
        del os.environ['CFFM_TABLES']


def _sharded_class_worker(rank, world, tmp):
    """Two uninterrupted epochs against one epoch + save + restore + one epoch (tests/test_sharded_class_cpu.py::_checkpoint_worker)
    with MomentumOptimizer; the restore must bring the Momentum slots of this rank's shard back."""
    def run():
        out = {}
        data, Mf, F = S._data()
        kw = dict(optimizer='MomentumOptimizer')
        a = S._model(os.path.join(tmp, 'full%d' % world), Mf, F, epochs=2, pretrain=-1 if world > 1 else 0, rng=np.random.RandomState(77), **kw)
        a.train(data)                                    # (at world 2 every epoch also writes the shards)
        assert a.world == world and (a._sh is not None) == (world > 1)
        out['full'] = (a.engine.export_params(), a.engine.export_accumulators(), (a.train_rmse, a.valid_rmse, a.test_rmse))
        if world == 1:
            return out
        data, Mf, F = S._data()
        rng = np.random.RandomState(77)
        b1 = S._model(os.path.join(tmp, 'half'), Mf, F, epochs=1, pretrain=-1, rng=rng, **kw)
        b1.train(data)
        b2 = S._model(os.path.join(tmp, 'half'), Mf, F, epochs=1, pretrain=1, rng=rng, **kw)
        b2.build_graph()
        saved, restored = b1.engine.export_accumulators(), b2.engine.export_accumulators()
        assert any(np.any(saved[k] != 0) for k in TABLES)
        for k, v in saved.items():
            np.testing.assert_array_equal(restored[k], v, err_msg='slot ' + k)
        for k, v in b1.engine.export_params().items():
            np.testing.assert_array_equal(b2.engine.export_params()[k], v, err_msg=k)
        b2.train(data)
        out['resumed'] = (b2.engine.export_params(), b2.engine.export_accumulators(), (b2.train_rmse[-1], b2.valid_rmse[-1], b2.test_rmse[-1]))
        return out
    return _with_stand_in(run)


def test_cffm_class_trains_momentum_row_sharded_saves_and_resumes(tmp_path):
    one = H._run(_sharded_class_worker, 1, str(tmp_path))[0]['full']
    two = H._run(_sharded_class_worker, 2, str(tmp_path))
    for rank in (0, 1):
        full, resumed = two[rank]['full'], two[rank]['resumed']
        for a, b in zip(one[2], full[2]):                                   # world 2 equals world 1: metrics, parameters, slots
            np.testing.assert_allclose(b, a, rtol=1e-9, atol=1e-12, err_msg='rank %d' % rank)
        for which in (0, 1):
            for k, v in full[which].items():
                ref = one[which][k][rank::2] if k in TABLES else one[which][k]
                np.testing.assert_allclose(v, ref, rtol=1e-8, atol=1e-11, err_msg='rank %d %s %s' % (rank, ('', 'slot')[which], k))
            for k in full[which]:                                           # the resumed run reaches the uninterrupted run's state
                np.testing.assert_allclose(resumed[which][k], full[which][k], rtol=1e-12, atol=1e-15, err_msg='rank %d %s' % (rank, k))
        np.testing.assert_allclose(resumed[2], [m[-1] for m in full[2]], rtol=1e-9, atol=1e-12)
