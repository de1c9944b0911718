"""cffm_amd.CFFM with CFFM_TABLES=sharded on the CPU: world-2 / world-4 gloo runs of the drop-in class against the SAME class at
world size 1.  The collectives, the routing, the forward-only path (ShardedStep.predict / eval_sums), the matched rounds of a
ragged evaluate, the sharded checkpoints and merge_shards are the product's; the per-rank compute is the float64 oracle over a
shard that spec.table_rows draws by global row (the twin of cffm_init_table_rows), plugged in through
CFFM.sharded_engine_factory.  So the comparison is tight: a run at world N and the run at world 1 are the same model in float64.

The small case is the one of tests/test_dist_cpu.py::test_cffm_class_trains_data_parallel_under_a_process_group (M 40, F 4, two
epochs, batch 8, pinned block starts) and the tolerances are that test's: metrics rtol 1e-9 / atol 1e-12, tables rtol 1e-8 /
atol 1e-11.  The spawn harness' 180 s queue timeout is what a hang (unmatched all-to-alls) would run into."""
import os

import numpy as np
import pytest
import torch

from cffm_amd.spec import init_params, table_rows
from oracle import cffm_oracle as orc
from tests import test_dist_cpu as H

TABLES = ('inner_embeddings', 'outer_embeddings', 'feature_bias')


class ShardedOracleEngine(H.ShardedOracleCompute):
    """What cffm_amd.CFFM and cffm_amd.dist.ShardedStep need from HipEngine(params='device_rows'), computed by the float64
    oracle: local row l holds global row rank + l * world of the by-row draw; one dense seed."""
    device = torch.device('cpu')
    opt_step = 0

    def __init__(self, cfg, seed, rank, world, M_global):
        assert cfg.M == len(range(rank, M_global, world))
        p = init_params(cfg, seed=seed, dtype=np.float64, tables=False)
        p.update(table_rows(cfg, seed, rank + world * np.arange(cfg.M), dtype=np.float64))
        H.ShardedOracleCompute.__init__(self, cfg, p)

    # ---- the forward-only half of the step interface ----
    def forward_staged(self, y, B):
        H.ShardedOracleCompute.forward_staged(self, torch.zeros(B, dtype=torch.float64) if y is None else y, B)

    def predictions(self, B):
        assert self.out.shape == (B,)
        return torch.from_numpy(np.array(self.out, dtype=np.float64))

    def eval_sums_add(self, pred, y, lo, hi, sums):
        yt = y.numpy().astype(np.float64)
        pr = np.minimum(np.maximum(pred.numpy(), lo), hi)
        sums += torch.tensor([np.sum((yt - pr) ** 2), yt.sum(), np.sum(yt * yt)], dtype=torch.float64)
        return sums

    # ---- the single-process surface (world size 1) ----
    train_step = H.OracleEngine.train_step
    eval_sums = H.OracleEngine.eval_sums

    def predict(self, ids):
        return torch.from_numpy(orc.forward(self.p, ids.numpy(), self.cfg)[0])

    # ---- checkpoints ----
    def export_params(self):
        return {k: np.asarray(v, dtype=np.float64).copy() for k, v in self.p.items()}

    def export_accumulators(self):
        return {k: np.asarray(v, dtype=np.float64).copy() for k, v in self.acc.items()}

    def load_params(self, params, accs=None, accs2=None):
        self.p = {k: np.array(v, dtype=np.float64) for k, v in params.items()}
        if accs is not None:
            self.acc = {k: np.array(accs[k], dtype=np.float64) for k in self.acc}


class _Split(dict):
    pass


class _Data(object):
    pass


def _data(sizes=(37, 11, 9)):
    from cffm_amd import synth
    rng = np.random.default_rng(11)
    Mf, F = 40, 4
    data = _Data()
    splits = [_Split(X=synth.sample_ids(rng, Mf, F, n).tolist(), Y=synth.sample_labels(rng, n).tolist()) for n in sizes]
    data.Train_data, data.Validation_data, data.Test_data = splits
    return data, Mf, F


def _model(save_file, Mf, F, epochs=2, pretrain=0, batch=8, optimizer='AdagradOptimizer', loss='square_loss', lamda=0, rng=None):
    from cffm_amd import CFFM as M
    return M.CFFM(Mf, pretrain, save_file, 8, 8, loss, epochs, batch, 0.05, lamda, [1.0, 1.0], optimizer, 0, 0, 0, F, 1, 0, 1.0, 1,
                  1.0, 1, 1.0, 'relu', batch_rng=rng)


def _with_stand_in(fn):
    from cffm_amd import CFFM as M
    os.environ['CFFM_TABLES'] = 'sharded'
    M.CFFM.sharded_engine_factory = ShardedOracleEngine
    try:
        return fn()
    finally:
        M.CFFM.sharded_engine_factory = None
        del os.environ['CFFM_TABLES']


def _train_worker(rank, world, tmp, sizes):
    def run():
        data, Mf, F = _data(sizes)
        m = _model(os.path.join(tmp, 'w%d' % world), Mf, F, rng=np.random.RandomState(77))     # the block starts, pinned
        m.train(data)
        assert m.world == world and (m._sh is not None) == (world > 1) and m._dp is None
        assert m.engine.cfg.M == len(range(rank, Mf, world)) and m.config.M == Mf
        assert m.calculate_parameters() == _model(os.path.join(tmp, 'count'), Mf, F).calculate_parameters()   # the GLOBAL model's count
        preds = [m.predict_split(s) for s in (data.Train_data, data.Validation_data, data.Test_data)]
        again = [m.evaluate(s) for s in (data.Train_data, data.Validation_data, data.Test_data)]
        reused = m._sh.plans_reused if m._sh is not None else None
        return (m.train_rmse, m.valid_rmse, m.test_rmse, m.train_r2, m.valid_r2, m.test_r2), m.engine.export_params(), preds, again, reused
    return _with_stand_in(run)


def _check_against_world1(one, many, world):
    for rank in range(world):
        metrics, params, preds, again, reused = many[rank]
        for a, b in zip(one[0], metrics):                    # per-epoch metrics: equal to the single-process run ...
            np.testing.assert_allclose(b, a, rtol=1e-9, atol=1e-12, err_msg='rank %d' % rank)
        for a, b in zip(many[0][0], metrics):                # ... and IDENTICAL on every rank (early stopping fires everywhere at once)
            assert list(a) == list(b), rank
        assert again == many[0][3]
        for k, v in params.items():
            if k in TABLES:                                  # this rank's shard = rows rank::world of the single-process tables
                np.testing.assert_allclose(v, one[1][k][rank::world], rtol=1e-8, atol=1e-11, err_msg='rank %d %s' % (rank, k))
            else:                                            # dense parameters: bit-identical replicas
                np.testing.assert_array_equal(v, many[0][1][k], err_msg='rank %d %s' % (rank, k))
                np.testing.assert_allclose(v, one[1][k], rtol=1e-8, atol=1e-11, err_msg='rank %d %s' % (rank, k))
        for s, (p1, pn) in enumerate(zip(one[2], preds)):    # predict_split: the WHOLE split, the same array on every rank
            assert pn.shape == p1.shape and pn.dtype == np.float64
            np.testing.assert_array_equal(pn, many[0][2][s])
            np.testing.assert_allclose(pn, p1, rtol=1e-9, atol=1e-12)
        assert reused > 0                                    # the routing plans ran one step ahead


@pytest.mark.parametrize('world', [2, 4])
def test_cffm_class_trains_row_sharded_like_world1(world, tmp_path):
    sizes = (37, 11, 9)
    one = H._run(_train_worker, 1, str(tmp_path), sizes)[0]
    assert one[4] is None
    many = H._run(_train_worker, world, str(tmp_path), sizes)
    _check_against_world1(one, many, world)
    # the world-1 twin really is the by-row draw moved by training, not init_params' tables
    assert one[1]['inner_embeddings'].shape == (40, 8)


def test_ragged_evaluate_with_a_rank_that_owns_no_row_of_a_split(tmp_path):
    """Split sizes 37 / 11 / 1 at world 4: ranks 1..3 have no row of the test split (and rank 3 has 2 of the 11 validation rows
    against 3 elsewhere).  They take part in every round with empty blocks; nothing hangs, the metrics are world 1's."""
    sizes = (37, 11, 1)
    one = H._run(_train_worker, 1, str(tmp_path), sizes)[0]
    many = H._run(_train_worker, 4, str(tmp_path), sizes)
    _check_against_world1(one, many, 4)
    assert many[3][2][2].shape == (1,)


def _checkpoint_worker(rank, world, tmp):
    """Uninterrupted two epochs against one epoch + save + restore + one epoch, at the same world size.  The second half
    continues on the SAME data object (train() leaves the split in its shuffled order) and the same stream of block starts."""
    def run():
        out = {}
        data, Mf, F = _data()
        a = _model(os.path.join(tmp, 'full'), Mf, F, epochs=2, pretrain=-1, rng=np.random.RandomState(77))
        a.train(data)
        out['full'] = (a.engine.export_params(), a.engine.export_accumulators(), (a.train_rmse[-1], a.valid_rmse[-1], a.test_rmse[-1]),
                       [a.evaluate(s) for s in (data.Train_data, data.Validation_data, data.Test_data)])
        data, Mf, F = _data()
        rng = np.random.RandomState(77)
        b1 = _model(os.path.join(tmp, 'half'), Mf, F, epochs=1, pretrain=-1, rng=rng)
        b1.train(data)
        b2 = _model(os.path.join(tmp, 'half'), Mf, F, epochs=1, pretrain=1, rng=rng)
        b2.build_graph()
        restored = b2.engine.export_params()
        for k, v in b1.engine.export_params().items():
            np.testing.assert_array_equal(restored[k], v, err_msg=k)
        b2.train(data)
        out['resumed'] = (b2.engine.export_params(), b2.engine.export_accumulators(), (b2.train_rmse[-1], b2.valid_rmse[-1], b2.test_rmse[-1]))
        return out
    return _with_stand_in(run)


def _merged_worker(rank, world, tmp):
    def run():
        from cffm_amd.dist import merge_shards
        data, Mf, F = _data()
        merged = merge_shards(os.path.join(tmp, 'full'), 2, os.path.join(tmp, 'merged'))
        blob = torch.load(merged, weights_only=True)                          # plain tensors
        assert blob['config'] == {'M': Mf, 'F': F, 'K': 8, 'D': 8} and blob['params']['inner_embeddings'].shape == (Mf, 8)
        m = _model(os.path.join(tmp, 'merged'), Mf, F, pretrain=1)
        m.build_graph()
        assert m.world == 1 and m._sh is None
        return [m.evaluate(s) for s in (data.Train_data, data.Validation_data, data.Test_data)], m.engine.export_params()
    return _with_stand_in(run)


def test_sharded_checkpoints_resume_and_merge_to_world1(tmp_path):
    res = H._run(_checkpoint_worker, 2, str(tmp_path))
    for rank in (0, 1):
        full, resumed = res[rank]['full'], res[rank]['resumed']
        for a, b in zip(full[:2], resumed[:2]):                # parameters and Adagrad slots: the state an uninterrupted run reaches
            for k in a:
                np.testing.assert_allclose(b[k], a[k], rtol=1e-12, atol=1e-15, err_msg='rank %d %s' % (rank, k))
        np.testing.assert_allclose(resumed[2], full[2], rtol=1e-9, atol=1e-12)
    for name in ('full', 'half'):
        for r in (0, 1):
            assert os.path.exists(os.path.join(str(tmp_path), '%s.shard%d-of-2.pt' % (name, r)))
    # train on 2, load on one: the merged checkpoint in a world-1 class evaluates to the same metrics (RMSE and R2 do not depend
    # on the order of a split's rows)
    evals, params = H._run(_merged_worker, 1, str(tmp_path))[0]
    np.testing.assert_allclose(np.asarray(evals), np.asarray(res[0]['full'][3]), rtol=1e-9, atol=1e-12)
    for k in TABLES:
        for r in (0, 1):
            np.testing.assert_array_equal(params[k][r::2], res[r]['full'][0][k], err_msg=k)


def _refusal_worker(rank, world, tmp):
    def run():
        _, Mf, F = _data()
        out = {}
        for what, kw in (('AdamOptimizer', dict(optimizer='AdamOptimizer')), ('hybrid', dict(loss='hybrid')), ('lamda', dict(lamda=0.01)),
                         ('batch_size', dict(batch=9))):
            m = _model(os.path.join(tmp, 'refuse'), Mf, F, **kw)
            try:
                m.build_graph()
            except ValueError as e:
                out[what] = str(e)
            else:
                out[what] = None
        return out
    return _with_stand_in(run)


def test_sharded_class_refuses_what_the_sharded_step_does_not_implement(tmp_path):
    res = H._run(_refusal_worker, 2, str(tmp_path))
    for rank in (0, 1):
        for what, msg in res[rank].items():
            assert msg is not None and what in msg, (rank, what, msg)


def test_replicated_stays_the_default(tmp_path, monkeypatch):
    """Without CFFM_TABLES (or with 'replicated') build_graph() takes the path it always took: the engine comes from engine_factory
    and the sharded hook is not consulted."""
    from cffm_amd import CFFM as M
    _, Mf, F = _data()
    called = []
    monkeypatch.setattr(M.CFFM, 'sharded_engine_factory', lambda *a: called.append(a))
    monkeypatch.setattr(M.CFFM, 'engine_factory', H.OracleEngine)
    for env in (None, 'replicated'):
        if env is None:
            monkeypatch.delenv('CFFM_TABLES', raising=False)
        else:
            monkeypatch.setenv('CFFM_TABLES', env)
        m = _model(str(tmp_path / 'plain'), Mf, F)
        assert isinstance(m.build_graph(), H.OracleEngine) and m._sh is None and not called


def _typo_worker(rank, world, tmp):
    from cffm_amd import CFFM as M
    _, Mf, F = _data()
    os.environ['CFFM_TABLES'] = 'Sharded'
    M.CFFM.engine_factory = H.OracleEngine
    try:
        _model(os.path.join(tmp, 'typo'), Mf, F).build_graph()
    except ValueError as e:
        return str(e)
    finally:
        M.CFFM.engine_factory = None
        del os.environ['CFFM_TABLES']
    return None


def test_an_unknown_table_mode_is_refused_by_name(tmp_path):
    res = H._run(_typo_worker, 2, str(tmp_path))
    for rank in (0, 1):
        assert res[rank] is not None and "'Sharded'" in res[rank] and "'sharded'" in res[rank] and "'replicated'" in res[rank]
