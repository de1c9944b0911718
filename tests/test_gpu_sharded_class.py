"""Row-sharded tables through the public surface, ON THE GPU: the by-global-row draw (cffm_init_table_rows) against its numpy twin,
ShardedStep's forward-only path at world size 2 (two ranks on cuda:0 over gloo, the rehearsal of tests/test_gpu_dist.py), the
drop-in class with CFFM_TABLES=sharded and its real engine against the same class at world size 1, and one GPU's share of
config 5 through the forward-only path over RCCL loopback.  The world-2 tests spawn two ranks, one after the other world size, as
tests/test_gpu_dist.py does: with the pytest process itself, which has opened the GPU for the kernel tests, three processes hold it.

The kernel's bound.  The draw is integer Philox (exact) followed by log, sqrt and sin / cos in float32.  The numpy twin evaluated
in float32 against itself in float64 ON THE SAME ROWS is what float32 evaluation costs with a libm that is a few ulps off; the
device may use a libm of its own that is allowed the same few ulps, so it is held to TWICE that floor, in standard deviations
of the table (the stored value divided by 0.1 or 0.01).  The measured figures go to init_table_rows_error.json under $CFFM_TEST_OUT
(default prof_out/) and are quoted in profiles/init_table_rows.md."""
import ctypes as C
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from cffm_amd import hip
from cffm_amd.spec import TABLE_STD, CFFMConfig, init_params, table_rows, table_words, unit_normals
from oracle import cffm_oracle as orc
from oracle.parity import close, to64
from tests import test_dist_cpu as H  # the spawn / gloo harness
from tests import test_gpu_dist as GD  # its world-2 cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = ('inner_embeddings', 'outer_embeddings', 'feature_bias')
BAD_SHAPE = 10001
GUARD = 8                     # rows behind every drawn table that must come back untouched


def _shape(M, K, D, inner_conv=1, outer_conv=1):
    return hip.Shape(M=M, F=32, K=K, D=D, act=0, linear_att=1, inner_conv=inner_conv, outer_conv=outer_conv, loss=0, lamda_att=1.0,
                     beta_outer=1.0, lr=0.05, lamda=0.0, optimizer=0)


class _Drawn(object):
    """Three device tables of n rows (+ GUARD rows), pre-filled with NaN / ones, drawn by cffm_init_table_rows."""

    def __init__(self, n, K, D):
        self.n, self.K, self.D = n, K, D
        self.inner = torch.full((n + GUARD, K), float('nan'), dtype=torch.float32, device='cuda')
        self.outer = torch.full((n + GUARD, D), float('nan'), dtype=torch.float32, device='cuda')
        self.fbias = torch.ones(n + GUARD, dtype=torch.float32, device='cuda')
        self.tab = hip.Tables(self.inner.data_ptr(), self.outer.data_ptr(), self.fbias.data_ptr())
        self.shape = _shape(n, K, D)

    def draw(self, seed, row0, row_step, n_rows=None):
        rc = hip.fast().cffm_init_table_rows(C.addressof(self.shape), C.addressof(self.tab), seed, row0, row_step,
                                             self.n if n_rows is None else n_rows, 0)
        torch.cuda.synchronize()
        return rc

    def check_written_and_guarded(self):
        n = self.n
        assert not bool(torch.isnan(self.inner[:n]).any()) and not bool(torch.isnan(self.outer[:n]).any())
        assert bool(torch.isnan(self.inner[n:]).all()) and bool(torch.isnan(self.outer[n:]).all())      # nothing past the last row
        assert not bool(self.fbias[:n].any()) and bool((self.fbias[n:] == 1).all())


def _errors_against_twin(dev, seed, rows, table, width, chunk=1 << 15):
    """(device error, twin float32 floor): max over ``rows`` of |stored / std - z64| for the device table ``dev`` [len(rows), width]
    and for the twin evaluated in float32, both against the twin in float64."""
    std = TABLE_STD[('inner_embeddings', 'outer_embeddings')[table]]

    def one(s):
        r = rows[s:s + chunk]
        words = table_words(seed, r, table, width)
        z64 = unit_normals(words, width, np.float64)
        t32 = unit_normals(words, width, np.float32) * np.float32(std)
        got = dev[s:s + chunk].cpu().numpy()
        assert got.dtype == np.float32 and t32.dtype == np.float32
        return (float(np.abs(got.astype(np.float64) / std - z64).max()), float(np.abs(t32.astype(np.float64) / std - z64).max()))
    with ThreadPoolExecutor(8) as pool:
        res = list(pool.map(one, range(0, len(rows), chunk)))
    return max(r[0] for r in res), max(r[1] for r in res)


def _record(key, value):
    out = os.path.join(ROOT, os.environ.get('CFFM_TEST_OUT', 'prof_out'))
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, 'init_table_rows_error.json')
    blob = json.load(open(path)) if os.path.exists(path) else {}
    blob[key] = value
    with open(path, 'w') as fh:
        json.dump(blob, fh, indent=1, sort_keys=True)


@pytest.mark.parametrize('K', [64, 34])
def test_rows_drawn_on_the_device_against_the_twin(K):
    """F 32, D 64, K 64 (16-byte stores) and K 34 (8-byte stores, the last group keeps two columns): 2^18 rows drawn as rank 3 of 8
    are rows 3::8 of the first 8 * 2^18 rows drawn by one process, bit for bit; both draws within twice the twin's own
    float32 floor of the float64 twin."""
    seed, D, n = 2021, 64, 1 << 18
    whole, shard = _Drawn(8 * n, K, D), _Drawn(n, K, D)
    assert whole.draw(seed, 0, 1) == 0 and shard.draw(seed, 3, 8) == 0
    whole.check_written_and_guarded()
    shard.check_written_and_guarded()
    assert torch.equal(shard.inner[:n], whole.inner[3:8 * n:8]) and torch.equal(shard.outer[:n], whole.outer[3:8 * n:8])
    fig = {}
    for name, rows, d in (('whole (0, 1)', np.arange(8 * n), whole), ('shard (3, 8)', 3 + 8 * np.arange(n), shard)):
        for t, (tab, width) in enumerate(((d.inner, K), (d.outer, D))):
            err, floor = _errors_against_twin(tab[:d.n], seed, rows, t, width)
            fig['%s table %d' % (name, t)] = {'device_err_sigma': err, 'twin_fp32_floor_sigma': floor}
            print('K %d %s table %d: device %.3e sigma, float32 twin %.3e sigma' % (K, name, t, err, floor))
    _record('K%d_D%d_rows_2^18' % (K, D), fig)
    for what, f in fig.items():
        assert f['device_err_sigma'] <= 2 * f['twin_fp32_floor_sigma'], (K, what, f)
    # another seed is another model
    again = _Drawn(n, K, D)
    assert again.draw(seed + 1, 3, 8) == 0 and not torch.equal(again.inner[:n], shard.inner[:n])


def test_rows_beyond_2_to_the_32_and_bad_arguments():
    seed, K, D, n = 5, 64, 64, 4096
    row0 = 2 ** 33 + 1
    far, near = _Drawn(n, K, D), _Drawn(n, K, D)
    assert far.draw(seed, row0, 3) == 0 and near.draw(seed, 1, 3) == 0           # the same low words of the counter
    far.check_written_and_guarded()
    assert not torch.equal(far.inner[:n], near.inner[:n])
    rows = row0 + 3 * np.arange(n, dtype=np.int64)
    fig = {}
    for t, (tab, width) in enumerate(((far.inner, K), (far.outer, D))):
        err, floor = _errors_against_twin(tab[:n], seed, rows, t, width)
        fig['table %d' % t] = {'device_err_sigma': err, 'twin_fp32_floor_sigma': floor}
        assert err <= 2 * floor, (t, err, floor)
    _record('rows_from_2^33+1', fig)
    # seeds use both key words
    hi = _Drawn(n, K, D)
    assert hi.draw(seed + 2 ** 32, row0, 3) == 0 and not torch.equal(hi.inner[:n], far.inner[:n])
    # bad arguments: CFFM_ERR_BAD_SHAPE and nothing written
    t = _Drawn(n, K, D)
    for args in ((-1, 1, n), (0, 0, n), (0, 1, -1), (0, 1, n + 1), (2 ** 62, 2 ** 62, n)):
        assert t.draw(seed, *args) == BAD_SHAPE, args
    lib = hip.fast()
    no_inner = hip.Tables(0, t.outer.data_ptr(), t.fbias.data_ptr())
    assert lib.cffm_init_table_rows(C.addressof(t.shape), C.addressof(no_inner), seed, 0, 1, n, 0) == BAD_SHAPE
    assert lib.cffm_init_table_rows(0, C.addressof(t.tab), seed, 0, 1, n, 0) == BAD_SHAPE
    odd = _shape(n, 33, D)
    assert lib.cffm_init_table_rows(C.addressof(odd), C.addressof(t.tab), seed, 0, 1, n, 0) == BAD_SHAPE
    assert t.draw(seed, 0, 1, 0) == 0                                               # n_rows == 0: fine, and no launch
    torch.cuda.synchronize()
    assert bool(torch.isnan(t.inner).all()) and bool(torch.isnan(t.outer).all()) and bool((t.fbias == 1).all())
    # a disabled branch: its table is not written (and may be NULL); fewer rows than the table holds
    off = _shape(n, K, D, outer_conv=0)
    only_inner = hip.Tables(t.inner.data_ptr(), 0, t.fbias.data_ptr())
    assert lib.cffm_init_table_rows(C.addressof(off), C.addressof(only_inner), seed, 1, 3, 100, 0) == 0
    torch.cuda.synchronize()
    assert torch.equal(t.inner[:100], near.inner[:100]) and bool(torch.isnan(t.inner[100:]).all()) and bool(torch.isnan(t.outer).all())
    assert not bool(t.fbias[:100].any()) and bool((t.fbias[100:] == 1).all())


def test_engine_device_rows_is_independent_of_the_sharding():
    from cffm_amd.engine import HipEngine
    cfg = CFFMConfig(M=1000, F=10, K=32, D=32)
    one = HipEngine(cfg, params='device_rows', seed=9).export_params()
    twin = table_rows(cfg, 9, np.arange(cfg.M), dtype=np.float32)
    dense = init_params(cfg, seed=9, tables=False)
    for r, G in ((0, 3), (2, 3)):
        lcfg = CFFMConfig(M=len(range(r, cfg.M, G)), F=10, K=32, D=32)
        eng = HipEngine(lcfg, params='device_rows', seed=9, table_rows=(r, G))
        part = eng.export_params()
        for k in TABLES:
            np.testing.assert_array_equal(part[k], one[k][r::G], err_msg=k)
        for k, v in dense.items():                                          # dense parameters: init_params(seed), as for 'device'
            np.testing.assert_array_equal(part[k], v.reshape(part[k].shape), err_msg=k)
        assert float(eng.inner_acc.min()) == float(eng.inner_acc.max()) == np.float32(1e-8)      # the slots are the engine's business
    np.testing.assert_allclose(one['inner_embeddings'], twin['inner_embeddings'], rtol=0, atol=1e-5 * 0.1)
    assert not one['feature_bias'].any()
    with pytest.raises(ValueError):
        HipEngine(cfg, params='device_row')


# ---- ShardedStep.predict / eval_sums at world size 2 ----------------------------------------------------------------------------
LO, HI = -0.02, 0.03          # a narrow clip range, so that the clip of cffm_eval_sums takes part


def _params(cfg):
    p = init_params(cfg, seed=7)
    rng = np.random.default_rng(3)
    p['feature_bias'] = (rng.standard_normal(p['feature_bias'].shape) * 0.3).astype(np.float32)
    return p


def _blocks(rank, X, y):
    """Rank 0 sweeps two blocks, rank 1 one: its second round is an EMPTY block."""
    per = X.shape[1] // 2
    if rank == 0:
        return np.concatenate([X[0, :per], X[1, :per]]), np.concatenate([y[0, :per], y[1, :per]]), per
    return X[0, per:], y[0, per:], per


def _predict_worker(rank, world, wide):
    from cffm_amd.dist import ShardedStep, local_rows_count, shard_params
    from cffm_amd.engine import HipEngine
    import copy
    cfg, X, y = GD._case(wide)
    lcfg = copy.copy(cfg)
    lcfg.M = local_rows_count(cfg.M, rank, world)
    eng = HipEngine(lcfg, params=shard_params(_params(cfg), rank, world), device='cuda:0')
    sh = ShardedStep(eng, M_global=cfg.M)
    assert eng.packed_ok() == wide
    Xr, yr, per = _blocks(rank, X, y)
    ids, yt = torch.from_numpy(Xr.copy()).cuda(), torch.from_numpy(yr.copy()).cuda()
    sums = sh.eval_sums(ids, yt, LO, HI, per, 2)
    preds = [sh.predict(ids[b * per:(b + 1) * per]) for b in range(2)]          # the same two rounds, one block at a time
    torch.cuda.synchronize()
    assert preds[1].shape[0] == (per if rank == 0 else 0) and preds[1].dtype == torch.float32
    with pytest.raises(ValueError):
        sh.eval_sums(ids, yt, LO, HI, per, 0)                                     # rows that do not fit the rounds: before any collective
    return torch.cat(preds).cpu().numpy(), sums.cpu().numpy()


@pytest.mark.parametrize('wide', [False, True])
def test_sharded_predict_and_eval_sums_world2_on_the_gpu(wide):
    """Two ranks on cuda:0 over gloo: the predictions of each rank's rows against the float64 oracle forward on the GLOBAL
    parameters (oracle/parity.py close(), default tolerance), narrow (staged) and wide (records read in place); eval_sums of the
    two ranks added up against float64 sums over those clipped predictions; rank 1's second round is an empty block."""
    res = H._run(_predict_worker, 2, wide)
    cfg, X, y = GD._case(wide)
    p64 = to64(_params(cfg))
    total, want = np.zeros(3), np.zeros(3)
    for rank in (0, 1):
        Xr, yr, per = _blocks(rank, X, y)
        pred, sums = res[rank]
        assert pred.shape == (Xr.shape[0],) and pred.dtype == np.float32
        ref, _ = orc.forward(p64, Xr, cfg)
        close(pred, ref, 'sharded predict world 2 %s rank %d' % ('wide' if wide else 'narrow', rank))
        clipped = np.minimum(np.maximum(pred, np.float32(LO)), np.float32(HI)).astype(np.float64)
        yt = yr.astype(np.float64)
        want += [np.sum((yt - clipped) ** 2), yt.sum(), np.sum(yt * yt)]
        total += sums
    np.testing.assert_allclose(total, want, rtol=1e-12, atol=0)


# ---- the drop-in class, CFFM_TABLES=sharded, real engine ----------------------------------------------------------------------
def _class_worker(rank, world, tmp):
    from cffm_amd import CFFM as M
    from cffm_amd import synth

    class Split(dict):
        pass

    rng = np.random.default_rng(11)
    Mf, F = 40, 4

    def split(n):
        return Split(X=synth.sample_ids(rng, Mf, F, n).tolist(), Y=synth.sample_labels(rng, n).tolist())

    class Data(object):
        pass
    data = Data()
    data.Train_data, data.Validation_data, data.Test_data = split(37), split(11), split(9)
    os.environ['CFFM_TABLES'] = 'sharded'
    try:
        m = M.CFFM(Mf, 0, os.path.join(tmp, 's%d_w%d' % (rank, world)), 8, 8, 'square_loss', 2, 8, 0.05, 0, [1.0, 1.0],
                   'AdagradOptimizer', 0, 0, 0, F, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'relu')
        np.random.seed(77)                                   # the reference's batch starts are unseeded: pin them for the test
        m.build_graph()
        first = m.engine.export_params()
        m.train(data)
        preds = m.predict_split(data.Test_data)
    finally:
        del os.environ['CFFM_TABLES']
    assert m.world == world and (m._sh is not None) == (world > 1) and m._dp is None
    reused = m._sh.plans_reused if m._sh is not None else None
    return (m.train_rmse, m.valid_rmse, m.test_rmse, m.train_r2), first, m.engine.export_params(), preds, reused


def test_cffm_class_trains_row_sharded_on_the_gpu(tmp_path):
    """The case of tests/test_gpu_dist.py::test_cffm_class_trains_data_parallel_on_the_gpu with CFFM_TABLES=sharded.  Every world
    size starts from the SAME model (tables drawn by global row); free-running fp32 epochs then differ by summation order, so the
    metrics are held to that test's rtol 2e-2 / atol 2e-3 (its header)."""
    one = H._run(_class_worker, 1, str(tmp_path))[0]
    two = H._run(_class_worker, 2, str(tmp_path))
    for rank in (0, 1):
        for k in TABLES:                                     # initial tables: bit-identical to rows rank::2 of the world-1 engine's
            np.testing.assert_array_equal(two[rank][1][k], one[1][k][rank::2], err_msg='rank %d %s' % (rank, k))
        assert two[rank][4] > 0
    for k in two[0][1]:
        if k not in TABLES:                                  # one dense seed, rank 0's state broadcast: identical replicas, before and after
            np.testing.assert_array_equal(two[0][1][k], one[1][k], err_msg=k)
            np.testing.assert_array_equal(two[0][1][k], two[1][1][k], err_msg=k)
            np.testing.assert_array_equal(two[0][2][k], two[1][2][k], err_msg=k)
    for a, b in zip(two[0][0], two[1][0]):                   # per-epoch metrics: the SAME numbers on both ranks
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    for a, b in zip(one[0], two[0][0]):
        np.testing.assert_allclose(np.asarray(a), np.asarray(b), rtol=2e-2, atol=2e-3)
    np.testing.assert_array_equal(two[0][3], two[1][3])      # predict_split: the whole split on every rank
    assert two[0][3].shape == one[3].shape == (9,)


# ---- one GPU's share of config 5 through the forward-only path, RCCL loopback ----------------------------------------------------
@pytest.fixture
def nccl_world1():
    import torch.distributed as dist
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29543')
    created = not dist.is_initialized()
    if created:
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    yield
    if created:
        dist.destroy_process_group()


def test_cfg5_share_forward_only_world1(nccl_world1):
    """Config 5 (10 M features, 32 fields, dim 64) has 1.25 M rows per GPU at world 8.  One process stands for rank 3 of 8: its
    engine holds global rows 3, 11, 19, ... drawn by row, and at world size 1 the routing r -> (r % 1, r // 1) sends every id to
    that one shard, so the ids of the batch ARE local rows.  ShardedStep.predict / eval_sums (plan, three all-to-alls over RCCL
    loopback, owner-side gather, the forward on the received records) against the engine's own replicated-table forward on the
    same ids, against the oracle on four examples, and the sums against float64 sums over the predictions.  What this does
    NOT show is anything at world size > 1 on RCCL: no multi-GPU node has been available.  CFFM.evaluate() itself cannot be the
    entry here: at world size 1 the class runs a plain engine (_sh is None) and never reaches the forward-only path, so the test
    calls what evaluate() calls at world size > 1, ShardedStep.eval_sums, directly."""
    from cffm_amd import synth
    from cffm_amd.dist import ShardedStep, local_rows_count
    from cffm_amd.engine import HipEngine
    M_global, world, rank = 10_000_000, 8, 3
    cfg = CFFMConfig(M=local_rows_count(M_global, rank, world), F=32, K=64, D=64, activation='relu')
    assert cfg.M == 1_250_000
    B = 8192
    eng = HipEngine(cfg, params='device_rows', seed=2021, table_rows=(rank, world))
    probe = np.array([0, 1, 77, cfg.M - 1])
    twin = table_rows(cfg, 2021, rank + world * probe, dtype=np.float32)
    for name, tab in (('inner_embeddings', eng.inner), ('outer_embeddings', eng.outer)):
        err, floor = _errors_against_twin(tab[torch.from_numpy(probe).cuda()], 2021, rank + world * probe, TABLES.index(name), 64)
        assert err <= 2 * floor and twin[name].shape == (4, 64), (name, err, floor)
    eng.fbias.normal_(0.0, 0.3, generator=torch.Generator(device='cuda').manual_seed(1))     # the first-order term is 0 at init
    X, y = synth.batches(cfg.M, cfg.F, B, 2, seed=11)
    ids, yt = torch.from_numpy(X.reshape(2 * B, cfg.F)).cuda(), torch.from_numpy(y.reshape(2 * B)).cuda()
    sh = ShardedStep(eng, M_global=cfg.M)
    assert eng.packed_ok()
    lo, hi = -0.01, 0.01
    sums = sh.eval_sums(ids, yt, lo, hi, B, 2)
    pred = torch.cat([sh.predict(ids[:B]), sh.predict(ids[B:])])
    plain = eng.predict(ids[:B])
    torch.cuda.synchronize()
    pred_h = pred.cpu().numpy()
    close(pred_h[:B], plain.cpu().numpy().astype(np.float64), 'cfg5 share: records against tables')
    rows = [0, 1, B // 2, 2 * B - 1]
    uniq, inv = np.unique(X.reshape(2 * B, cfg.F)[rows].reshape(-1), return_inverse=True)
    ut = torch.from_numpy(uniq).cuda().long()
    p64 = to64(eng.export_params_dense())
    p64['inner_embeddings'] = eng.inner[ut].cpu().numpy().astype(np.float64)
    p64['outer_embeddings'] = eng.outer[ut].cpu().numpy().astype(np.float64)
    p64['feature_bias'] = eng.fbias[ut].cpu().numpy().astype(np.float64).reshape(-1, 1)
    ref, _ = orc.forward(p64, inv.reshape(len(rows), cfg.F), cfg)
    close(pred_h[rows], ref, 'cfg5 share: forward-only rows against the oracle')
    clipped = np.minimum(np.maximum(pred_h, np.float32(lo)), np.float32(hi)).astype(np.float64)
    y64 = y.reshape(-1).astype(np.float64)
    np.testing.assert_allclose(sums.cpu().numpy(), [np.sum((y64 - clipped) ** 2), y64.sum(), np.sum(y64 * y64)], rtol=1e-12, atol=0)
