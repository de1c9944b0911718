"""Drop-in for the reference's CFFM.py surface on top of the HIP engine.

Same command line (24 flags, CFFM.py:24-78), same constructor signature (CFFM.py:98-101), same
``train(data)`` / ``evaluate(data) -> (RMSE, R2)`` methods, same public metric lists and helper methods,
same log line formats (CFFM.py:174-179, :218-221, :553, :658-664, :684-695).  What is different underneath:

* the TensorFlow session is replaced by ``cffm_amd.engine.HipEngine`` (hand-written gfx950 kernels behind
  the C ABI of include/cffm_hip.h); there is no CPU fallback;
* the libfm splits are packed once into int32/fp32 tensors resident in HBM; the reference's per-sample
  Python batchers (CFFM.py:560-581, :617-629) reduce to slicing those tensors.  The batch COMPOSITION rule
  is the reference's: a contiguous block from ``np.random.randint(0, N - batch_size)`` after a per-epoch
  ``sklearn.utils.shuffle(..., random_state=2021)`` (quirk Q9), ordered blocks with a ragged last one in
  ``evaluate``;
* quirks that crash the reference are not reproduced: ``--tensorboard 1`` (Q6) is accepted and ignored with
  a warning, ``--pretrain 1`` (Q7) restores THIS model's tensors, no CUDA_VISIBLE_DEVICES pin (Q8).
"""
import argparse
import ast
import logging
import math
import os
from time import time

import numpy as np
from sklearn.utils import shuffle

from . import LoadData as DATA
from .spec import CFFMConfig, logged_param_count


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Run CFFM.")
    add = parser.add_argument
    add('--path', nargs='?', default='data/', help='Input data path.')
    add('--dataset', nargs='?', default='frappe', help='Choose a dataset.')
    add('--epoch', type=int, default=50, help='Number of epochs.')
    add('--pretrain', type=int, default=0,
        help='flag for pretrain. 1: initialize from pretrain; 0: randomly initialize; -1: save the model to pretrain file')
    add('--batch_size', type=int, default=1024, help='Batch size.')
    add('--inner_dims', type=int, default=32, help='Number of inner dimensions.')
    add('--outer_dims', type=int, default=32, help='Number of outer dimensions.')
    add('--lamda', type=float, default=0, help='Regularizer for bilinear part.')
    add('--keep', nargs='?', default='[1.0,1.0]', help='Keep probility (1-dropout) of each layer (parsed, unused).')
    add('--lr', type=float, default=0.05, help='Learning rate.')
    add('--loss_type', nargs='?', default='square_loss',
        help='Specify a loss type (square_loss or log_loss or mse or mae).')
    add('--optimizer', nargs='?', default='AdagradOptimizer', help='Specify an optimizer type (AdagradOptimizer, GradientDescentOptimizer, MomentumOptimizer, AdamOptimizer; '
                            'under a process group every one but AdamOptimizer).')
    add('--verbose', type=int, default=1, help='Show the results per X epochs (0, 1 ... any positive integer)')
    add('--batch_norm', type=int, default=0, help='Parsed, unused (as in the reference graph).')
    add('--tensorboard', type=int, default=0, help='Accepted and ignored (the reference crashes with 1).')
    add('--num_field', type=int, default=3,
        help='Valid dimension of the dataset. (e.g. frappe=10, ml-tag=3, book-crossing=6)')
    add('--linear_att', type=int, default=1, help='Linear attention part (0 disable or 1 enable)')
    add('--att_dim', type=int, default=0, help='Dimension of linear attention (0 is the same as num_field)')
    add('--lamda_att', type=float, default=1.0, help='Softmax temperature of the linear attention part')
    add('--inner_conv', type=int, default=1, help='Inner convolution part (0 disable or 1 enable)')
    add('--gamma_inner', type=int, default=1.0, help='Parsed, unused (as in the reference graph).')
    add('--outer_conv', type=int, default=1, help='Outer convolution part (0 disable or 1 enable)')
    add('--beta_outer', type=int, default=1.0, help='Weight of the outer convolution component')
    add('--activation', nargs='?', default='relu', help='Activation function (relu, prelu, elu, selu, gelu)')
    return parser.parse_args(argv)


def configure_logging(logFilename):
    logging.basicConfig(level=logging.DEBUG, format='%(asctime)s %(filename)s:%(message)s',
                        datefmt='%Y-%m-%d %A %H:%M:%S', filename=logFilename, filemode='a')
    console = logging.StreamHandler()
    console.setLevel(logging.INFO)
    console.setFormatter(logging.Formatter('%(asctime)s %(filename)s:%(message)s'))
    logging.getLogger().addHandler(console)


# CFFM.recommend / CFFM.evaluate_ranking(sweep='auto'): the smallest candidate count from which the shared sweep
# (HipEngine.score_candidates_shared) is used where the shape is served.  Set from profiles/sweep_vs_expand.md (how: there).
SWEEP_MIN_N = 4082


def ranking_metrics(ranks, k):
    """(HR@k, NDCG@k) of 0-based ranks of one relevant item each: HR = mean(rank < k), NDCG = mean(1 / log2(rank + 2) if
    rank < k else 0), in float64 on the host.  A negative rank (a target that was no candidate) counts as a miss."""
    r = np.asarray(ranks, dtype=np.int64).reshape(-1)
    if r.size == 0:
        raise ValueError('ranking_metrics() needs at least one rank')
    hit = (r >= 0) & (r < int(k))
    gain = np.where(hit, 1.0 / np.log2(np.where(hit, r, 0).astype(np.float64) + 2.0), 0.0)
    return float(hit.mean()), float(gain.mean())


class CFFM(object):
    def __init__(self, features_M, pretrain_flag, save_file, inner_dims, outer_dims, loss_type, epoch, batch_size,
                 learning_rate, lamda_bilinear, keep, optimizer_type, batch_norm, verbose, tensorboard, num_field,
                 linear_att, att_dim, lamda_att, inner_conv, gamma_inner, outer_conv, beta_outer,
                 activation_function, random_seed=2021, batch_rng=None):
        self.batch_size = batch_size
        self.learning_rate = learning_rate
        self.inner_dims = inner_dims
        self.outer_dims = outer_dims
        self.pretrain_flag = pretrain_flag
        self.save_file = save_file
        self.loss_type = loss_type
        self.features_M = features_M
        self.lamda_bilinear = lamda_bilinear
        self.keep = keep
        self.epoch = epoch
        self.random_seed = random_seed
        self.optimizer_type = optimizer_type
        self.batch_norm = batch_norm
        self.verbose = verbose
        self.tensorboard = tensorboard
        self.num_field = num_field
        self.linear_att = linear_att
        self.att_dim = num_field if att_dim == 0 else att_dim
        if self.linear_att == 1 and self.att_dim != num_field:
            # the reference's matmul [B,F] x [att_dim,att_dim] (CFFM.py:432) only type-checks for att_dim == F
            raise ValueError('att_dim must equal num_field (or be 0)')
        self.lamda_att = lamda_att
        self.inner_conv = inner_conv
        self.gamma_inner = gamma_inner
        self.outer_conv = outer_conv
        self.beta_outer = beta_outer
        self.num_interactions = int(self.num_field * (self.num_field - 1) / 2)
        self.activation_function = activation_function
        if optimizer_type not in ('AdagradOptimizer', 'AdamOptimizer', 'GradientDescentOptimizer', 'MomentumOptimizer'):
            # the reference leaves self.optimizer unset for any other string and dies at the first sess.run (CFFM.py:517-529)
            raise ValueError('unknown optimizer %r' % (optimizer_type,))
        if loss_type == 'square_loss' and lamda_bilinear > 0:
            # create_loss regularises self.weights['inner_embeddings'] and ['outer_embeddings'] (CFFM.py:489-491), which
            # only exist for an enabled branch (CFFM.py:255, :262): the reference dies with this KeyError at graph build
            for flag, name in ((inner_conv, 'inner_embeddings'), (outer_conv, 'outer_embeddings')):
                if flag != 1:
                    raise KeyError(name)
        if tensorboard > 0:
            logging.warning('--tensorboard is accepted and ignored (it crashes the reference, CFFM.py:194-196)')
        self.config = CFFMConfig(M=features_M, F=num_field, K=inner_dims, D=outer_dims, activation=activation_function,
                                 lamda_att=lamda_att, beta_outer=beta_outer, linear_att=linear_att,
                                 inner_conv=inner_conv, outer_conv=outer_conv, loss_type=loss_type,
                                 lamda_bilinear=lamda_bilinear, lr=learning_rate, optimizer=optimizer_type)
        self.create_save_folder(save_file)
        self.train_rmse, self.valid_rmse, self.test_rmse = [], [], []
        self.train_r2, self.valid_r2, self.test_r2 = [], [], []
        self.engine = None
        self._packed = {}
        self.examples_per_sec = []
        # Source of the random block starts (CFFM.py:561 draws them from the unseeded process-global np.random; SURVEY A.6
        # Q9: "behind an injectable RNG").  Anything with numpy's randint(low, high, size=None) works; the default IS the
        # global np.random, so an unpinned run behaves like the reference.  batch_starts keeps the draws, one array per epoch.
        self.batch_rng = np.random if batch_rng is None else batch_rng
        self.batch_starts = []
        # multi-GPU (set by build_graph under torch.distributed): one process per GPU, data parallel over the batch
        # _sh: CFFM_TABLES=sharded at world size > 1 - cffm_amd.dist.ShardedStep over this rank's rows of the tables
        self.world, self.rank, self._dp, self._sh = 1, 0, None, None
        self._train_split = None                       # the train split last passed to train()

    # ---- engine / data residency -----------------------------------------------------------------------
    def build_graph(self):
        """Creates the device state (the reference builds the TF graph here, CFFM.py:531-541)."""
        import torch
        # one process per GPU: the device is the launcher's LOCAL_RANK (torch.distributed.run) or the process's current
        # device; it is made current so that the library's launches and torch's stream agree on it
        dev = int(os.environ.get('LOCAL_RANK', torch.cuda.current_device() if torch.cuda.is_available() else 0))
        if torch.cuda.is_available():
            torch.cuda.set_device(dev)
        sharded = os.environ.get('CFFM_TABLES', 'replicated') == 'sharded'
        if sharded:
            self._build_sharded(dev)                   # the engine over this rank's rows and, from two ranks up, its step
        else:
            self.engine = self._make_engine(dev)
        if self.pretrain_flag > 0:
            self.load(self.save_file)
        if not sharded:
            self._setup_dist()
        return self.engine

    def _refuse_uneven_batch(self):
        if self.batch_size % self.world:
            raise ValueError('--batch_size %d is not a multiple of the %d ranks' % (self.batch_size, self.world))

    engine_factory = None          # tests plug a CPU stand-in (the oracle) in here; the product path is HipEngine

    def _make_engine(self, dev):
        if self.engine_factory is not None:
            return type(self).engine_factory(self.config, self.random_seed)
        from .engine import HipEngine
        return HipEngine(self.config, seed=self.random_seed, device='cuda:%d' % dev)

    # CFFM_TABLES=sharded: (local config, seed, rank, world, global rows) -> the engine over THIS rank's rows of the tables
    # (global rows rank, rank + world, ...), drawn by global row; the CPU tests plug an oracle stand-in built from
    # spec.table_rows in here, the product path is HipEngine(params='device_rows')
    sharded_engine_factory = None

    def _join_group(self, device):
        """(world, rank) of the process group: the one the caller initialised, or the launcher's (RANK / WORLD_SIZE in the
        environment, torch.distributed.run); (1, 0) without either."""
        import torch
        import torch.distributed as dist
        if not dist.is_available():
            return 1, 0
        if not dist.is_initialized():
            if int(os.environ.get('WORLD_SIZE', '1')) <= 1:
                return 1, 0
            on_gpu = torch.cuda.is_available()
            dist.init_process_group('nccl' if on_gpu else 'gloo', device_id=device if on_gpu else None)
        return dist.get_world_size(), dist.get_rank()

    def _build_sharded(self, dev):
        """CFFM_TABLES=sharded: row r of the three tables and of their Adagrad slots lives on rank r % world at local row
        r // world (vocabularies beyond one GPU's HBM), the dense parameters are replicated (rank 0's are broadcast), and the
        tables are drawn BY GLOBAL ROW from --random_seed, so every world size trains the same model: at world size 1 this is a
        plain engine whose tables are drawn the same way, the single-process twin of every multi-rank run.  train() steps
        through cffm_amd.dist.ShardedStep with the routing plan one step ahead; evaluate() / predict_split() sweep a
        contiguous share of the rows per rank through its forward-only path."""
        import copy
        import torch
        from .dist import ShardedStep, local_rows_count
        self.world, self.rank = self._join_group(torch.device('cuda', dev) if torch.cuda.is_available() else None)
        if self.world > 1:
            # what the row-sharded step does not implement is refused here, by name, before the first collective
            from .dist import MULTI_GPU_OPTIMIZERS
            if self.optimizer_type not in MULTI_GPU_OPTIMIZERS:
                raise ValueError('CFFM_TABLES=sharded: the multi-GPU update implements %s; --optimizer %s runs on one GPU'
                                 % (', '.join(MULTI_GPU_OPTIMIZERS), self.optimizer_type))
            if self.loss_type == 'hybrid':
                raise ValueError('CFFM_TABLES=sharded: --loss_type hybrid runs on one GPU only')
            if self.loss_type == 'square_loss' and self.lamda_bilinear > 0:
                raise ValueError('CFFM_TABLES=sharded: --lamda > 0 (a regulariser over whole tables) runs on one GPU only')
            self._refuse_uneven_batch()
            if self.features_M < self.world:
                raise ValueError('CFFM_TABLES=sharded: %d features over %d ranks leaves a rank without rows' % (self.features_M, self.world))
        cfg = copy.copy(self.config)
        cfg.M = local_rows_count(self.features_M, self.rank, self.world)
        if self.sharded_engine_factory is not None:
            self.engine = type(self).sharded_engine_factory(cfg, self.random_seed, self.rank, self.world, self.features_M)
        else:
            from .engine import HipEngine
            self.engine = HipEngine(cfg, params='device_rows', seed=self.random_seed, table_seed=self.random_seed,
                                    table_rows=(self.rank, self.world), device='cuda:%d' % dev)
        if self.world > 1:
            self._sh = ShardedStep(self.engine, M_global=self.features_M)

    def _setup_dist(self):
        """One process per GPU under torch.distributed.run (RANK / WORLD_SIZE / LOCAL_RANK in the environment), or a process
        group the caller initialised: the train step becomes cffm_amd.dist.DataParallelStep - every rank its slice of the
        SAME global batch, two collectives per step, replicas bit-identical (rank 0's parameters are broadcast at
        construction) - and evaluate() splits the rows over the ranks and all-reduces the three metric sums.  The reference
        is single-device (CFFM.py:19 pins one GPU), so this replaces nothing in it; at world size 1 nothing changes."""
        self.world, self.rank = self._join_group(self.engine.device)
        if self.world == 1:
            return
        tables = os.environ.get('CFFM_TABLES', 'replicated')
        if tables != 'replicated':                     # 'sharded' went through _build_sharded
            raise ValueError("CFFM_TABLES=%r: the accepted values are 'replicated' (default) and 'sharded'" % (tables,))
        self._refuse_uneven_batch()
        from .dist import DataParallelStep
        self._dp = DataParallelStep(self.engine)

    def _info(self, msg):
        if self.rank == 0:
            logging.info(msg)

    def _all_reduce_sum(self, t):
        if self.world > 1:
            import torch.distributed as dist
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t

    def _device_split(self, data):
        """{'X': lists, 'Y': list} -> (ids int32 [N,F], y fp32 [N], (min label, max label)) in HBM, packed once per split
        object (re-packed when the caller swaps the lists)."""
        import torch
        key = id(data)
        hit = self._packed.get(key)
        if hit is not None and hit[2] is self._token(data):
            return hit[0], hit[1], hit[3]
        X, Y = DATA.LoadData.packed(data)
        if X.shape[1] != self.num_field:
            raise ValueError('rows have %d ids, --num_field is %d' % (X.shape[1], self.num_field))
        dev = self.engine.device
        ids, y = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
        span = (float(Y.min()), float(Y.max())) if Y.size else (0.0, 0.0)      # clip range of evaluate(), CFFM.py:607-609
        self._packed[key] = (ids, y, self._token(data), span)
        return ids, y, span

    @staticmethod
    def _token(data):
        """What identifies the current content of a split: the loader's packed array while its lists have not been built
        or re-bound (cffm_amd.LoadData._Split), else the 'X' list object itself."""
        arrays = getattr(data, '_arrays', None)
        return arrays[0] if arrays is not None else data['X']

    # ---- training loop (CFFM.py:157-228) -------------------------------------------------------------
    def _train_step(self):
        """The step of train(), decided once per call: step(ids, y, starts, i) trains on batch i of an epoch's block starts, under
        a process group on this rank's slice of it."""
        per = self.batch_size // self.world

        def part(t, starts, i):
            lo = int(starts[i]) + self.rank * per
            return t[lo:lo + per]

        if self._sh is not None:
            # this rank's slice of the batch, and of the NEXT one: its routing plan (and the read of the per-owner counts) is
            # issued before this step's kernels
            return lambda ids, y, starts, i: self._sh.train_step(part(ids, starts, i), part(y, starts, i),
                                                                 next_ids=part(ids, starts, i + 1) if i + 1 < len(starts) else None)
        run = self._dp.train_step if self._dp is not None else self.engine.train_step
        return lambda ids, y, starts, i: run(part(ids, starts, i), part(y, starts, i))

    def train(self, data):
        import torch
        if self.engine is None:
            self.build_graph()
        step = self._train_step()
        self._train_split = data.Train_data            # recommend() / evaluate_ranking() draw their default candidates from it
        self.calculate_parameters()
        if self.verbose > 0:
            t2 = time()
            init_train_rmse, init_train_r2 = self.evaluate(data.Train_data)
            init_valid_rmse, init_validation_r2 = self.evaluate(data.Validation_data)
            init_test_rmse, init_test_r2 = self.evaluate(data.Test_data)
            self._info(("Init_RMSE: train=%.4f,validation=%.4f,test=%.4f | Init_R2: train=%.4f,validation=%.4f,"
                        "test=%.4f [%.1f s] " % (init_train_rmse, init_valid_rmse, init_test_rmse, init_train_r2,
                                                init_validation_r2, init_test_r2, time() - t2)))
        ids, y, span = self._device_split(data.Train_data)
        n = ids.shape[0]
        # shuffle_in_unison_scary (CFFM.py:183, :556-558): sklearn's shuffle with the SAME random_state every epoch, i.e. one
        # fixed permutation of n positions applied to the CURRENT order each time.  It is built once and kept on the
        # device; `order` tracks the composition so that the caller's lists can be left as the reference leaves them.
        perm = shuffle(np.arange(n), random_state=self.random_seed)
        pt = torch.from_numpy(perm).to(ids.device)
        order = np.arange(n)
        try:
            for epoch in range(self.epoch):
                t1 = time()
                ids, y = ids[pt].contiguous(), y[pt].contiguous()
                order = order[perm]
                total_batch = int(n / self.batch_size)
                # CFFM.py:561: one np.random.randint per step, from self.batch_rng (the unseeded global np.random unless the
                # caller injected one).  Drawn for the whole epoch at once (the same stream as one call per step); under
                # torch.distributed rank 0's draws are everyone's, so that the ranks cut their slices out of the SAME
                # global batch.
                starts = self.batch_rng.randint(0, n - self.batch_size, size=total_batch)
                if self.world > 1:
                    import torch.distributed as dist
                    st = torch.from_numpy(starts.astype(np.int64)).to(ids.device)
                    dist.broadcast(st, src=0)
                    starts = st.cpu().numpy()
                self.batch_starts.append(np.asarray(starts, dtype=np.int64))
                for i in range(len(starts)):
                    step(ids, y, starts, i)
                if torch.cuda.is_available():
                    torch.cuda.synchronize()
                t2 = time()
                self.examples_per_sec.append(total_batch * self.batch_size / max(t2 - t1, 1e-9))
                self._packed[id(data.Train_data)] = (ids, y, self._token(data.Train_data), span)   # evaluate() sees the shuffled order
                train_rmse, train_r2 = self.evaluate(data.Train_data)
                valid_rmse, valid_r2 = self.evaluate(data.Validation_data)
                test_rmse, test_r2 = self.evaluate(data.Test_data)
                self.train_rmse.append(train_rmse)
                self.valid_rmse.append(valid_rmse)
                self.test_rmse.append(test_rmse)
                self.train_r2.append(train_r2)
                self.valid_r2.append(valid_r2)
                self.test_r2.append(test_r2)
                if self.verbose > 0 and epoch % self.verbose == 0:
                    self._info(("Epoch %d [%.1f s] RMSE: train=%.4f,validation=%.4f,Test=%.4f | R2: train=%.4f,"
                                "validation=%.4f,Test=%.4f [%.1f s]" % (epoch + 1, t2 - t1, train_rmse, valid_rmse,
                                                                        test_rmse, train_r2, valid_r2, test_r2,
                                                                        time() - t2)))
                    self._info("Epoch %d throughput: %.0f training examples/s%s" % (
                        epoch + 1, self.examples_per_sec[-1], ' (%d ranks)' % self.world if self.world > 1 else ''))
                if self.eva_termination(self.valid_rmse):
                    break
                if self.pretrain_flag < 0 and (self.rank == 0 or self._sh is not None):
                    # replicated tables: the replicas are identical, rank 0 writes; row-sharded: every rank writes its shard
                    self._info("Save model to file as pretrain.")
                    self.save(self.save_file)
            if self._sh is not None and self.verbose > 0:
                self._info("Row-sharded tables over %d ranks: %d train steps ran on a routing plan issued one step ahead (plans_reused)"
                           % (self.world, self._sh.plans_reused))
        finally:
            # the reference re-binds data.Train_data['X'] / ['Y'] to the shuffled lists every epoch (CFFM.py:183); the device
            # copy is what the loop trains on, so the caller's lists are brought to the same (composed) order once, here
            if not np.array_equal(order, np.arange(n)):
                X0, Y0 = data.Train_data['X'], data.Train_data['Y']
                data.Train_data['X'] = [X0[i] for i in order]
                data.Train_data['Y'] = [Y0[i] for i in order]
                self._packed[id(data.Train_data)] = (ids, y, self._token(data.Train_data), span)

    # ---- evaluation (CFFM.py:583-615) ------------------------------------------------------------------
    def evaluate(self, data):
        """RMSE and R2 of the clipped predictions (CFFM.py:583-615).  The whole sweep stays on the device: ordered blocks
        with a ragged last one (CFFM.py:590-596; the forward is per example, so the block size does not change a
        prediction - blocks of >= 8192 rows run the conv kernels at 12 M examples/s against 3.7 M at 256), clip to the
        split's label range, and the three float64 sums of the metrics; three doubles come back to the host."""
        if self.engine is None:
            self.build_graph()
        ids, y, (lo, hi) = self._device_split(data)
        num_example = int(ids.shape[0])
        if num_example == 0:
            raise ValueError('evaluate() needs at least one example')
        # the forward is per example: every rank sweeps its contiguous share of the rows, the three sums are added up
        r0, r1, _, block, n_blocks = self._share(num_example)
        if self._sh is not None:
            # row-sharded tables: a forward needs the owners of its rows, so every rank runs the SAME number of rounds of
            # collectives - what the largest share (rank 0's) needs; a rank whose rows have run out joins with empty blocks
            sums = self._sh.eval_sums(ids[r0:r1], y[r0:r1], lo, hi, block, n_blocks)
        else:
            sums = self.engine.eval_sums(ids[r0:r1], y[r0:r1], lo, hi, block=block)
        ss_res, sy, syy = (float(v) for v in self._all_reduce_sum(sums).cpu().numpy())
        if not math.isfinite(ss_res):
            # np.maximum/np.minimum propagate NaN and sklearn's mean_squared_error raises on it (CFFM.py:607-612): a
            # diverged model must not come back with a finite metric
            raise ValueError('evaluate(): predictions contain NaN or infinity')
        RMSE = math.sqrt(ss_res / num_example)                  # sqrt(mean_squared_error), CFFM.py:610-612
        ss_tot = syy - sy * sy / num_example                    # sum (y - mean(y))^2
        R2 = 1.0 - ss_res / ss_tot if ss_tot > 0 else (1.0 if ss_res == 0 else 0.0)    # sklearn r2_score, CFFM.py:614
        return RMSE, R2

    def _share(self, num_example):
        """This rank's contiguous share [r0, r1) of a split's rows, the size of the LARGEST share (shares only get shorter with the
        rank, so that is rank 0's), the block size of the sweep and the number of blocks the largest share takes."""
        r0, r1, share = self._row_share(num_example)
        block = max(int(self.batch_size), 8192)
        return r0, r1, share, block, -(-share // block)

    def _row_share(self, n):
        """This rank's contiguous share [r0, r1) of n rows and the size of the largest share; all of them without a process group."""
        share = -(-n // self.world)
        return min(self.rank * share, n), min((self.rank + 1) * share, n), share

    def predict_split(self, data):
        """Raw (unclipped) predictions of a split as a host float64 array, in the split's current order."""
        import torch
        ids, _, _ = self._device_split(data)
        n = int(ids.shape[0])
        r0, r1, share, block, n_blocks = self._share(n)
        if self._sh is not None:
            # every rank predicts its share (in matched rounds, as evaluate() does) and gets the whole split back
            import torch.distributed as dist
            mine = None
            for b in range(n_blocks):
                s0, s1 = min(r0 + b * block, r1), min(r0 + (b + 1) * block, r1)
                out = self._sh.predict(ids[s0:s1])
                if mine is None:
                    mine = out.new_zeros(share)
                mine[s0 - r0:s1 - r0] = out
            if mine is None:
                return np.zeros((0,))
            full = mine.new_empty(share * self.world)
            dist.all_gather_into_tensor(full, mine)
            return full[:n].cpu().numpy().astype(np.float64)
        outs = [self.engine.predict(ids[s:s + block]) for s in range(0, n, block)]
        return torch.cat(outs).cpu().numpy().astype(np.float64) if outs else np.zeros((0,))

    # ---- candidate ranking: what a trained recommender is asked for ------------------------------------------------------
    # The reference stops at RMSE / R2; these sweep (context, candidate) pairs on the device (cffm_amd/csrc/rank.hip): the ids of
    # the pairs are expanded there, scored by the ordinary forward, and top-k / rank-of-target run on the score buffer in ONE
    # total order (score descending, -0 == +0, NaN last, ties by candidate position), so equal scores - frequent with +-1 labels
    # and saturated predictions - always come back the same way.
    def _ranking_engine(self):
        if self.engine is None:
            self.build_graph()
        if self._sh is not None:
            # the row-sharded forward is a matched collective over all ranks; a ranking sweep on it is not implemented
            raise ValueError('CFFM_TABLES=sharded: recommend / evaluate_ranking run on replicated tables')
        return self.engine

    @staticmethod
    def _scorer(eng, sweep, fields, N, per_context=False):
        """score(ctx, cand), the engine call that scores one group of contexts.  fields: an int for recommend / evaluate_ranking
        (cand [N]; 'expand' is score_candidates, called exactly as before the shared sweep existed, and there is no 'tuples'), or
        the list of columns of the *_tuples methods (cand [N, nf], or [C, N, nf] per context; 'expand' is score_candidate_tuples,
        bit for bit predict on the expanded rows).  'shared': the shared sweep, one field only (ValueError for tuples or a shape
        that is not served).  'auto': the shared sweep for one field at a served shape with N >= SWEEP_MIN_N, else expand.
        'tuples': the tuple sweep (score_candidate_tuples_shared) for any nf >= 1, ValueError where (shape, nf) is not served;
        'auto' never picks it."""
        one = isinstance(fields, int)
        allowed = ('expand', 'shared', 'auto') if one else ('expand', 'shared', 'auto', 'tuples')
        if sweep not in allowed:
            raise ValueError('sweep must be %s or %r, not %r' % (', '.join(repr(a) for a in allowed[:-1]), allowed[-1], sweep))
        cols = [fields] if one else fields
        nf = len(cols)
        if sweep == 'tuples':
            if not eng.sweep_tuples_ok(nf):
                raise ValueError("sweep='tuples': the tuple sweep does not serve this shape for tuples of %d (both branches, D = 32, "
                                 "F <= 10, nf <= 4, the candidate kernel within a CU's LDS)" % nf)
            return lambda ctx, cand: eng.score_candidate_tuples_shared(ctx, fields, cand)
        if sweep == 'shared':
            if nf > 1:
                raise ValueError("sweep='shared': the shared sweep scores one field, not tuples of %d" % nf)
            if not eng.sweep_ok():
                raise ValueError("sweep='shared': the shared sweep does not serve this shape (both branches, D = 32, F <= 10)")
        elif sweep == 'expand' or nf > 1 or SWEEP_MIN_N is None or N < SWEEP_MIN_N or not eng.sweep_ok():
            expand = eng.score_candidates if one else eng.score_candidate_tuples
            return lambda ctx, cand: expand(ctx, fields, cand)
        if per_context:
            return lambda ctx, cand: eng.score_candidate_lists_shared(ctx, cols[0], cand.reshape(cand.shape[0], cand.shape[1]))
        return lambda ctx, cand: eng.score_candidates_shared(ctx, cols[0], cand.reshape(-1))

    def _distinct(self, splits, cols, counts=False):
        """The distinct tuples at the columns `cols` (ids, for one column) over the given splits, sorted, int32 on the device; with
        counts, the number of rows (any label) that carry each of them instead."""
        import torch
        rows = torch.cat([self._device_split(d)[0][:, cols] for d in splits])
        if counts:
            return torch.unique(rows, dim=0, return_counts=True)[1]
        return torch.unique(rows, dim=0).to(torch.int32)

    def _eval_splits(self, data):
        """The splits an evaluation's default candidates come from: the train split last passed to train(), and `data`."""
        return [data] if self._train_split is None or self._train_split is data else [self._train_split, data]

    def _candidates(self, candidates, field, splits):
        import torch
        if not 0 <= int(field) < self.num_field:
            raise ValueError('field %r is outside [0, %d)' % (field, self.num_field))
        if candidates is None:
            return self._distinct(splits, int(field))
        cand = np.asarray(candidates)
        if cand.ndim != 1 or cand.size == 0:
            raise ValueError('candidates must be a non-empty 1-D array of feature ids')
        return torch.from_numpy(np.ascontiguousarray(cand.astype(np.int32))).to(self.engine.device)

    # ---- ranking without the items an owner has already seen -----------------------------------------------
    def _seen_args(self, who, exclude, by, cols, refuse=()):
        """exclude= / by= of the four ranking methods, checked before anything runs: None without them, else (the list of splits,
        the owner column).  cols: the swept columns; refuse: (keyword, value, why) triples of keywords exclude does not go with."""
        if exclude is None and by is None:
            return None
        if exclude is None:
            raise ValueError('%s: by= names the owner column of exclude=, which is missing: pass exclude too' % who)
        if by is None:
            raise ValueError('%s: exclude= needs by=, the column whose id names the owner of a seen item: pass by too' % who)
        for name, value, why in refuse:
            if value:
                raise ValueError('%s: exclude= does not go with %s: %s' % (who, name, why))
        if isinstance(by, bool) or not isinstance(by, (int, np.integer)) or not 0 <= int(by) < self.num_field:
            raise ValueError('%s: by=%r is not a column of [0, %d)' % (who, by, self.num_field))
        if int(by) in cols:
            raise ValueError('%s: by=%d is a swept column; the owner column must be one the candidates leave alone' % (who, int(by)))
        splits = [exclude] if isinstance(exclude, dict) else list(exclude)
        if not splits or not all(isinstance(d, dict) and 'X' in d and 'Y' in d for d in splits):
            raise ValueError("%s: exclude must be a split {'X': ..., 'Y': ...} or a list of splits" % who)
        return splits, int(by)

    def _seen_relation(self, seen, cols, cand):
        """The seen relation of a call as a CSR over candidate POSITIONS, built on the device once (cffm_amd.spec.seen_index is the
        specification): (keys [R] the sorted distinct owners, off int32 [R + 1], pos int32 [nnz]).  Owner u has seen every entry of
        cand - ids [N] for one swept column, tuples [N, nf] otherwise - that occurs at the swept columns of a row of the splits with
        label > 0 and id u at the owner column, at EVERY position that holds it; a seen tuple cand lacks is dropped.  The one
        device-to-host read is the number of pairs, for the int32 bound and the kernel's argument."""
        import torch
        splits, by = seen
        rows = torch.cat([ids[y.reshape(-1) > 0] for ids, y, _ in (self._device_split(d) for d in splits)])
        N = int(cand.shape[0])
        what = rows[:, cols[0]] if cand.dim() == 1 else rows[:, cols]
        first = self._positions(cand, what.to(cand.dtype))                      # the first position that holds the seen entry, N if none
        here = first < N
        owner, first = rows[:, by][here].long(), first[here]
        # the list may repeat an entry: position n stands for the first position that holds cand[n], and a seen entry takes every
        # position of its group
        group, order = torch.sort(self._positions(cand, cand), stable=True)
        lo = torch.searchsorted(group, first)
        n_of = torch.searchsorted(group, first, right=True) - lo
        start = torch.repeat_interleave(lo, n_of)
        within = torch.arange(int(start.numel()), device=start.device) - torch.repeat_interleave(torch.cumsum(n_of, 0) - n_of, n_of)
        keys, krow = torch.unique(torch.repeat_interleave(owner, n_of), return_inverse=True)
        pairs = torch.unique(krow * N + order[start + within])                 # (CSR row, position), sorted, each once
        nnz = int(pairs.numel())
        if nnz >= 1 << 31:
            raise ValueError('exclude: the seen relation holds %d (owner, position) pairs; the CSR indexes fewer than 2^31' % nnz)
        R = int(keys.numel())
        off = torch.searchsorted(torch.div(pairs, N, rounding_mode='floor'), torch.arange(R + 1, device=pairs.device)).to(torch.int32)
        return keys, off, (pairs % N).to(torch.int32)

    def _seen_masks(self, eng, seen, cols, cand, ctx, N, skip=None):
        """mask(c0, c1) for the group loops of _topk_sweep and _rank_targets: the seen set of every context's owner as the uint8
        [c1 - c0, N] skip mask of topk / rank_of, OR-ed with the rows of skip (uint8 [C, N] on the device, or None).  The CSR row of
        EVERY context is looked up here, once, next to the relation build (keys is sorted and distinct: a searchsorted and a compare,
        -1 for an owner that is not there); a group is then a slice of that vector and one HipEngine.seen_mask launch, and nothing in
        the returned mask(c0, c1) synchronises with the host."""
        import torch
        keys, off, pos = self._seen_relation(seen, cols, cand)
        owner = ctx[:, seen[1]].to(keys.dtype).contiguous()
        R = int(keys.numel())
        if R == 0:
            row = torch.full((int(owner.shape[0]),), -1, dtype=torch.int32, device=owner.device)
        else:
            at = torch.searchsorted(keys, owner).clamp(max=R - 1)
            row = torch.where(keys[at] == owner, at, torch.full_like(at, -1)).to(torch.int32)
        return lambda c0, c1: eng.seen_mask(off, pos, row[c0:c1], N, skip=None if skip is None else skip[c0:c1])

    def recommend(self, contexts, field, candidates=None, k=10, skip=None, score_rows=1 << 22, sweep='expand', exclude=None, by=None):
        """For every context row (contexts [C,F] feature ids), the k candidates that score highest when their id is put at column
        `field`.  candidates: 1-D feature ids (default: the sorted distinct ids in column `field` of the train split last passed
        to train()); skip: optional boolean [C,N] over candidate positions, True = leave out (e.g. items already seen).
        Contexts are processed in groups of max(1, score_rows // N), so the score buffer stays bounded.  Returns host arrays
        (ids int32 [C,k] candidate feature ids, -1 padded; scores float32 [C,k] their raw predictions, NaN padded).  Local to
        the calling rank: no collective.  sweep: 'expand' (default) scores the expanded id rows with the ordinary forward;
        'shared' does the fixed-field work once per context (equal to rounding, not bit for bit; ValueError for a shape it does
        not serve); 'auto' picks 'shared' where it is served and N >= SWEEP_MIN_N.
        exclude / by (together, or a ValueError names the missing one; default None: every call as without them): exclude is a split
        (the dict train() / evaluate() take) or a list of splits, by the column whose id names the owner of a seen item (the user
        column; not `field`).  Every candidate that occurs at column `field` of a row of exclude with label > 0 and the context's
        own id at column by is left out for that context, at every position of an explicit list that holds it, OR-ed with skip.
        The relation goes to the device once as a CSR and the mask is made there per group of contexts (HipEngine.seen_mask)
        instead of a dense host [C, N] array."""
        import torch
        eng = self._ranking_engine()
        seen = self._seen_args('recommend()', exclude, by, [int(field)])
        if candidates is None and self._train_split is None:
            raise ValueError('recommend(): no train split yet (train() was not called) - pass candidates')
        if not 1 <= int(k) <= 1024:
            raise ValueError('recommend(): k must be in [1, 1024]')
        cand = self._candidates(candidates, field, [self._train_split])
        pos, val = self._topk_sweep(eng, self._contexts(eng, contexts), int(field), cand, False, None, int(k), skip, score_rows, sweep, seen)
        cand64 = cand.long()
        ids = torch.where(pos >= 0, cand64[pos.clamp(min=0).long()], cand64.new_full((), -1)).to(torch.int32)
        return ids.cpu().numpy(), val.cpu().numpy()

    def _contexts(self, eng, contexts):
        """The caller's context rows [C, F], checked, as int32 on the device."""
        import torch
        ctx = np.asarray(contexts)
        if ctx.ndim != 2 or ctx.shape[1] != self.num_field:
            raise ValueError('contexts must be [C, %d] feature ids' % self.num_field)
        return torch.from_numpy(np.ascontiguousarray(ctx.astype(np.int32))).to(eng.device)

    def _topk_sweep(self, eng, ctx, fields, cand, per_context, counts, k, skip, score_rows, sweep, seen=None):
        """The top-k sweep of recommend and recommend_tuples over ctx and cand on the device (fields and cand as _scorer takes
        them), the contexts in groups of max(1, score_rows // N): (pos int32 [C, k] candidate positions, -1 padded; val float32
        [C, k], NaN padded) on the device.  skip and counts are the caller's host arrays; counts is merged into the skip mask.
        seen: what _seen_args returned; with it the skip mask of a group is made on the device from the seen relation, that host
        mask OR-ed in (_seen_masks)."""
        import torch
        C, N = int(ctx.shape[0]), int(cand.shape[1 if per_context else 0])
        if per_context and cand.shape[0] != C:
            raise ValueError('per_context candidates must hold one list per context: [%d, N, ...], not %r' % (C, tuple(cand.shape)))
        mask = None
        if skip is not None:
            mask = np.asarray(skip) != 0
            if mask.shape != (C, N):
                raise ValueError('skip must be [%d, %d]: contexts x candidates' % (C, N))
        if counts is not None:
            if not per_context:
                raise ValueError('counts belongs to per_context candidate lists')
            cnt = np.asarray(counts)
            if cnt.shape != (C,) or cnt.dtype.kind not in 'iu' or (cnt < 0).any() or (cnt > N).any():
                raise ValueError('counts must be [%d] integers in [0, %d]' % (C, N))
            pad = np.arange(N)[None, :] >= cnt[:, None]
            mask = pad if mask is None else (mask | pad)
        if mask is not None:
            mask = torch.from_numpy(np.ascontiguousarray(mask)).to(eng.device).to(torch.uint8)
        pos_out = torch.empty((C, k), dtype=torch.int32, device=eng.device)
        val_out = torch.empty((C, k), dtype=torch.float32, device=eng.device)
        group = max(1, int(score_rows) // N)
        score = self._scorer(eng, sweep, fields, N, per_context)
        if seen is not None:
            seen_of = self._seen_masks(eng, seen, [fields] if isinstance(fields, int) else fields, cand, ctx, N, mask)
        for c0 in range(0, C, group):
            c1 = min(C, c0 + group)
            scores = score(ctx[c0:c1], cand[c0:c1] if per_context else cand)
            if seen is not None:
                idx, val, _ = eng.topk(scores, k, skip=seen_of(c0, c1))
            else:
                idx, val, _ = eng.topk(scores, k, skip=None if mask is None else mask[c0:c1])
            pos_out[c0:c1] = idx
            val_out[c0:c1] = val
        return pos_out, val_out

    def evaluate_ranking(self, data, field, k=10, candidates=None, score_rows=1 << 22, sweep='expand', exclude=None, by=None):
        """(HR@k, NDCG@k) of a split: for every row with label > 0 the context is the row and the target is the row's own id at
        column `field`, ranked among the candidates (default: the sorted distinct ids in column `field` over the train split and
        `data` together, so every target is a candidate).  Explicit candidates that lack a target raise ValueError.  The sweep
        stays on the device: scores, rank of the target, and the two sums and the count in float64; under a process group with
        replicated tables every rank takes a contiguous share of the positive rows and the sums are all-reduced.  sweep: as in
        recommend().
        exclude / by (together; default None: every call as without them): as in recommend() - every positive row is ranked among
        the candidates its own owner (the row's id at column by) has NOT got in exclude (label > 0), the filtered protocol of
        full-ranking evaluations with exclude = the train split.  The target itself always stays: a pair that is in both splits is
        still ranked (cffm_rank_of ignores the flag at the target).  Under a process group every rank builds the whole relation."""
        eng = self._ranking_engine()
        seen = self._seen_args('evaluate_ranking()', exclude, by, [int(field)])
        ids, y, _ = self._device_split(data)
        cand = self._candidates(candidates, field, self._eval_splits(data))
        field, k = int(field), int(k)
        if k < 1:
            raise ValueError('evaluate_ranking(): k must be >= 1')
        ctx = ids[y.reshape(-1) > 0]
        P, N = int(ctx.shape[0]), int(cand.numel())
        if P == 0:
            raise ValueError('evaluate_ranking() needs at least one row with a positive label')
        tgt = ctx[:, field]
        tpos = self._positions(cand, tgt)
        missing = tpos == N
        if bool(missing.any()):
            raise ValueError('evaluate_ranking(): target id %d at field %d is not among the candidates'
                             % (int(tgt[missing][0]), field))
        r0, r1, _ = self._row_share(P)
        seen_of = None if seen is None else self._seen_masks(eng, seen, [field], cand, ctx, N)
        return self._rank_targets('evaluate_ranking()', eng, self._scorer(eng, sweep, field, N), ctx, lambda c0, c1: cand, tpos, r0, r1,
                                  N, k, score_rows, seen_of)

    def _rank_targets(self, who, eng, score, ctx, cand_of, tpos, r0, r1, N, k, score_rows, seen_of=None):
        """(HR@k, NDCG@k) of the rows [r0, r1) of ctx, in groups of max(1, score_rows // N): score(ctx[c0:c1], cand_of(c0, c1)) and
        the rank of candidate tpos[c] in row c, the sums [hits, gains, rows, NaN flag] accumulated on the device in float64,
        all-reduced and read once.  who names the calling method in the NaN error.  seen_of: None, or _seen_masks' mask(c0, c1),
        handed to rank_of as its skip (the flag at the target's own position is ignored there)."""
        import torch
        tpos = tpos.to(torch.int32)
        sums = torch.zeros(4, dtype=torch.float64, device=eng.device)
        group = max(1, int(score_rows) // N)
        for c0 in range(r0, r1, group):
            c1 = min(r1, c0 + group)
            scores = score(ctx[c0:c1], cand_of(c0, c1))
            if seen_of is None:
                rank = eng.rank_of(scores, tpos[c0:c1]).double()
            else:
                rank = eng.rank_of(scores, tpos[c0:c1], skip=seen_of(c0, c1)).double()
            hit = rank < k
            sums[0] += hit.sum()
            sums[1] += torch.where(hit, 1.0 / torch.log2(rank + 2.0), torch.zeros_like(rank)).sum()
            sums[2] += c1 - c0
            sums[3] += torch.isnan(scores).any()
        hits, gains, rows, bad = (float(v) for v in self._all_reduce_sum(sums).cpu().numpy())
        if bad:
            raise ValueError('%s: predictions contain NaN' % who)
        return hits / rows, gains / rows

    # ---- candidates that are tuples of ids, and a candidate list per context ----------------------------
    # recommend / evaluate_ranking put ONE id at ONE column and leave the context's other ids alone.  Where an item's attributes are
    # fields of their own (frappe: the app's cost next to the app id) that scores rows that cannot occur; the methods below replace
    # several columns together, from one shared list or from a list per context.  Both pairs are wrappers with their own defaults
    # and messages around the same code: _scorer picks the engine call (an int field is the one-id form, which still goes to
    # score_candidates), _topk_sweep is the top-k loop of both recommend methods, _rank_targets the metric loop of both evaluations.
    def _tuple_fields(self, fields):
        cols = [fields] if isinstance(fields, (int, np.integer)) else list(fields)
        cols = [int(f) for f in cols]
        if not cols or len(set(cols)) != len(cols) or not all(0 <= f < self.num_field for f in cols):
            raise ValueError('fields must be a column or distinct columns of [0, %d), not %r' % (self.num_field, fields))
        return cols

    @staticmethod
    def _tuple_array(candidates, nf, lead, what):
        """candidates as int32 [..., nf] with `lead` leading axes; one field may come without the last axis."""
        cand = np.asarray(candidates)
        if nf == 1 and cand.ndim == lead:
            cand = cand[..., None]
        if cand.ndim != lead + 1 or cand.shape[-1] != nf or cand.size == 0 or cand.dtype.kind not in 'iu':
            raise ValueError('%s must be integer ids of shape %s' % (what, ('[C, N' if lead == 2 else '[N') + (', %d]' % nf if nf > 1 else ']')))
        return np.ascontiguousarray(cand.astype(np.int32))

    def recommend_tuples(self, contexts, fields, candidates, per_context=False, counts=None, k=10, skip=None, score_rows=1 << 22,
                         sweep='expand', exclude=None, by=None):
        """For every context row, the k candidates that score highest when their ids are put at the columns `fields` (an int or
        distinct columns) TOGETHER.  candidates: [N] / [N, nf] (one list for every context) or, with per_context, [C, N] /
        [C, N, nf] (a list per context); counts: optional [C] for per-context lists, list c holding counts[c] <= N candidates and
        padding behind them (any id may sit there; it is merged into the skip mask); skip: optional boolean [C, N] over candidate
        positions.  Returns host arrays (pos int32 [C, k] candidate POSITIONS in the caller's list, -1 padded - a tuple has no
        single id to return; scores float32 [C, k], NaN padded).  sweep: 'expand' (default) is bit for bit predict on the expanded
        rows; 'shared' serves one field at a served shape (ValueError otherwise); 'auto' takes it only there and for
        N >= SWEEP_MIN_N; 'tuples' is the tuple sweep (HipEngine.score_candidate_tuples_shared: everything without a swept field once
        per context) for any nf >= 1, equal to 'expand' to rounding, ValueError naming 'tuples' where (shape, nf) is not served
        (nf <= 4; nf = 3 at F = 10, K = 32 is not).  Measured at the frappe shape, nf = 2: 0.60 of expand's time for one shared list,
        0.79 for lists of 100 per context (profiles/sweep_tuples.md, one box); 'auto' never picks it.  Local to the calling rank: no
        collective.
        exclude / by: as in recommend(), the seen set of an owner being the tuples at `fields` of its rows of exclude with label > 0;
        one shared list only - per_context=True with exclude raises ValueError (positions then differ per context)."""
        import torch
        eng = self._ranking_engine()
        cols = self._tuple_fields(fields)
        seen = self._seen_args('recommend_tuples()', exclude, by, cols,
                               [('per_context', per_context, 'candidate positions then differ per context; one shared list only')])
        if not 1 <= int(k) <= 1024:
            raise ValueError('recommend_tuples(): k must be in [1, 1024]')
        ctx = self._contexts(eng, contexts)
        cand = torch.from_numpy(self._tuple_array(candidates, len(cols), 2 if per_context else 1, 'candidates')).to(eng.device)
        pos, val = self._topk_sweep(eng, ctx, cols, cand, per_context, counts, int(k), skip, score_rows, sweep, seen)
        return pos.cpu().numpy(), val.cpu().numpy()

    @staticmethod
    def _positions(cand, tgt):
        """Position in cand [N, nf] of every row of tgt [P, nf] - or in ids [N] of every id of [P] - the first one, should the list
        repeat an entry; N where it is missing.  On the device: one torch.unique(dim=0) over both."""
        import torch
        N = int(cand.shape[0])
        inv = torch.unique(torch.cat([cand, tgt]), dim=0, return_inverse=True)[1]      # one number per distinct tuple
        cs, order = torch.sort(inv[:N], stable=True)
        at = torch.searchsorted(cs, inv[N:]).clamp(max=N - 1)
        return torch.where(cs[at] == inv[N:], order[at], torch.full_like(at, N))

    @staticmethod
    def _draw_lists(rng, at, U, m):
        """The sampled protocol's draw, shared by evaluate_ranking_tuples and train_ranking: for every row r a list of m + 1 indices
        into a distinct set of U tuples - its target at[r] and m distinct others (one permutation of the set without the target per
        row) - with the target at a position drawn afterwards, for all rows at once.  Returns (lists int64 [P, m + 1], place [P])."""
        P = int(at.shape[0])
        lists = np.empty((P, m + 1), dtype=np.int64)                   # indices into the distinct set
        for r in range(P):
            neg = rng.permutation(U - 1)[:m]
            lists[r, 1:] = neg + (neg >= at[r])                        # the set without the target
        place = rng.randint(0, m + 1, size=P)
        lists[:, 0] = lists[np.arange(P), place]
        lists[np.arange(P), place] = at
        return lists, place

    @staticmethod
    def _check_sampler(who, sampler, negatives):
        if sampler not in ('host', 'device'):
            raise ValueError("%s: sampler must be 'host' or 'device', not %r" % (who, sampler))
        if sampler == 'device' and negatives is not None and int(negatives) > 1023:
            raise ValueError("%s: sampler='device' draws lists of at most 1024: negatives must be <= 1023, not %d" % (who, int(negatives)))

    @staticmethod
    def _negative_cdf(who, eng, negative_weights, negative_power, sampler, m, U, counts, host=False):
        """The cdf words of HipEngine.draw_lists_weighted on the device (int32 storage of cffm_amd.spec.weight_cdf, built on the
        host once per call; U words cross the bus), or None for negative_weights=None.  counts: a callable that returns the
        occurrence count of every distinct tuple as a device tensor [U] (for 'popularity'), or None where there is no data to count.
        host=True: (that, the same words as the host's uint32 array or None) - what cffm_amd.spec.logq_table reads."""
        import torch
        from .spec import weight_cdf
        if negative_weights is None:
            return (None, None) if host else None
        if sampler != 'device':
            raise ValueError("%s: negative_weights needs sampler='device', the only sampler that draws weighted lists (not %r)"
                             % (who, sampler))
        if isinstance(negative_weights, str):
            if negative_weights != 'popularity':
                raise ValueError("%s: negative_weights must be None, 'popularity' or an array of %d weights, not %r"
                                 % (who, U, negative_weights))
            if counts is None:
                raise ValueError("%s: negative_weights='popularity' counts the tuples of the data the candidates are built from; with "
                                 "explicit candidates pass negative_weights as an array of %d weights" % (who, U))
            power = float(negative_power)
            if not np.isfinite(power):
                raise ValueError('%s: negative_power must be finite, not %r' % (who, negative_power))
            w = counts().double().cpu().numpy() ** power
        else:
            w = np.asarray(negative_weights, dtype=np.float64)
            if w.shape != (U,):
                raise ValueError('%s: negative_weights must hold one weight per distinct tuple, shape (%d,), in the lexicographic order '
                                 'of the tuples, not shape %s' % (who, U, w.shape))
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError('%s: negative_weights must be non-negative and finite' % who)
        if int((w > 0).sum()) < m + 1:
            raise ValueError('%s: negative_weights has %d positive weights; lists of %d need at least %d'
                             % (who, int((w > 0).sum()), m + 1, m + 1))
        words = weight_cdf(w)
        dev = torch.from_numpy(words.view(np.int32)).to(eng.device)
        return (dev, words) if host else dev

    @staticmethod
    def _draw_lists_device(eng, seed, list0, at, U, m, cand, cdf=None, who=None, with_lists=False):
        """HipEngine.draw_lists for the lists list0 .. list0 + len(at) - 1, in as many calls as the 2^31 element bound of one call
        asks for (a list is a function of its id, so the split does not show): (tuples int32 [G, m + 1, nf], target int32 [G]).
        With cdf (from _negative_cdf) the lists are those of HipEngine.draw_lists_weighted, and a list that came back incomplete
        raises ValueError (one device reduction and one read per call of this function).  with_lists=True: (tuples, lists int32
        [G, m + 1] the indices the draw wrote, target)."""
        import torch
        G = int(at.shape[0])
        per = max(1, ((1 << 31) - 1) // ((m + 1) * int(cand.shape[1])))

        def draw(g0, a):
            if cdf is None:
                return eng.draw_lists(seed, g0, a, U, m, cand)
            return eng.draw_lists_weighted(seed, g0, a, cdf, m, cand)

        if G <= per:
            tuples, lists, target = draw(list0, at)
        else:
            parts = [draw(list0 + g0, at[g0:g0 + per]) for g0 in range(0, G, per)]
            tuples, lists, target = (torch.cat([p[i] for p in parts]) for i in range(3))
        if cdf is not None:
            short = int(((target < 0) & (at >= 0) & (at < U)).sum())
            if short:
                raise ValueError('%s: negative_weights is too skewed for lists of %d under the word cap of the weighted draw: %d of %d '
                                 'lists did not collect their %d negatives (cffm_amd.spec.draw_weighted_cap)' % (who, m + 1, short, G, m))
        return (tuples, lists, target) if with_lists else (tuples, target)

    def evaluate_ranking_tuples(self, data, fields, k=10, candidates=None, negatives=None, seed=0, score_rows=1 << 22, sweep='expand',
                                sampler='host', negative_weights=None, negative_power=0.75, exclude=None, by=None):
        """(HR@k, NDCG@k) over the rows of `data` with a positive label, the target being the row's own tuple at `fields`.
        negatives=None: one shared list - by default the distinct tuples at `fields` over the train split and `data`, sorted
        (torch.unique(dim=0) on the device); explicit candidates [N] / [N, nf] that lack a target raise ValueError.  negatives=m:
        the sampled protocol - every row is ranked in a list of its own: its target and m distinct tuples drawn without it from
        the distinct tuples of that set, with np.random.RandomState(seed) on the host (one permutation of the set per row).  The
        target's POSITION in its list is drawn from the same generator: ties go to the smaller position and CFFM scores tie often,
        so a target fixed at position 0 would win every tie.  m >= the number of distinct tuples raises ValueError.  Under a process
        group every rank draws all lists from the same seed and then takes its contiguous share of the rows.  The sums stay on the
        device in float64 and are read once, as in evaluate_ranking.  sweep: as in recommend_tuples ('tuples': the tuple sweep for the
        shared list and for the sampled lists alike).
        sampler: 'host' (default) is the draw above.  'device' draws the lists on the GPU (HipEngine.draw_lists(seed, 0, ...):
        cffm_amd.spec.draw_lists is the specification, list r a function of (seed, r) alone) - other lists than 'host' draws, of the
        same distribution, at most 1023 negatives; under a process group every rank draws its own share of the rows only.
        negative_weights (with negatives=m and sampler='device' only; a ValueError names it otherwise): None (default) draws the
        negatives uniformly, everything as without the keyword.  'popularity' draws them in proportion to count ** negative_power,
        count the number of rows (any label) of the train split plus `data` that carry the tuple; with explicit `candidates` there
        is nothing to count and a ValueError asks for an array.  An array [U] gives non-negative finite weights in the lexicographic
        order of the distinct tuples (a zero weight is never drawn).  The lists are those of HipEngine.draw_lists_weighted(seed, r0,
        ...) (cffm_amd.spec.draw_lists_weighted is the specification: successive sampling without replacement by rejection, list r
        a function of (seed, r) alone); they differ from the uniform device lists even for equal weights.  Fewer than m + 1
        positive weights, and weights so skewed that a list does not collect its m negatives under the word cap, raise ValueError.
        exclude / by (negatives=None only; default None: every call as without them): as in evaluate_ranking(), the seen set of an
        owner being the tuples at `fields` of its rows of exclude with label > 0.  With negatives=m a ValueError names exclude and
        negatives: drawn lists that avoid seen items belong to the draw kernels.
        Out of scope: hard-negative (model-scored) draws, seen-aware draws."""
        import torch
        self._check_sampler('evaluate_ranking_tuples()', sampler, negatives)
        eng = self._ranking_engine()
        cols = self._tuple_fields(fields)
        seen = self._seen_args('evaluate_ranking_tuples()', exclude, by, cols,
                               [('negatives=%r' % (negatives,), negatives is not None,
                                 'lists drawn without the seen items are not implemented; exclude filters the shared list (negatives=None)')])
        ids, y, _ = self._device_split(data)
        k = int(k)
        if k < 1:
            raise ValueError('evaluate_ranking_tuples(): k must be >= 1')
        colt = torch.tensor(cols, dtype=torch.long, device=eng.device)
        if candidates is None:
            cand = self._distinct(self._eval_splits(data), colt)
        else:
            cand = torch.from_numpy(self._tuple_array(candidates, len(cols), 1, 'candidates')).to(eng.device)
            if negatives is not None:
                cand = torch.unique(cand, dim=0)
        ctx = ids[y.reshape(-1) > 0]
        P, U = int(ctx.shape[0]), int(cand.shape[0])
        if P == 0:
            raise ValueError('evaluate_ranking_tuples() needs at least one row with a positive label')
        tgt = ctx[:, colt].to(torch.int32)
        tpos = self._positions(cand, tgt)
        missing = tpos == U
        if bool(missing.any()):
            raise ValueError('evaluate_ranking_tuples(): target %s at fields %s is not among the candidates'
                             % (tuple(int(v) for v in tgt[missing][0]), tuple(cols)))
        r0, r1, _ = self._row_share(P)
        N, cand_of = U, lambda c0, c1: cand
        if negatives is None and negative_weights is not None:
            raise ValueError('evaluate_ranking_tuples(): negative_weights weighs the drawn negatives; it needs negatives=m')
        if negatives is not None:
            m = int(negatives)
            if m < 1 or m >= U:
                raise ValueError('evaluate_ranking_tuples(): negatives must be in [1, %d): the distinct tuples without the target' % U)
            N = m + 1

            # rows of any label, in the order of cand; explicit candidates leave nothing to count
            counts = None if candidates is not None else lambda: self._distinct(self._eval_splits(data), colt, counts=True)
            cdf = self._negative_cdf('evaluate_ranking_tuples()', eng, negative_weights, negative_power, sampler, m, U, counts)
            if sampler == 'device':                                            # this rank's rows only: list r is row r's
                drawn, place = self._draw_lists_device(eng, seed, r0, tpos[r0:r1], U, m, cand, cdf, 'evaluate_ranking_tuples()')
                tpos = torch.cat([tpos.new_zeros(r0), place.to(tpos.dtype), tpos.new_zeros(P - r1)])
                cand_of = lambda c0, c1: drawn[c0 - r0:c1 - r0]
            else:
                lists, place = self._draw_lists(np.random.RandomState(seed), tpos.cpu().numpy(), U, m)
                lists = torch.from_numpy(lists).to(eng.device)
                tpos = torch.from_numpy(place).to(eng.device)
                cand_of = lambda c0, c1: cand[lists[c0:c1]]
        score = self._scorer(eng, sweep, cols, N, negatives is not None)
        seen_of = None if seen is None else self._seen_masks(eng, seen, cols, cand, ctx, N)
        return self._rank_targets('evaluate_ranking_tuples()', eng, score, ctx, cand_of, tpos, r0, r1, N, k, score_rows, seen_of)

    # ---- training on ranked lists ----------------------------------------------------------------------------
    def train_ranking(self, data, fields, negatives=4, loss='bpr', epochs=1, lists_per_step=None, seed=0, step='stages', sampler='host',
                      negative_weights=None, negative_power=0.75, hard_pool=None, logq=False):
        """Train on what evaluate_ranking_tuples(negatives=m) measures: every row of `data` with a positive label becomes a list of
        its own tuple at `fields` and `negatives` distinct tuples drawn without it from the distinct tuples at `fields` of `data`,
        the positive at a drawn position (the rule of evaluate_ranking_tuples), and the model takes Adagrad steps on the list loss
        'bpr' (mean softplus of negative minus positive score) or 'softmax' (cross entropy of the list) - HipEngine.train_step_lists,
        lists_per_step lists at a time (default batch_size // (negatives + 1)), ragged last step.  Per epoch the positives are
        permuted and the lists drawn with np.random.RandomState(seed + epoch).  Returns the per-epoch mean loss over the lists as a
        list of floats (read from the device once per epoch) and logs it.  The --lamda regulariser of the pointwise step is not part
        of the list step.  One GPU, replicated tables, Adagrad, and not loss_type='log_loss' (its forward leaves sigmoid(out), not
        the score): each refused with a ValueError that names it.
        step: 'stages' (default) takes every step through HipEngine.train_step_lists, the stage launches; 'fused' through
        train_step_lists_fused, the launches of the pointwise step, and raises a ValueError where a step's size is not served
        (HipEngine.list_step_ok, the ragged last step included); 'auto' takes the fused step where it is served, step by step, and the
        stage step elsewhere.
        sampler: 'host' (default) is the draw above.  'device' keeps the epoch permutation (RandomState(seed + epoch).permutation,
        the only thing that crosses the bus) and draws the epoch's lists on the GPU: list j of epoch e, the one of the j-th permuted
        positive, is list e * P + j of HipEngine.draw_lists(seed, ...) (cffm_amd.spec.draw_lists is the specification), a function of
        (seed, e * P + j) alone and so the same under every lists_per_step.  Other lists than 'host' draws, of the same
        distribution; at most 1023 negatives.
        negative_weights (with sampler='device' only; a ValueError names it otherwise): None (default) draws the negatives
        uniformly, everything as without the keyword.  'popularity' draws them in proportion to count ** negative_power, count the
        number of rows of `data` (any label) that carry the tuple - the usual remedy for uniform negatives that are almost all
        trivially easy on a long-tailed catalogue.  An array [U] gives non-negative finite weights in the lexicographic order of the
        distinct tuples (a zero weight is never drawn).  The cdf is built once per call on the host (cffm_amd.spec.weight_cdf; U
        words cross the bus) and list e * P + j is that of HipEngine.draw_lists_weighted(seed, ...): successive sampling without
        replacement by rejection, cffm_amd.spec.draw_lists_weighted the specification.  These lists differ from the uniform device
        lists even for equal weights.  The BPR and softmax losses are used as they are unless logq=True (below).  Fewer than negatives + 1 positive weights, and weights so skewed that a list does not collect its negatives
        under the word cap (checked after each epoch's draw, before its first step), raise ValueError.
        hard_pool (with sampler='device' only; a ValueError names both otherwise): None (default) trains on the drawn lists,
        everything as without the keyword.  hard_pool=p, negatives < p <= min(U - 1, 1023) over the U distinct tuples, is dynamic
        negative sampling: per epoch every positive draws a pool of p negatives instead of `negatives` (list e * P + j of the draw
        above at m = p, the weighted draw under negative_weights, whose checks then speak of lists of p + 1), and every step first
        scores its pools with the parameters as they stand before it (HipEngine.score_candidate_tuples, bit for bit predict) and
        trains on the `negatives` best-scored members of each pool, hardest first, in the order of HipEngine.topk, around the
        positive at a place drawn from (seed, e * P + j) (HipEngine.pick_hard; cffm_amd.spec.pick_hard is the specification) -
        three launches ahead of the unchanged list step at the frappe shape, and the same lists under every lists_per_step only as
        far as the parameters that score them are the same.  The losses are used as they are: no correction of the softmax for the
        selection is applied.
        logq (default False: every call, launch and bit as without the keyword): True corrects the sampled softmax for the proposal q
        the negatives were drawn from - the weights of negative_weights, or 1 / U for the uniform device draw.  The positive, in
        every list with probability 1, takes no correction; a negative n of a list with positive t has log(m q_n / (1 - q_t))
        subtracted from its score inside the loss (m = negatives), the importance weight of sum_{j != t} exp(s_j) under the draw's
        own proposal q_j / (1 - q_t) - the with-replacement correction, meant for negatives far fewer than the distinct tuples.  The
        table (cffm_amd.spec.logq_table, float32 [U, 2]) is built once per call on the host and U x 2 floats cross the bus; every
        step hands its lists' indices and the table to the list step (HipEngine.train_step_lists[_fused](..., lists, corr): the same
        launches), and the returned per-epoch loss is the mean corrected term.  Ranking (evaluate_ranking_tuples) is on raw scores
        and does not change.  Needs sampler='device', loss='softmax' and hard_pool=None: a ValueError names the keyword at fault
        (no agreed correction of pairwise BPR exists, and the selection bias of a hard pool is a different problem).
        Out of scope: the multi-GPU list step, other optimizers."""
        import torch
        from . import hip
        self._check_sampler('train_ranking()', sampler, negatives)
        if logq:
            if sampler != 'device':
                raise ValueError("train_ranking(): logq=True needs sampler='device', whose draws hand on the list indices and the "
                                 "proposal (not sampler=%r)" % (sampler,))
            if loss in hip.LIST_LOSS_IDS and loss != 'softmax':
                raise ValueError("train_ranking(): logq=True corrects the sampled softmax: it needs loss='softmax', not loss=%r" % (loss,))
            if hard_pool is not None:
                raise ValueError('train_ranking(): logq=True needs hard_pool=None: the selection bias of a scored pool is not what '
                                 'logQ corrects (hard_pool=%r)' % (hard_pool,))
        if hard_pool is not None and sampler != 'device':
            raise ValueError("train_ranking(): hard_pool needs sampler='device', the only sampler that draws the pool (not sampler=%r)"
                             % (sampler,))
        if step not in ('stages', 'fused', 'auto'):
            raise ValueError("train_ranking(): step must be 'stages', 'fused' or 'auto', not %r" % (step,))
        if self.optimizer_type != 'AdagradOptimizer':
            raise ValueError('train_ranking(): the list step implements AdagradOptimizer, not --optimizer %s' % self.optimizer_type)
        if self.loss_type == 'log_loss':
            raise ValueError("train_ranking(): --loss_type log_loss leaves sigmoid(out) in the forward, not the score the list losses rank")
        if loss not in hip.LIST_LOSS_IDS:
            raise ValueError("train_ranking(): loss must be one of %s, not %r" % (sorted(hip.LIST_LOSS_IDS), loss))
        if os.environ.get('CFFM_TABLES', 'replicated') == 'sharded' or self._sh is not None:
            raise ValueError('train_ranking(): CFFM_TABLES=sharded is not implemented for the list step; it runs on replicated tables')
        if self.engine is None:
            self.build_graph()
        if self.world > 1:
            raise ValueError('train_ranking(): a process group of %d ranks is not implemented for the list step; it runs on one GPU'
                             % self.world)
        eng = self.engine
        cols = self._tuple_fields(fields)
        m, epochs = int(negatives), int(epochs)
        ids, y, _ = self._device_split(data)
        colt = torch.tensor(cols, dtype=torch.long, device=eng.device)
        cand = self._distinct([data], colt)
        ctx = ids[y.reshape(-1) > 0]
        P, U = int(ctx.shape[0]), int(cand.shape[0])
        if P == 0:
            raise ValueError('train_ranking() needs at least one row with a positive label')
        if m < 1 or m >= U:
            raise ValueError('train_ranking(): negatives must be in [1, %d): the distinct tuples without the target' % U)
        per = int(self.batch_size // (m + 1) if lists_per_step is None else lists_per_step)
        if per < 1:
            raise ValueError('train_ranking(): lists_per_step must be >= 1 (batch_size %d holds no list of %d)' % (self.batch_size, m + 1))
        drawn = m                                                              # negatives per drawn list: the pool under hard_pool
        if hard_pool is not None:
            drawn = int(hard_pool)
            if not m < drawn <= min(U - 1, 1023):
                raise ValueError('train_ranking(): hard_pool must be in (negatives, min(U - 1, 1023)] = (%d, %d]: a pool larger than '
                                 'the negatives picked from it, drawn from the %d distinct tuples without the target, not %d'
                                 % (m, min(U - 1, 1023), U, drawn))
        at_dev = self._positions(cand, ctx[:, colt].to(torch.int32))
        at = at_dev.cpu().numpy() if sampler == 'host' else None
        cdf, cdf_host = self._negative_cdf('train_ranking()', eng, negative_weights, negative_power, sampler, drawn, U,
                                           lambda: self._distinct([data], colt, counts=True), host=True)
        corr = None
        if logq:                                                               # once per call: U x 2 floats cross the bus
            from .spec import logq_table
            corr = torch.from_numpy(logq_table(cdf_host, m, U)).to(eng.device)
        means = []
        for epoch in range(epochs):
            t1 = time()
            rng = np.random.RandomState(seed + epoch)
            perm = rng.permutation(P)
            if sampler == 'device':
                permt = torch.from_numpy(perm).to(eng.device)
                rows = ctx[permt]
                tuples, lists, target = self._draw_lists_device(eng, seed, epoch * P, at_dev[permt], U, drawn, cand, cdf,
                                                                'train_ranking()', with_lists=True)
            else:
                lists, place = self._draw_lists(rng, at[perm], U, m)
                rows = ctx[torch.from_numpy(perm).to(eng.device)]
                tuples = cand[torch.from_numpy(lists).to(eng.device)]              # [P, m + 1, nf]
                target = torch.from_numpy(place.astype(np.int32)).to(eng.device)
            total = torch.zeros(1, dtype=torch.float64, device=eng.device)         # sum over the lists, read once per epoch
            for r0 in range(0, P, per):
                r1 = min(P, r0 + per)
                fused = step == 'fused' or (step == 'auto' and eng.list_step_ok((r1 - r0) * (m + 1)))
                run = eng.train_step_lists_fused if fused else eng.train_step_lists
                if hard_pool is None:
                    step_tuples, step_target = tuples[r0:r1].contiguous(), target[r0:r1]
                else:                                                          # the pool scored as the parameters stand now
                    scores = eng.score_candidate_tuples(rows[r0:r1], cols, tuples[r0:r1])
                    step_tuples, _, step_target = eng.pick_hard(seed, epoch * P + r0, scores, target[r0:r1], m, tuples=tuples[r0:r1])
                if logq:
                    step_loss = run(rows[r0:r1], cols, step_tuples, step_target, loss, lists=lists[r0:r1], corr=corr)
                else:
                    step_loss = run(rows[r0:r1], cols, step_tuples, step_target, loss)
                total += step_loss.double() * (r1 - r0)
            means.append(float(total.cpu()[0]) / P)
            self._info('Ranking epoch %d [%.1f s] %s loss over %d lists of %d: %.6f' % (epoch + 1, time() - t1, loss, P, m + 1, means[-1]))
        return means

    # ---- host-side helpers with the reference's list semantics (CFFM.py:556-635) -------------------------
    def shuffle_in_unison_scary(self, x, y):
        x_, y_ = shuffle(x, y, random_state=self.random_seed)
        return x_, y_

    def get_random_block_from_data(self, data, batch_size):
        """A block from a random start, filled forward over rows as long as the start row, then BACKWARD from the
        same start (which re-adds the start row when the forward fill stopped short) - CFFM.py:560-581."""
        start_index = self.batch_rng.randint(0, len(data['Y']) - batch_size)
        want = len(data['X'][start_index])
        X, Y = [], []
        for step in (1, -1):
            i = start_index
            while len(X) < batch_size and 0 <= i < len(data['X']) and len(data['X'][i]) == want:
                Y.append([data['Y'][i]])
                X.append(data['X'][i])
                i += step
        return {'X': X, 'Y': Y}

    def get_ordered_block_from_data(self, data, batch_size, index):
        start_index = index * batch_size
        X, Y = [], []
        i = start_index
        while len(X) < batch_size and i < len(data['X']) and len(data['X'][i]) == len(data['X'][start_index]):
            Y.append(data['Y'][i])
            X.append(data['X'][i])
            i += 1
        return {'X': X, 'Y': Y}

    def eva_termination(self, valid):
        if len(valid) > 5:
            if valid[-1] > valid[-2] > valid[-3] > valid[-4] > valid[-5]:
                return True
        return False

    def calculate_parameters(self):
        total_parameters = logged_param_count(self.config)
        if self.verbose > 0:
            self._info("#params: %d" % total_parameters)
        return total_parameters

    def create_save_folder(self, save_file):
        os.makedirs(save_file, exist_ok=True)          # every rank of a job names the same folder: no exists-then-create race

    # ---- checkpoint: this model's tensors AND the optimizer slots (the reference restore is broken, Q7) ---------------
    # A plain dict of tensors and scalars: loads with torch.load(weights_only=True), no pickled code.
    def save(self, save_file):
        import torch
        from .dist import save_sharded, tensors_of as t
        if self._sh is not None:                       # row-sharded: one file per rank (cffm_amd.dist.save_sharded)
            import torch.distributed as dist
            save_sharded(self.engine, save_file, self.rank, self.world, opt_step=int(getattr(self.engine, 'opt_step', 0)))
            dist.barrier()                             # on return every shard is on disk (a restore reads shard 0 on every rank)
            return
        cfg = {k: (v if isinstance(v, (int, float, str)) else float(v)) for k, v in self.config.__dict__.items()}
        torch.save({'format': 2, 'config': cfg, 'params': t(self.engine.export_params()),
                    'accumulators': t(self.engine.export_accumulators()),
                    'second_moments': t(self.engine.export_second_moments()), 'opt_step': int(self.engine.opt_step)},
                   save_file + '.pt')

    def load(self, save_file):
        import torch
        from .dist import arrays_of as n, load_sharded
        if self._sh is not None:                       # the shards a run at THIS world size wrote; dist.merge_shards for world 1
            self.engine.opt_step = load_sharded(self.engine, save_file, self.rank, self.world)
            return
        blob = torch.load(save_file + '.pt', weights_only=True)
        saved = blob.get('config', {})
        for k in ('M', 'F', 'K', 'D'):
            if k in saved and int(saved[k]) != int(getattr(self.config, k)):
                raise ValueError('checkpoint %s.pt was written for %s=%s, this model has %s' % (save_file, k, saved[k], getattr(self.config, k)))
        self.engine.load_params(n(blob['params']), n(blob['accumulators']), n(blob.get('second_moments')))
        self.engine.opt_step = int(blob.get('opt_step', 0))


def main(argv=None):
    args = parse_args(argv)
    configure_logging('logging.log')
    if args.verbose > 0:
        logging.info(
            "CFFM: dataset=%s, factors=%d, loss_type=%s, #epoch=%d, batch=%d, lr=%.4f, lambda=%.1e, keep=%s, optimizer=%s"
            ", batch_norm=%d, num_field=%d, linear_att=%d, att_dim=%d,lamda_att=%.2f,inner_conv=%d,gamma_inner=%.1f,"
            "outer_conv=%d,beta_outer=%.1f, activation=%s"
            % (args.dataset, args.inner_dims, args.loss_type, args.epoch, args.batch_size, args.lr, args.lamda,
               ast.literal_eval(args.keep), args.optimizer, args.batch_norm, args.num_field, args.linear_att, args.att_dim,
               args.lamda_att, args.inner_conv, args.gamma_inner, args.outer_conv, args.beta_outer, args.activation))
    data = DATA.LoadData(args.path, args.dataset, args.loss_type)
    save_file = 'pretrain/CFFM/%s_%d/%s_%d' % (args.dataset, args.inner_dims, args.dataset, args.inner_dims)
    t1 = time()
    cf_fm = CFFM(data.features_M, args.pretrain, save_file, args.inner_dims, args.outer_dims, args.loss_type,
                 args.epoch, args.batch_size, args.lr, args.lamda, ast.literal_eval(args.keep), args.optimizer, args.batch_norm,
                 args.verbose, args.tensorboard, args.num_field, args.linear_att, args.att_dim, args.lamda_att,
                 args.inner_conv, args.gamma_inner, args.outer_conv, args.beta_outer, args.activation)
    cf_fm.train(data)
    best_valid_score = min(cf_fm.valid_rmse)
    best_epoch = cf_fm.valid_rmse.index(best_valid_score)
    logging.info("Best Iter of RMSE (validation)= %d train = %.4f, valid = %.4f, test = %.4f [%.1f s]"
                 % (best_epoch + 1, cf_fm.train_rmse[best_epoch], cf_fm.valid_rmse[best_epoch],
                    cf_fm.test_rmse[best_epoch], time() - t1))
    best_r2 = cf_fm.valid_r2.index(max(cf_fm.valid_r2))
    logging.info("Best Iter of R2 (validation)= %d train = %.4f, valid = %.4f, test = %.4f [%.1f s]"
                 % (best_epoch + 1, cf_fm.train_r2[best_r2], cf_fm.valid_r2[best_r2], cf_fm.test_r2[best_r2],
                    time() - t1))       # prints best_epoch + 1 from the RMSE search, as the reference does (Q15)
    return cf_fm


if __name__ == '__main__':
    main()
