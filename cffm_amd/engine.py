"""Device-side state and step functions of the CFFM hot path: the replacement for the TF session.

``HipEngine`` owns what ``tf.Session`` owned in the reference (CFFM.py:160): the variables and their
Adagrad accumulators, resident in HBM for the life of the object as torch tensors, plus a per-batch-size
workspace.  ``predict`` and ``train_step`` are the two ``sess.run`` call shapes (CFFM.py:596, :200); both
are single calls into libcffm_hip.so, asynchronous on torch's current stream.
"""
import ctypes as C

import numpy as np
import torch

from . import hip
from .spec import ADAGRAD_INIT_ACC, TABLES, CFFMConfig, init_params, param_shapes

# theta member -> reference variable name (reshaped flat, row-major)
_THETA_MEMBERS = [
    ('att_W', 'bias_W'), ('att_b', 'bias_b'), ('bias', 'bias'),
    ('inner_cw', 'inner_layer_conv_weight_0'), ('inner_cb', 'inner_layer_conv_bias_0'),
    ('inner_dw', 'dense_kernel'), ('inner_db', 'dense_bias'),
    ('d1_w', 'dense_1_kernel'), ('d1_b', 'dense_1_bias'), ('d2_w', 'dense_2_kernel'), ('d2_b', 'dense_2_bias'),
    ('lin_w', 'dense_3_kernel'), ('lin_b', 'dense_3_bias'),
]


def _ptr(t):
    """Borrowed device pointer of a torch tensor as a plain integer (0 for None): what both bindings take."""
    return t.data_ptr() if t is not None else 0


class WorkspacePool(object):
    """ONE grow-only byte buffer plus the bookkeeping that captured HIP graphs need.

    A captured graph has the buffer's address baked into its kernel arguments.  Every re-allocation starts a new
    GENERATION; ``pin()`` says "a graph now references the current generation" and returns that generation, ``unpin(gen)``
    says that graph was dropped or re-captured.  A buffer that is outgrown while its generation is pinned is RETIRED (kept
    alive) and freed the moment the last pin of ITS generation goes - not when the pin count of all generations reaches 0:
    with two captured batch shapes one regrowth used to leave a ~50 GB buffer (F32 D64 B8192) alive for as long as any
    graph existed.  ``alloc(nbytes)`` is the allocator (torch.empty on the device; tests pass a host one)."""

    def __init__(self, alloc):
        self._alloc = alloc
        self.buf = None
        self.generation = 0
        self.pins = {}          # generation -> captured graphs that reference that generation's buffer
        self.retired = {}       # generation -> outgrown buffer those graphs may still replay against

    def get(self, nbytes):
        nbytes = int(nbytes)
        if self.buf is None or self.buf.numel() < nbytes:
            if self.buf is not None:
                if self.pins.get(self.generation, 0) > 0:
                    self.retired[self.generation] = self.buf
                self.generation += 1
            self.buf = None                               # release (unless retired) before allocating the larger one
            self.buf = self._alloc(nbytes)
        return self.buf

    def pin(self):
        self.pins[self.generation] = self.pins.get(self.generation, 0) + 1
        return self.generation

    def unpin(self, generation):
        left = self.pins.get(generation, 0) - 1
        if left > 0:
            self.pins[generation] = left
        else:
            self.pins.pop(generation, None)
            self.retired.pop(generation, None)            # the last graph of that generation is gone: free its buffer

    def retired_bytes(self):
        return sum(int(b.numel()) for b in self.retired.values())


class HipEngine(object):
    def __init__(self, cfg, params=None, seed=2021, device='cuda:0', table_seed=None, table_rows=(0, 1)):
        if not torch.cuda.is_available():
            raise RuntimeError('cffm_amd.HipEngine needs an MI355X (torch.cuda.is_available() is False); '
                               'there is no CPU fallback')
        hip.load()
        self.lib = hip.fast()                         # pybind11 layer (ctypes when it is not built): integer pointers
        self.cfg = cfg
        self.device = torch.device(device)
        self.shape = hip.make_shape(cfg)
        self.tl = hip.theta_layout(self.shape)
        self._ws = {}
        self._pool = WorkspacePool(lambda nbytes: torch.empty(nbytes, dtype=torch.uint8, device=self.device))
        self._eval_scratch = None
        self._flat_dirty = False                      # dense-image route: the image is zero on entry, zero on exit
        self._host_only = {}
        self.row_grad_width = 1 + cfg.K + cfg.D + 1   # floats of a row-gradient record (id bits | dEi | dEo | dfb)
        self.packed_width = cfg.K + cfg.D + 4         # floats of a packed row (inner | outer | bias, 0, 0, 0)
        # params == 'device': the three tables are drawn ON the GPU with the reference's distributions (N(0, 0.1),
        # N(0, 0.01), exact zeros - CFFM.py:257-277); for vocabularies where a host-side draw + copy of M*(K+D) floats
        # would dominate start-up (10 M features: 5 GB).  Dense parameters still come from init_params(seed); the device
        # draw of the tables uses table_seed (default: seed).  Row-sharded ranks pass ONE seed for the replicated dense
        # parameters and table_seed = seed + rank for their own shard of the tables.
        # params == 'device_rows': the tables are drawn on the GPU BY GLOBAL ROW (cffm_init_table_rows; spec.table_rows is its
        # numpy twin): local row l holds global row row0 + l * row_step with table_rows = (row0, row_step), and a value depends
        # on (table_seed, global row, table, column) alone.  Rank r of G passes (r, G) and ONE table_seed on every rank, a single
        # process (0, 1): the model no longer depends on the world size.  'device' above is left as it is.
        by_row = isinstance(params, str) and params == 'device_rows'
        device_tables = (isinstance(params, str) and params == 'device') or by_row
        if isinstance(params, str) and not device_tables:
            raise ValueError("params must be a dict, None, 'device' or 'device_rows', not %r" % (params,))
        if params is None or device_tables:
            params = init_params(cfg, seed=seed, tables=not device_tables)
        n = int(self.tl.n)
        dev = self.device
        # optimizer slots (CFFM.py:517-529): Adagrad accumulators start at 1e-8, Momentum accumulators / Adam m, v at 0
        self.acc0 = acc0 = ADAGRAD_INIT_ACC if cfg.optimizer == 'AdagradOptimizer' else 0.0
        # ONE table of the state: a (theta, inner, outer, fbias) set of the parameters, one of the first slots and, for Adam, one of the
        # second moments.  The named attributes alias these tensors; load, export and replicated_state walk self._sets.
        sizes = ((n,), (cfg.M, cfg.K), (cfg.M, cfg.D), (cfg.M,))
        self._sets = [tuple(torch.full(sz, fill, dtype=torch.float32, device=dev) for sz in sizes)
                      for fill in (0.0, acc0) + ((0.0,) if cfg.optimizer == 'AdamOptimizer' else ())]
        tabs = [hip.Tables(*(t.data_ptr() for t in st[1:])) for st in self._sets]
        self.theta, self.inner, self.outer, self.fbias = self._sets[0]
        self.theta_acc, self.inner_acc, self.outer_acc, self.fbias_acc = self._sets[1]
        self.tables, self.tables_acc = tabs[:2]
        self.theta_acc2 = self.tables_acc2 = None
        if len(self._sets) > 2:                                      # second moment
            self.theta_acc2, self.inner_acc2, self.outer_acc2, self.fbias_acc2 = self._sets[2]
            self.tables_acc2 = tabs[2]
        self.grad = torch.zeros(n + 4, dtype=torch.float32, device=dev)[:n]      # +4: loss-sum slot of the DP step
        self._grad_full = self.grad._base if self.grad._base is not None else self.grad
        self.opt_step = 0
        self.loss_buf = torch.zeros(1, dtype=torch.float32, device=dev)
        # addresses of the small host structs (kept alive by self)
        self._s = C.addressof(self.shape)
        self._t = C.addressof(self.tables)
        self._ta = C.addressof(self.tables_acc)
        self._ta2 = C.addressof(self.tables_acc2) if self.tables_acc2 is not None else 0
        self.load_params(params)
        if by_row:
            self.init_table_rows(int(seed if table_seed is None else table_seed), int(table_rows[0]), int(table_rows[1]))
        elif device_tables:
            gen = torch.Generator(device=dev).manual_seed(int(seed if table_seed is None else table_seed))
            self.inner.normal_(0.0, 0.1, generator=gen)
            self.outer.normal_(0.0, 0.01, generator=gen)

    def init_table_rows(self, table_seed, row0=0, row_step=1):
        """(Re)draw the three tables by global row: local row l <- global row row0 + l * row_step (cffm_init_table_rows).  The
        optimizer slots are not touched."""
        hip.check(self.lib.cffm_init_table_rows(self._s, self._t, int(table_seed) & 0xffffffffffffffff, int(row0), int(row_step),
                                                int(self.cfg.M), self._stream()))

    def replicated_state(self, tables=True):
        """Tensors that must be bit-identical on every rank of a multi-GPU job (cffm_amd.dist.sync_replicas): the dense
        parameters and their optimizer slots; with ``tables`` (data-parallel mode) also the three tables and their slots.
        In row-sharded mode the tables are per-rank shards and stay out."""
        return [st[0] for st in self._sets] + ([t for st in self._sets for t in st[1:]] if tables else [])

    # ---- named parameters <-> device buffers -------------------------------------------------------
    def _members(self):
        out = [(getattr(self.tl, m), name) for m, name in _THETA_MEMBERS]
        for l in range(self.tl.live):
            out.append((self.tl.conv_w[l], 'outer_layer_conv_weight_%d' % l))
            out.append((self.tl.conv_b[l], 'outer_layer_conv_bias_%d' % l))
        return out

    def _pack(self, name, v):
        """Reference variable -> its flat image inside theta (conv weights/biases are channel-padded to Pp)."""
        v = np.asarray(v, dtype=np.float32)
        P, Pp = self.tl.P, self.tl.Pp
        if name.startswith('outer_layer_conv_weight_'):
            out = np.zeros((4, Pp, Pp), dtype=np.float32)
            out[:, :P, :P] = v.reshape(4, P, P)
            return out.reshape(-1)
        if name.startswith('outer_layer_conv_bias_'):
            out = np.zeros(Pp, dtype=np.float32)
            out[:P] = v.reshape(-1)
            return out
        return v.reshape(-1)

    def _unpack(self, name, flat, off, shp):
        P, Pp = self.tl.P, self.tl.Pp
        if name.startswith('outer_layer_conv_weight_'):
            return flat[off:off + 4 * Pp * Pp].reshape(4, Pp, Pp)[:, :P, :P].reshape(shp).copy()
        if name.startswith('outer_layer_conv_bias_'):
            return flat[off:off + P].copy()
        n = int(np.prod(shp)) if shp else 1
        return flat[off:off + n].reshape(shp).copy()

    def load_params(self, params, accs=None, accs2=None):
        shapes = param_shapes(self.cfg)
        self._load_set(0, params, 'inner_embeddings' in params)  # absent: tables initialised on the device (params='device')
        trained = set(n for _, n in self._members()) | set(TABLES)
        self._host_only = {k: np.array(params[k], dtype=np.float32) for k in shapes if k not in trained and k in params}
        if accs is not None:
            self._load_set(1, accs)
        if accs2 is not None and self.theta_acc2 is not None:
            self._load_set(2, accs2)

    def _load_set(self, s, values, tables=True):
        """Set s of self._sets from reference variables by name: the dense members packed into the flat image, then the three tables.
        What no member covers keeps the set's initial value: 0, and in the first slots (s == 1) the initial accumulator acc0."""
        flat, fill = self._sets[s][0], np.float32(self.acc0 if s == 1 else 0.0)
        host = np.full(int(self.tl.n), fill, dtype=np.float32)
        for off, name in self._members():
            v = self._pack(name, values[name])
            if s == 1 and name.startswith('outer_layer_conv_'):
                v = np.where(v == 0, fill, v)                          # pads keep the initial accumulator
            host[off:off + v.size] = v
        flat.copy_(torch.from_numpy(host))
        if tables:
            for t, k in zip(self._sets[s][1:], TABLES):
                v = np.asarray(values[k], dtype=np.float32)
                t.copy_(torch.from_numpy(v.reshape(-1) if t.dim() == 1 else v))

    def _export(self, flat, *tables):
        """The flat image by reference variable name; with (inner, outer, fbias) also the three tables."""
        shapes = param_shapes(self.cfg)
        host = flat.detach().cpu().numpy()
        out = {}
        for off, name in self._members():
            out[name] = self._unpack(name, host, off, shapes[name])
        for k, t in zip(TABLES, tables):
            v = t.detach().cpu().numpy()
            out[k] = (v.reshape(-1, 1) if k == 'feature_bias' else v).copy()
        return out

    def export_params_dense(self):
        """Every variable except the three tables (for vocabularies where a host copy of the tables is not wanted)."""
        out = self._export(self.theta)
        out.update({k: v.copy() for k, v in self._host_only.items()})
        return out

    def export_params(self):
        out = self._export(*self._sets[0])
        out.update({k: v.copy() for k, v in self._host_only.items()})
        return out

    def export_accumulators(self):
        return self._export(*self._sets[1])

    def export_second_moments(self):
        """Adam's v slots (None for the other optimizers)."""
        return self._export(*self._sets[2]) if self.theta_acc2 is not None else None

    def export_grad(self):
        """Dense-parameter gradients of the last backward, by reference variable name."""
        return self._export(self.grad)

    # ---- workspace ---------------------------------------------------------------------------------
    def workspace(self, B):
        """(buffer, layout) for a batch of B rows.  ONE buffer serves every batch size: the library recomputes the
        layout from B on every call, and a call only needs ``layout(B).bytes`` bytes from the start of the buffer, so
        the buffer is re-allocated exactly when a layout asks for more bytes than it has (the byte count is NOT monotonic
        in B - the slab plan of the backward changes with B - hence the check on bytes, never on B).  It only ever grows;
        at F32 D64 B8192 it is ~50 GB, so one copy per distinct B would exhaust HBM within a few steps.

        A captured HIP graph (DataParallelStep(use_graph=True)) has the buffer's address baked into its kernel arguments:
        see WorkspacePool - an outgrown buffer is kept alive exactly as long as a graph captured against it is pinned, and
        ``ws_generation`` changes so that the owner of the graph re-captures against the new buffer."""
        B = int(B)
        wl = self._ws.get(B)
        if wl is None:
            if len(self._ws) > 4096:                     # layouts are tiny structs, but do not hoard them forever
                self._ws = {k: v for k, v in self._ws.items() if not isinstance(k, int)}
            wl = hip.ws_layout(self.shape, B)
            self._ws[B] = wl
        return self._pool.get(wl.bytes), wl

    @property
    def ws_generation(self):
        return self._pool.generation

    def reserve_workspace(self, B):
        """Grow the workspace to what a batch of B rows needs (e.g. evaluate()'s 8192-row blocks) BEFORE a graph is
        captured, so that no later call outgrows the captured buffer."""
        return self.workspace(B)[0]

    def pin_workspace(self):
        """A graph that references the current workspace buffer exists from now on; returns the generation to unpin."""
        return self._pool.pin()

    def unpin_workspace(self, generation):
        """The graph pinned at `generation` was dropped or re-captured."""
        self._pool.unpin(generation)

    def ws_tensor(self, B, member, shape, dtype=torch.float32, index=None):
        """View of one workspace intermediate (for the parity tests)."""
        buf, wl = self.workspace(B)
        off = getattr(wl, member)
        if index is not None:
            off = off[index]
        n = int(np.prod(shape))
        itemsize = torch.empty(0, dtype=dtype).element_size()
        return buf[int(off):int(off) + n * itemsize].view(dtype).reshape(shape)

    def _stream(self):
        return int(torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _ids(ids):
        if ids.dtype != torch.int32 or not ids.is_contiguous():
            ids = ids.to(torch.int32).contiguous()
        return ids

    @staticmethod
    def _labels(y):
        """y as contiguous float32 [B]."""
        y = y.reshape(-1)
        if y.dtype != torch.float32 or not y.is_contiguous():
            y = y.to(torch.float32).contiguous()
        return y

    def _cached(self, key, make):
        """self._ws[key], made by make() on first use and kept."""
        v = self._ws.get(key)
        if v is None:
            v = self._ws[key] = make()
        return v

    def _contexts(self, ctx):
        """ctx as contiguous int32 [C, F]."""
        ctx, F = self._ids(ctx), int(self.cfg.F)
        if ctx.dim() != 2 or int(ctx.shape[1]) != F:
            raise ValueError('contexts must be [C, %d] feature ids' % F)
        return ctx

    def _fields(self, fields, who, block=None):
        """`fields`, a column or several, as a list of 1 to F distinct ints of [0, F).  block: the piece size of an expand sweep,
        refused in the same message where it is < 1."""
        F = int(self.cfg.F)
        fields = [int(f) for f in (fields if hasattr(fields, '__len__') else [fields])]
        nf = len(fields)
        if not 1 <= nf <= F or len(set(fields)) != nf or not all(0 <= f < F for f in fields) or (block is not None and block < 1):
            raise ValueError('%s: needs %s1 to %d distinct fields of [0, %d)' % (who, '' if block is None else 'block >= 1 and ', F, F))
        return fields

    # ---- the two sess.run call shapes ---------------------------------------------------------------
    def predict(self, ids):
        """sess.run(self.out) (CFFM.py:596): int32 ids [B,F] on device -> fp32 [B] on device."""
        ids = self._ids(ids)
        B = ids.shape[0]
        if B == 0:
            return torch.empty(0, dtype=torch.float32, device=self.device)
        buf, _ = self.workspace(B)
        out = torch.empty(B, dtype=torch.float32, device=self.device)
        hip.check(self.lib.cffm_predict(self._s, self._t, _ptr(self.theta), _ptr(ids),
                                        B, _ptr(buf), _ptr(out), self._stream()))
        return out

    def eval_sums(self, ids, y, lo, hi, block=8192):
        """evaluate()'s sweep (CFFM.py:590-614) entirely on the device: ordered blocks of rows through cffm_predict, the
        clip to [lo, hi] and the float64 sums the two metrics need (cffm_eval_sums).  Returns a float64 device tensor
        [sum (y - p)^2, sum y, sum y^2]; nothing is copied to the host and nothing synchronises here."""
        ids, y = self._ids(ids), self._labels(y)
        n = int(ids.shape[0])
        sums = torch.zeros(3, dtype=torch.float64, device=self.device)
        for s0 in range(0, n, block):
            m = min(block, n - s0)
            self.eval_sums_add(self.predict(ids[s0:s0 + m]), y[s0:s0 + m], lo, hi, sums)
        return sums

    def eval_sums_add(self, pred, y, lo, hi, sums):
        """One block of that sweep for predictions that are already there (the row-sharded forward, ShardedStep.eval_sums):
        clip pred [m] to [lo, hi] and ADD the three float64 sums over (pred, y) onto sums [3]."""
        m = int(pred.shape[0])
        if self._eval_scratch is None:
            self._eval_scratch = torch.empty(int(self.lib.cffm_eval_scratch_bytes()), dtype=torch.uint8, device=self.device)
        hip.check(self.lib.cffm_eval_sums(_ptr(pred), _ptr(self._labels(y)), m, float(lo), float(hi), _ptr(self._eval_scratch),
                                          _ptr(sums), self._stream()))
        return sums

    # ---- candidate ranking (csrc/rank.hip): scores of (context, candidate) pairs, top-k and rank-of-target on the device ----
    def score_candidates(self, ctx, field, cand, block=8192):
        """Raw predictions of every (context, candidate) pair: ctx int32 [C,F] and cand int32 [N] on the device -> fp32 [C,N] on
        the device, row c being context c with its id at `field` replaced by each candidate in turn.  The flattened [C*N] range
        is swept in consecutive pieces of `block` rows (ragged last one): cffm_expand_candidates writes a piece's id rows,
        cffm_predict writes its outputs into the piece's slice of the result.  The ordinary workspace serves every piece, as in
        eval_sums; nothing synchronises."""
        ctx, cand = self._contexts(ctx), self._ids(cand.reshape(-1))
        C, F = int(ctx.shape[0]), int(self.cfg.F)
        N, block, field = int(cand.numel()), int(block), int(field)
        if N < 1 or block < 1 or not 0 <= field < F:
            raise ValueError('score_candidates: needs a candidate, block >= 1 and 0 <= field < %d' % F)
        expand = self.lib.cffm_expand_candidates
        return self._piece_sweep(C, N, block, lambda s0, m, ids, st: expand(self._s, _ptr(ctx), C, field, _ptr(cand), N, s0, m, ids, st))

    def _piece_sweep(self, n_ctx, N, block, expand):
        """The sweep of score_candidates and score_candidate_tuples: the flattened [n_ctx * N] range in consecutive pieces of `block`
        rows, expand(s0, m, ids, stream) - the caller's expand entry point - writing a piece's id rows into the one reused buffer and
        cffm_predict its outputs into the piece's slice of the result -> fp32 [n_ctx, N] on the device."""
        F = int(self.cfg.F)
        scores = torch.empty((n_ctx, N), dtype=torch.float32, device=self.device)
        ids = self._cached(('cand_ids', block), lambda: torch.empty((block, F), dtype=torch.int32, device=self.device))
        flat, st = scores.view(-1), self._stream()
        for s0 in range(0, n_ctx * N, block):
            m = min(block, n_ctx * N - s0)
            buf, _ = self.workspace(m)
            hip.check(expand(s0, m, _ptr(ids), st))
            hip.check(self.lib.cffm_predict(self._s, self._t, _ptr(self.theta), _ptr(ids), m, _ptr(buf), _ptr(flat[s0:s0 + m]), st))
        return scores

    def _cand_lists(self, ctx, cand, nf, who):
        """(ctx, cand, C, N, stride) of a candidate argument [N, nf] (one list, stride 0) or [C, N, nf] (a list per context)."""
        ctx = self._contexts(ctx)
        C = int(ctx.shape[0])
        if cand.dim() not in (2, 3) or int(cand.shape[-1]) != nf or (cand.dim() == 3 and int(cand.shape[0]) != C):
            raise ValueError('%s: candidates must be [N, %d] or [%d, N, %d]' % (who, nf, C, nf))
        N = int(cand.shape[-2])
        if N < 1:
            raise ValueError('%s: needs a candidate' % who)
        return ctx, self._ids(cand), C, N, (N * nf if cand.dim() == 3 else 0)

    def score_candidate_tuples(self, ctx, fields, cand, block=8192):
        """score_candidates for candidates that are tuples of ids: `fields` are nf distinct columns, cand int32 [N, nf] (one list
        for every context) or [C, N, nf] (a list per context) on the device, row (c, n) being context c with its ids at `fields`
        replaced together by candidate n -> fp32 [C, N] on the device.  Swept exactly as score_candidates is: one reused id buffer
        (cffm_expand_candidates_ex), cffm_predict into the piece's slice of the result, nothing synchronises."""
        block = int(block)
        fields = self._fields(fields, 'score_candidate_tuples', block)
        nf = len(fields)
        ctx, cand, nctx, N, stride = self._cand_lists(ctx, cand, nf, 'score_candidate_tuples')
        host_fields = (C.c_int32 * nf)(*fields)                  # read before the launch, like the shape
        expand = self.lib.cffm_expand_candidates_ex
        return self._piece_sweep(nctx, N, block, lambda s0, m, ids, st: expand(self._s, _ptr(ctx), nctx, C.addressof(host_fields), nf,
                                                                               _ptr(cand), stride, N, s0, m, ids, st))

    def sweep_ok(self):
        """True where score_candidates_shared serves this engine's shape (cffm_sweep_ok, include/cffm_hip.h)."""
        return bool(self.lib.cffm_sweep_ok(self._s))

    def score_candidates_shared(self, ctx, field, cand):
        """The scores of score_candidates with the fixed-field work done once per context (cffm_score_sweep, csrc/sweep.hip):
        same arguments, fp32 [C,N] on the device, equal to score_candidates to rounding (not bit for bit).  The per-context
        scratch is kept in self._ws; the ordinary workspace is not touched and nothing synchronises.  ValueError for a shape the
        sweep does not serve (sweep_ok())."""
        ctx, cand = self._contexts(ctx), self._ids(cand.reshape(-1))
        F, N = int(self.cfg.F), int(cand.numel())
        if N < 1 or not 0 <= int(field) < F:
            raise ValueError('score_candidates_shared: needs a candidate and 0 <= field < %d' % F)
        C = int(ctx.shape[0])
        if not self.sweep_ok():
            raise ValueError('score_candidates_shared: the shared sweep does not serve this shape (both branches, D = 32, F <= 10)')
        return self._sweep_launch('sweep', ctx, C, [int(field)], cand, 0, N)

    def _sweep_scratch(self, n_ctx, nf=1, key='sweep'):
        """The grow-only per-context scratch of the shared sweeps for nf swept fields (cffm_sweep_tuples_scratch_bytes; nf = 1 is
        cffm_sweep_scratch_bytes), kept in self._ws[key]."""
        scratch = self._ws.get(key)
        nbytes = int(self.lib.cffm_sweep_tuples_scratch_bytes(self._s, nf, n_ctx))
        if scratch is None or int(scratch.numel()) < nbytes:
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._ws[key] = scratch
        return scratch

    def _sweep_launch(self, key, ctx, nctx, fields, cand, stride, N):
        """The two launches of the three score_*_shared methods, every argument checked: cffm_score_sweep_tuples, the entry point
        cffm_score_sweep and cffm_score_sweep_lists forward to with one field -> fp32 [nctx, N] on the device."""
        scores = torch.empty((nctx, N), dtype=torch.float32, device=self.device)
        if nctx == 0:
            return scores
        nf = len(fields)
        host_fields = (C.c_int32 * nf)(*fields)                  # read before the launch, like the shape
        hip.check(self.lib.cffm_score_sweep_tuples(self._s, self._t, _ptr(self.theta), _ptr(ctx), nctx, C.addressof(host_fields), nf,
                                                   _ptr(cand), stride, N, _ptr(scores), N, _ptr(self._sweep_scratch(nctx, nf, key)),
                                                   self._stream()))
        return scores

    def score_candidate_lists_shared(self, ctx, field, cand):
        """score_candidates_shared with a candidate list per context: cand int32 [C, N] on the device, row c scored against its own
        list (cffm_score_sweep_lists) -> fp32 [C, N].  A (context, id) pair gives the bits score_candidates_shared gives it.
        ValueError for a shape the sweep does not serve (sweep_ok())."""
        F = int(self.cfg.F)
        if cand.dim() != 2:
            raise ValueError('score_candidate_lists_shared: candidates must be [C, N]')
        ctx, cand, nctx, N, _ = self._cand_lists(ctx, cand.unsqueeze(-1), 1, 'score_candidate_lists_shared')
        if not 0 <= int(field) < F:
            raise ValueError('score_candidate_lists_shared: needs 0 <= field < %d' % F)
        if not self.sweep_ok():
            raise ValueError('score_candidate_lists_shared: the shared sweep does not serve this shape (both branches, D = 32, F <= 10)')
        return self._sweep_launch('sweep', ctx, nctx, [int(field)], cand, N, N)

    def sweep_tuples_ok(self, nf):
        """True where score_candidate_tuples_shared serves this engine's shape for tuples of nf ids (cffm_sweep_tuples_ok)."""
        return bool(self.lib.cffm_sweep_tuples_ok(self._s, int(nf)))

    def score_candidate_tuples_shared(self, ctx, fields, cand):
        """The scores of score_candidate_tuples with everything that involves no swept field done once per context
        (cffm_score_sweep_tuples, csrc/sweep.hip): `fields` nf distinct columns in any order, cand int32 [N, nf] (one list for every
        context) or [C, N, nf] (a list per context) on the device -> fp32 [C, N] on the device, equal to score_candidate_tuples to
        rounding.  The per-context scratch is kept in self._ws under a key of its own, grow-only; nothing synchronises.
        ValueError where (shape, nf) is not served (sweep_tuples_ok(nf))."""
        fields = self._fields(fields, 'score_candidate_tuples_shared')
        nf = len(fields)
        ctx, cand, nctx, N, stride = self._cand_lists(ctx, cand, nf, 'score_candidate_tuples_shared')
        if not self.sweep_tuples_ok(nf):
            raise ValueError('score_candidate_tuples_shared: the tuple sweep does not serve this shape for tuples of %d '
                             '(both branches, D = 32, F <= 10, nf <= 4, the candidate kernel within a CU\'s LDS)' % nf)
        return self._sweep_launch('sweep_tuples', ctx, nctx, fields, cand, stride, N)

    def _rank_args(self, scores, skip):
        if scores.dim() != 2 or scores.dtype != torch.float32 or (scores.shape[1] > 1 and scores.stride(1) != 1):
            raise ValueError('scores must be fp32 [C, N] with contiguous rows')
        C, N = int(scores.shape[0]), int(scores.shape[1])
        row_stride = int(scores.stride(0)) if C > 1 else N
        skip_stride = 0
        if skip is not None:
            if tuple(skip.shape) != (C, N):
                raise ValueError('skip must be [C, N] like the scores')
            if skip.dtype == torch.bool:
                skip = skip.contiguous().view(torch.uint8)
            elif skip.dtype != torch.uint8 or not skip.is_contiguous():
                skip = (skip != 0).contiguous().view(torch.uint8)
            skip_stride = N
        return C, N, row_stride, skip, skip_stride

    def topk(self, scores, k, skip=None):
        """The k best candidates of every row of scores fp32 [C,N] (device) in the order of include/cffm_hip.h (score descending,
        -0 == +0, NaN last, ties by position): (idx int32 [C,k] candidate positions, -1 padded; val fp32 [C,k] their scores bit
        for bit, NaN padded; count int32 [C] = min(k, N - skipped)).  skip: optional [C,N] mask, non-zero = leave out."""
        C, N, row_stride, skip, skip_stride = self._rank_args(scores, skip)
        k = int(k)
        dev = self.device

        def make():
            nbytes = int(self.lib.cffm_topk_scratch_bytes(C, N, k))
            if nbytes < 0:
                raise ValueError('topk: needs N >= 1 and 1 <= k <= 1024 (N = %d, k = %d)' % (N, k))
            return torch.empty(nbytes, dtype=torch.uint8, device=dev)

        scratch = self._cached(('topk', C, N, k), make)
        idx = torch.empty((C, k), dtype=torch.int32, device=dev)
        val = torch.empty((C, k), dtype=torch.float32, device=dev)
        count = torch.empty((C,), dtype=torch.int32, device=dev)
        hip.check(self.lib.cffm_topk(_ptr(scores), row_stride, _ptr(skip), skip_stride, C, N, k, _ptr(scratch), _ptr(idx), _ptr(val),
                                     _ptr(count), self._stream()))
        return idx, val, count

    def rank_of(self, scores, target, skip=None):
        """0-based rank of candidate target[c] among the non-skipped candidates of row c, in the same order as topk: int32 [C] on
        the device (-1 for a target outside [0, N))."""
        C, N, row_stride, skip, skip_stride = self._rank_args(scores, skip)
        target = self._ids(target.reshape(-1))
        if int(target.numel()) != C:
            raise ValueError('rank_of: one target per row of the scores')
        rank = torch.empty((C,), dtype=torch.int32, device=self.device)
        hip.check(self.lib.cffm_rank_of(_ptr(scores), row_stride, _ptr(skip), skip_stride, C, N, _ptr(target), _ptr(rank),
                                        self._stream()))
        return rank

    def seen_mask(self, off, pos, row, N, skip=None):
        """cffm_seen_mask: the skip mask of topk / rank_of from a sparse seen relation on the device - off int32 [R + 1] and pos int32
        [nnz] the CSR of candidate positions (cffm_amd.spec.seen_index builds one), row int32 [C] the CSR row of every context
        (outside [0, R): nothing seen) - OR-ed with skip, an optional [C, N] mask (non-zero = leave out).  Returns uint8 [C, N] on
        the device, cffm_amd.spec.seen_mask bit for bit.  The buffer is kept per (C, N) and written again by the next call of that
        shape: hand it to topk / rank_of before then.  Nothing synchronises."""
        N = int(N)
        if off.dim() != 1 or pos.dim() != 1 or row.dim() != 1 or int(off.numel()) < 1 or N < 1:
            raise ValueError('seen_mask: needs off [R + 1], pos [nnz], row [C] and N >= 1')
        off, pos, row = self._ids(off), self._ids(pos), self._ids(row)
        C, R, nnz = int(row.numel()), int(off.numel()) - 1, int(pos.numel())
        skip_stride = 0
        if skip is not None:
            if tuple(skip.shape) != (C, N):
                raise ValueError('skip must be [C, N]: one row per entry of row')
            if skip.dtype == torch.bool:
                skip = skip.contiguous().view(torch.uint8)
            elif skip.dtype != torch.uint8 or not skip.is_contiguous():
                skip = (skip != 0).contiguous().view(torch.uint8)
            skip_stride = N
        mask = self._cached(('seen_mask', C, N), lambda: torch.empty((C, N), dtype=torch.uint8, device=self.device))
        if C:
            hip.check(self.lib.cffm_seen_mask(_ptr(off), _ptr(pos) if nnz else 0, R, nnz, _ptr(row), _ptr(skip), skip_stride, C, N,
                                              _ptr(mask), N, self._stream()))
        return mask

    def predictions(self, B):
        """The [B] outputs the last forward (forward / forward_staged / forward_packed) left in the workspace, as a tensor of
        their own."""
        return self.ws_tensor(B, 'out', (B,)).clone()

    def train_step(self, ids, y):
        """sess.run((self.loss, self.optimizer)) (CFFM.py:200).  Returns the loss as a device scalar
        (no host sync)."""
        ids, y = self._ids(ids), self._labels(y)
        B = ids.shape[0]
        if B == 0:                                   # nothing to learn from: parameters and slots stay as they are
            return self.loss_buf
        buf, _ = self.workspace(B)
        if self.cfg.optimizer != 'AdagradOptimizer':
            self.opt_step += 1
            hip.check(self.lib.cffm_train_step_opt(
                self._s, self._t, self._ta,
                self._ta2, _ptr(self.theta),
                _ptr(self.theta_acc), _ptr(self.theta_acc2), _ptr(self.grad), _ptr(ids), _ptr(y), B, _ptr(buf),
                _ptr(self.loss_buf), self.opt_step, self._stream()))
            return self.loss_buf
        hip.check(self.lib.cffm_train_step(self._s, self._t, self._ta,
                                           _ptr(self.theta), _ptr(self.theta_acc), _ptr(self.grad), _ptr(ids),
                                           _ptr(y), B, _ptr(buf), _ptr(self.loss_buf), self._stream()))
        return self.loss_buf

    # ---- halves of the step (multi-GPU path and tests) ---------------------------------------------
    def forward(self, ids, y=None):
        ids = self._ids(ids)
        B = ids.shape[0]
        buf, _ = self.workspace(B)
        hip.check(self.lib.cffm_forward(self._s, self._t, _ptr(self.theta), _ptr(ids),
                                        _ptr(y), B, _ptr(buf), self._stream()))

    def gather_inner_fwd_ok(self):
        """Wide shapes (F*(F-1)/2 > 64, K == D in {32, 64}, F <= 32): predict / train_step never materialise the rows."""
        return bool(self.lib.cffm_gather_inner_fwd_ok(self._s))

    def gather_inner_fwd(self, ids):
        """cffm_gather_inner_fwd alone: the three lookups fused with the inner branch, the s0 pool and the first-order
        inputs (ws.inner_out, ws.t1[:, :D], ws.fb, ws.sort_keys); the kernel the gather roofline is quoted on."""
        ids = self._ids(ids)
        B = ids.shape[0]
        buf, _ = self.workspace(B)
        hip.check(self.lib.cffm_gather_inner_fwd(self._s, self._t, _ptr(self.theta), _ptr(ids), B, _ptr(buf), self._stream()))

    def shard_plan(self, ids, world, M_global, counts=None):
        """Routing plan of a [B,F] id batch through tables of M_global rows sharded r -> (r % world, r // world), entirely on the
        device (cffm_shard_plan: pack, one radix sort, head flags, scan, scatter - no int64 temporaries, no torch.sort).
        Returns int32 tensors (local_ids [B,F], order, uniq, pos, send_rows [B*F]) and counts int64 [world] (``counts``: a buffer
        to write them into; the call overwrites all of it, whatever it held)."""
        ids = self._ids(ids)
        n = int(ids.numel())
        dev = self.device

        def make():
            nbytes = int(self.lib.cffm_shard_plan_scratch_bytes(n))
            if nbytes < 0:
                raise RuntimeError('cffm_shard_plan_scratch_bytes failed')
            return torch.empty(nbytes, dtype=torch.uint8, device=dev)

        scratch = self._cached(('plan', n), make)
        local_ids = torch.empty(ids.shape, dtype=torch.int32, device=dev)
        order, uniq, pos, send_rows = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
        if counts is None:
            counts = torch.empty(int(world), dtype=torch.int64, device=dev)
        assert counts.dtype == torch.int64 and counts.numel() == int(world) and counts.is_contiguous()
        hip.check(self.lib.cffm_shard_plan(_ptr(ids), n, int(world), int(M_global), _ptr(scratch), _ptr(local_ids), _ptr(order),
                                           _ptr(uniq), _ptr(pos), _ptr(send_rows), _ptr(counts), self._stream()))
        return local_ids, order, uniq, pos, send_rows, counts

    def gather_packed(self, local_rows):
        """Owner side of a row-sharded lookup: int32 [m] local rows -> [m, packed_width] packed records
        (inner | outer | bias, 0, 0, 0), ONE kernel (cffm_gather_packed)."""
        m = int(local_rows.numel())
        out = torch.empty((m, self.packed_width), dtype=torch.float32, device=self.device)
        if m:
            rows = self._ids(local_rows.reshape(-1))
            hip.check(self.lib.cffm_gather_packed(self._s, self._t, _ptr(rows), m, _ptr(out), self._stream()))
        return out

    def stage_packed(self, packed, pos, B):
        """Requester side: slot i of the batch takes record pos[i] of packed [n_records, packed_width] -> ws.Ei / ws.Eo / ws.fb."""
        buf, _ = self.workspace(B)
        pos = self._ids(pos.reshape(-1)) if pos is not None else None
        hip.check(self.lib.cffm_stage_packed(self._s, _ptr(packed), _ptr(pos), int(packed.shape[0]), int(B), _ptr(buf),
                                             self._stream()))

    def packed_ok(self):
        """True when the row-sharded step can consume the packed records where they lie (the wide shapes)."""
        return bool(self.lib.cffm_gather_inner_fwd_ok(self._s))

    def forward_packed(self, packed, pos, y, B):
        """Forward half of a row-sharded step straight from the received records [n_records, packed_width]: slot i reads record pos[i]
        in the kernel that fetches it; ws.Ei / ws.Eo are never written (cffm_forward_packed)."""
        buf, _ = self.workspace(B)
        pos = self._ids(pos.reshape(-1))
        hip.check(self.lib.cffm_forward_packed(self._s, _ptr(self.theta), _ptr(packed), _ptr(pos), int(packed.shape[0]), _ptr(y),
                                               int(B), _ptr(buf), self._stream()))

    def backward_unscaled_packed(self, packed, pos, y, B, B_global):
        """Backward half over the same records (dL/dout = (out - y) / B_global); the row gradients stay in the workspace for
        pack_rows_dedup.  Returns grad_full [n+4] with this rank's loss-term sum at index n."""
        buf, _ = self.workspace(B)
        pos = self._ids(pos.reshape(-1))
        hip.check(self.lib.cffm_backward_unscaled_packed(self._s, _ptr(self.theta), _ptr(packed), _ptr(pos), int(packed.shape[0]),
                                                         _ptr(y), int(B), int(B_global), _ptr(buf), _ptr(self._grad_full),
                                                         self._stream()))
        return self._grad_full

    def forward_staged(self, y, B):
        """cffm_forward over rows that are already staged in the workspace (tab = NULL)."""
        buf, _ = self.workspace(B)
        hip.check(self.lib.cffm_forward(self._s, 0, _ptr(self.theta), 0, _ptr(y), int(B), _ptr(buf), self._stream()))

    def forward_rows(self, Ei, Eo, fb, y, B=None):
        """Forward from rows that are already looked up, given as three tensors Ei [B,F,K], Eo [B,F,D], fb [B,F]."""
        F = self.cfg.F
        B = Ei.numel() // (F * self.cfg.K) if B is None else B
        self.workspace(B)
        self.ws_tensor(B, 'Ei', (B, F, self.cfg.K)).copy_(Ei.reshape(B, F, self.cfg.K))
        self.ws_tensor(B, 'Eo', (B, F, self.cfg.D)).copy_(Eo.reshape(B, F, self.cfg.D))
        self.ws_tensor(B, 'fb', (B, F)).copy_(fb.reshape(B, F))
        self.forward_staged(y, B)

    def pack_rows_dedup(self, local_ids, order, uniq, B):
        """Row-gradient message with the duplicates of an id summed first (cffm_pack_rows_dedup): returns [B*F, row_grad_width]
        of which the first #distinct records are valid."""
        buf, _ = self.workspace(B)
        out = self._cached(('dedup', B), lambda: self._row_records(B))
        hip.check(self.lib.cffm_pack_rows_dedup(self._s, _ptr(self._ids(local_ids.reshape(-1))), _ptr(order), _ptr(uniq), int(B),
                                                _ptr(buf), _ptr(out), self._stream()))
        return out

    def _row_records(self, B):
        """An uninitialised row-gradient message for a batch of B rows: [B*F, row_grad_width]."""
        return torch.empty((B * self.cfg.F, self.row_grad_width), dtype=torch.float32, device=self.device)

    def backward(self, y, B, B_global=None):
        buf, _ = self.workspace(B)
        hip.check(self.lib.cffm_backward(self._s, _ptr(self.theta), _ptr(y), int(B),
                                         int(B if B_global is None else B_global), _ptr(buf), _ptr(self.grad),
                                         self._stream()))

    # ---- training on ranked lists: backward from a given dL/dout, the list losses, the list step -------------
    def backward_dout(self, dout, B):
        """Backward from the caller's dL/dout (cffm_backward_dout): dout fp32 [B] on the device, used as given (no 1/B, no loss).
        The forward was forward(ids, y or None); the gradients are read as after backward(): export_grad(), row_grads(B)."""
        self._backward_dout('backward_dout', self.lib.cffm_backward_dout, dout, B)

    def _backward_dout(self, who, entry, dout, B):
        """backward_dout and backward_dout_fused (who) around their entry points."""
        B = int(B)
        dout = dout.reshape(-1)
        if dout.dtype != torch.float32 or not dout.is_contiguous():
            dout = dout.to(torch.float32).contiguous()
        if int(dout.numel()) != B:
            raise ValueError('%s: dout must hold one value per example (%d, not %d)' % (who, B, int(dout.numel())))
        buf, _ = self.workspace(B)
        hip.check(entry(self._s, _ptr(self.theta), _ptr(dout), B, _ptr(buf), _ptr(self.grad), self._stream()))

    @staticmethod
    def _list_kind(kind):
        if kind not in hip.LIST_LOSS_IDS:
            raise ValueError("list loss must be one of %s, not %r" % (sorted(hip.LIST_LOSS_IDS), kind))
        return hip.LIST_LOSS_IDS[kind]

    def _logq_args(self, who, kind, lists, corr, G, Lg):
        """The operands of the logQ-corrected softmax, checked: lists int32 [G, Lg] and corr fp32 [U, 2] go together (a ValueError
        names the missing one), kind 'bpr' with them is refused by name -> (lists, corr, U), or None where both are None."""
        if lists is None and corr is None:
            return None
        if lists is None or corr is None:
            raise ValueError('%s: lists and corr go together: %s is missing' % (who, 'lists' if lists is None else 'corr'))
        if kind == 'bpr':
            raise ValueError("%s: the logQ correction (lists, corr) is that of the sampled softmax; kind 'bpr' has none" % who)
        if tuple(lists.shape) != (G, Lg):
            raise ValueError('%s: lists must be int32 [G = %d, Lg = %d], not %s' % (who, G, Lg, tuple(lists.shape)))
        if corr.dim() != 2 or int(corr.shape[1]) != 2 or int(corr.shape[0]) < 1 or corr.dtype != torch.float32 or \
                not corr.is_contiguous() or corr.device != lists.device:
            raise ValueError('%s: corr must be a contiguous fp32 [U, 2] on the device (cffm_amd.spec.logq_table)' % who)
        return self._ids(lists), corr, int(corr.shape[0])

    def list_loss(self, scores, target, G, Lg, kind, lists=None, corr=None):
        """cffm_list_loss over scores fp32 [G * Lg] (list g = rows g * Lg ..) with target int32 [G] the positives' positions, kind
        'bpr' or 'softmax': (loss [1], dout [G * Lg], terms [G]) on the device, dout = d loss / d scores.  Nothing synchronises.
        With lists int32 [G, Lg] (the candidates' indices into U distinct tuples) and corr fp32 [U, 2] (cffm_amd.spec.logq_table) the
        softmax is logQ-corrected (cffm_list_loss_logq; cffm_amd.spec.list_loss_logq is its float64 twin); 'bpr' is then refused."""
        kind_id, G, Lg = self._list_kind(kind), int(G), int(Lg)
        logq = self._logq_args('list_loss', kind, lists, corr, G, Lg)
        kind = kind_id
        scores, target = scores.reshape(-1), self._ids(target.reshape(-1))
        if scores.dtype != torch.float32 or not scores.is_contiguous():
            scores = scores.to(torch.float32).contiguous()
        if int(scores.numel()) != G * Lg or int(target.numel()) != G:
            raise ValueError('list_loss: scores must hold G * Lg = %d values and target G = %d' % (G * Lg, G))
        dev = self.device
        dout = torch.empty(G * Lg, dtype=torch.float32, device=dev)
        terms = torch.empty(G, dtype=torch.float32, device=dev)
        loss = torch.zeros(1, dtype=torch.float32, device=dev)
        if logq is None:
            hip.check(self.lib.cffm_list_loss(kind, _ptr(scores), G, Lg, _ptr(target), _ptr(dout), _ptr(terms), _ptr(loss),
                                              _ptr(self._list_scratch(G)), self._stream()))
        else:
            lists, corr, U = logq
            hip.check(self.lib.cffm_list_loss_logq(kind, _ptr(scores), G, Lg, _ptr(target), _ptr(lists), _ptr(corr), U, _ptr(dout),
                                                   _ptr(terms), _ptr(loss), _ptr(self._list_scratch(G)), self._stream()))
        return loss, dout, terms

    def _list_scratch(self, G):
        nbytes = int(self.lib.cffm_list_loss_scratch_bytes(int(G)))
        scratch = self._ws.get('list_loss')
        if scratch is None or int(scratch.numel()) < nbytes:
            scratch = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=self.device)
            self._ws['list_loss'] = scratch
        return scratch

    def _list_step_args(self, who, ctx, fields, cand, target, kind):
        """What train_step_lists and train_step_lists_fused (who) open with: the optimizer, the loss, the kind, the fields and the
        shapes checked -> (kind id, the fields as a host int32 array, nf, ctx, cand, target, G, Lg, stride).  Touches nothing."""
        if self.cfg.optimizer != 'AdagradOptimizer':
            raise ValueError('%s: the list step implements AdagradOptimizer, not %s' % (who, self.cfg.optimizer))
        if self.cfg.loss_type == 'log_loss':
            raise ValueError("%s: loss_type 'log_loss' leaves sigmoid(out) in the forward, not the score the list losses rank" % who)
        kind_id = self._list_kind(kind)
        fields = self._fields(fields, who)
        nf = len(fields)
        if cand.dim() != 3:
            raise ValueError('%s: candidates must be [G, Lg, %d]' % (who, nf))
        ctx, cand, G, Lg, stride = self._cand_lists(ctx, cand, nf, who)
        target = self._ids(target.reshape(-1))
        if Lg < 2 or int(target.numel()) != G:
            raise ValueError('%s: needs lists of at least 2 candidates and one target per list' % who)
        host_fields = (C.c_int32 * nf)(*fields)                  # read before the launch, like the shape
        return kind_id, host_fields, nf, ctx, cand, target, G, Lg, stride

    def _list_step_bufs(self, G, Lg):
        """The buffers a list step of G lists of Lg keeps: (ids int32 [B, F] under ('list_ids', B); dout fp32 [B] and terms fp32 [G]
        under ('list_out', G, Lg))."""
        B, F, dev = G * Lg, int(self.cfg.F), self.device
        ids = self._cached(('list_ids', B), lambda: torch.empty((B, F), dtype=torch.int32, device=dev))
        dout, terms = self._cached(('list_out', G, Lg), lambda: (torch.empty(B, dtype=torch.float32, device=dev),
                                                                  torch.empty(G, dtype=torch.float32, device=dev)))
        return ids, dout, terms

    def train_step_lists(self, ctx, fields, cand, target, kind, lists=None, corr=None):
        """One Adagrad step on G ranked lists: ctx int32 [G, F] the contexts, cand int32 [G, Lg, nf] every list's candidate tuples
        for the columns `fields`, target int32 [G] the position of each list's positive, kind 'bpr' or 'softmax'.  The id rows
        (cffm_expand_candidates_ex), the forward without labels, the list loss on ws.out, the backward from its dL/dout
        (cffm_backward_dout: the stage launches), then the dense and the sparse Adagrad update.  Returns the loss as a device
        scalar (no host sync).  Adagrad only, and not loss_type='log_loss', whose forward leaves sigmoid(out) and not the score.
        lists int32 [G, Lg] with corr fp32 [U, 2], together: the loss is the logQ-corrected softmax of list_loss (cffm_list_loss_logq
        where cffm_list_loss stands above), every other launch as it is; kind 'bpr' with them is a ValueError before any launch."""
        kind_id, host_fields, nf, ctx, cand, target, G, Lg, stride = self._list_step_args('train_step_lists', ctx, fields, cand, target, kind)
        logq = self._logq_args('train_step_lists', kind, lists, corr, G, Lg)
        B = G * Lg
        if B == 0:
            return self.loss_buf
        ids, dout, terms = self._list_step_bufs(G, Lg)
        hip.check(self.lib.cffm_expand_candidates_ex(self._s, _ptr(ctx), G, C.addressof(host_fields), nf, _ptr(cand), stride, Lg,
                                                     0, B, _ptr(ids), self._stream()))
        self.forward(ids, None)
        buf, wl = self.workspace(B)
        if logq is None:
            hip.check(self.lib.cffm_list_loss(kind_id, _ptr(buf) + int(wl.out), G, Lg, _ptr(target), _ptr(dout), _ptr(terms),
                                              _ptr(self.loss_buf), _ptr(self._list_scratch(G)), self._stream()))
        else:
            lists, corr, U = logq
            hip.check(self.lib.cffm_list_loss_logq(kind_id, _ptr(buf) + int(wl.out), G, Lg, _ptr(target), _ptr(lists), _ptr(corr), U,
                                                   _ptr(dout), _ptr(terms), _ptr(self.loss_buf), _ptr(self._list_scratch(G)),
                                                   self._stream()))
        self.backward_dout(dout, B)
        self.apply_dense()
        dEi, dEo, dfb = self.row_grads(B)
        self.apply_sparse(ids, dEi, dEo, dfb, B)
        return self.loss_buf

    def draw_lists(self, seed, list0, at, U, m, cand=None):
        """cffm_draw_lists: G = len(at) ranked lists over U distinct tuples, list g (id list0 + g) a function of (seed, id) alone -
        the positive at[g] (int32 [G] on the device), m distinct others, the positive at a drawn place; cffm_amd.spec.draw_lists
        is the specification.  cand: int32 [U, nf] on the device, or None for the indices alone.  Returns (tuples int32
        [G, m + 1, nf] = cand[lists] or None, lists int32 [G, m + 1], target int32 [G]) on the device.  Nothing synchronises."""
        return self._draw('draw_lists', self.lib.cffm_draw_lists, seed, list0, at, U, m, cand)

    def _draw(self, who, entry, seed, list0, at, U, m, cand, cdf=None):
        """draw_lists and draw_lists_weighted (who) around their entry points; the weighted one takes the cdf words after m.  m within
        [1, min(U - 1, 1023)] leaves no U below 2 through."""
        seed, list0, U, m = int(seed) & 0xffffffffffffffff, int(list0), int(U), int(m)
        at = self._ids(at.reshape(-1))
        G, nf = int(at.numel()), 0
        if cand is not None:
            if cand.dim() != 2 or int(cand.shape[0]) != U or int(cand.shape[1]) < 1:
                raise ValueError('%s: cand must be [U = %d, nf >= 1]' % (who, U))
            cand, nf = self._ids(cand), int(cand.shape[1])
        if not 1 <= m <= min(U - 1, 1023):
            raise ValueError('%s: needs 1 <= m <= min(U - 1, 1023) (U = %d, m = %d)' % (who, U, m))
        dev = self.device
        lists = torch.empty((G, m + 1), dtype=torch.int32, device=dev)
        target = torch.empty(G, dtype=torch.int32, device=dev)
        tuples = None if cand is None else torch.empty((G, m + 1, nf), dtype=torch.int32, device=dev)
        if G:
            weights = () if cdf is None else (_ptr(cdf),)
            hip.check(entry(seed, list0, G, _ptr(at), U, m, *weights, _ptr(cand), nf, _ptr(lists), _ptr(tuples), _ptr(target),
                            self._stream()))
        return tuples, lists, target

    def draw_lists_weighted(self, seed, list0, at, cdf, m, cand=None):
        """cffm_draw_lists_weighted: draw_lists with the m negatives drawn in proportion to weights, by rejection - successive
        sampling without replacement over the set without at[g]; cffm_amd.spec.draw_lists_weighted is the specification.  cdf: int32
        or uint32 [U] on the device, the words of cffm_amd.spec.weight_cdf (reinterpreted, not converted); U = len(cdf).  cand:
        int32 [U, nf] on the device, or None for the indices alone.  Returns (tuples int32 [G, m + 1, nf] = cand[lists] or None,
        lists int32 [G, m + 1], target int32 [G]) on the device; a list that did not collect m negatives within the word cap (too
        skewed weights) and one whose at[g] is outside [0, U) come back as -1 / zeros / target -1.  Nothing synchronises."""
        if cdf.dim() != 1 or cdf.dtype not in (torch.int32, torch.uint32) or cdf.device != at.device:
            raise ValueError('draw_lists_weighted: cdf must be an int32 / uint32 vector on the device (spec.weight_cdf)')
        return self._draw('draw_lists_weighted', self.lib.cffm_draw_lists_weighted, seed, list0, at, cdf.numel(), m, cand, cdf.contiguous())

    def pick_hard(self, seed, list0, scores, target_pool, m, lists=None, tuples=None):
        """cffm_pick_hard, the select step of dynamic negative sampling: from the scored pool of each of G lists (id list0 + g) the m
        best-scored negatives, hardest first, in the order of topk (score descending, -0 == +0, NaN last, ties by position), around
        the positive at a place drawn from (seed, id, m); cffm_amd.spec.pick_hard is the specification.  scores: fp32 [G, Lp] on the
        device, the last dimension contiguous, the row stride passed through (elements beyond Lp are never read); target_pool: int32
        [G], the pool position of each list's positive (the target of the draw that made the pool); lists: int32 [G, Lp] pool
        indices and / or tuples: int32 [G, Lp, nf] pool tuples, one of them at least.  Returns (tuples int32 [G, m + 1, nf] or None,
        lists int32 [G, m + 1] or None, target int32 [G]) on the device; a list whose target_pool lies outside [0, Lp) comes back as
        zeros / -1 / target -1.  Nothing synchronises."""
        who = 'pick_hard'
        seed, list0, m = int(seed) & 0xffffffffffffffff, int(list0), int(m)
        if scores.dim() != 2 or scores.dtype != torch.float32 or (scores.shape[1] > 1 and scores.stride(1) != 1):
            raise ValueError('%s: scores must be fp32 [G, Lp] with contiguous rows' % who)
        G, Lp = int(scores.shape[0]), int(scores.shape[1])
        row_stride = int(scores.stride(0)) if G > 1 else Lp
        if row_stride < Lp:
            raise ValueError('%s: the rows of scores overlap (row stride %d < Lp = %d)' % (who, row_stride, Lp))
        if not 2 <= Lp <= 1024 or not 1 <= m <= Lp - 1:
            raise ValueError('%s: needs 2 <= Lp <= 1024 and 1 <= m <= Lp - 1 (Lp = %d, m = %d)' % (who, Lp, m))
        target_pool = self._ids(target_pool.reshape(-1))
        if int(target_pool.numel()) != G:
            raise ValueError('%s: one target_pool per row of the scores (%d, not %d)' % (who, G, int(target_pool.numel())))
        if lists is None and tuples is None:
            raise ValueError('%s: needs the pool as lists [G, Lp], as tuples [G, Lp, nf], or both' % who)
        nf = 0
        if lists is not None:
            if tuple(lists.shape) != (G, Lp):
                raise ValueError('%s: lists must be [G = %d, Lp = %d]' % (who, G, Lp))
            lists = self._ids(lists)
        if tuples is not None:
            if tuples.dim() != 3 or tuple(tuples.shape[:2]) != (G, Lp) or int(tuples.shape[2]) < 1:
                raise ValueError('%s: tuples must be [G = %d, Lp = %d, nf >= 1]' % (who, G, Lp))
            tuples, nf = self._ids(tuples), int(tuples.shape[2])
        dev = self.device
        lists_out = None if lists is None else torch.empty((G, m + 1), dtype=torch.int32, device=dev)
        tuples_out = None if tuples is None else torch.empty((G, m + 1, nf), dtype=torch.int32, device=dev)
        target = torch.empty(G, dtype=torch.int32, device=dev)
        if G:
            hip.check(self.lib.cffm_pick_hard(seed, list0, G, _ptr(scores), row_stride, Lp, _ptr(target_pool), m, _ptr(lists), _ptr(tuples),
                                              nf, _ptr(lists_out), _ptr(tuples_out), _ptr(target), self._stream()))
        return tuples_out, lists_out, target

    def list_step_ok(self, B):
        """True where train_step_lists_fused serves B = G * Lg rows of this engine's shape (cffm_list_step_ok; host only)."""
        return bool(self.lib.cffm_list_step_ok(self._s, int(B)))

    def backward_dout_fused(self, dout, B):
        """backward_dout on the launches backward() takes where its fused top runs (cffm_backward_dout_fused); raises where it does not."""
        self._backward_dout('backward_dout_fused', self.lib.cffm_backward_dout_fused, dout, B)

    def train_step_lists_fused(self, ctx, fields, cand, target, kind, lists=None, corr=None):
        """train_step_lists through the fused top of the backward (cffm_train_step_lists, one library call): the id rows, the forward
        without labels, the list loss on ws.out, the backward from its dL/dout with the fused top placing the update's sort keys, and
        update_all.  Where the single-launch forward runs (cffm_fwd_all_ok: the frappe shape among them) these are the launches of
        train_step plus three, seven at the frappe shape; at D = 8 or 16, and at F = 11 with D = 32, the forward is the stage launches,
        a combination train_step itself does not run (it sorts and applies the rows separately there).  Same arguments,
        checks, return value and buffers (('list_ids', B), ('list_out', G, Lg), loss_buf) as train_step_lists.  Served where
        list_step_ok(G * Lg); elsewhere a ValueError names the shape and B, and nothing has been touched.  lists and corr as in
        train_step_lists: the same launches with the logQ-corrected softmax as the loss (cffm_train_step_lists_logq)."""
        who = 'train_step_lists_fused'
        kind_id, host_fields, nf, ctx, cand, target, G, Lg, stride = self._list_step_args(who, ctx, fields, cand, target, kind)
        logq = self._logq_args(who, kind, lists, corr, G, Lg)
        B = G * Lg
        if B == 0:
            return self.loss_buf
        if not self.list_step_ok(B):
            raise ValueError('%s: the fused list step does not serve F=%d K=%d D=%d %s, lamda_bilinear=%g at B = %d x %d = %d rows '
                             '(list_step_ok); train_step_lists does' % (who, int(self.cfg.F), self.cfg.K, self.cfg.D, self.cfg.activation,
                                                                       self.cfg.lamda_bilinear, G, Lg, B))
        ids, dout, terms = self._list_step_bufs(G, Lg)
        buf, _ = self.workspace(B)
        args = (self._s, self._t, self._ta, _ptr(self.theta), _ptr(self.theta_acc), _ptr(self.grad), _ptr(ctx), G,
                C.addressof(host_fields), nf, _ptr(cand), stride, Lg, _ptr(target), kind_id, _ptr(ids), _ptr(dout), _ptr(terms), _ptr(buf),
                _ptr(self.loss_buf), _ptr(self._list_scratch(G)))
        if logq is None:
            hip.check(self.lib.cffm_train_step_lists(*args, self._stream()))
        else:
            lists, corr, U = logq
            hip.check(self.lib.cffm_train_step_lists_logq(*args, _ptr(lists), _ptr(corr), U, self._stream()))
        return self.loss_buf

    # ---- data-parallel halves with late loss normalisation (cffm_amd/dist.py) ----------------------------------
    def backward_unscaled(self, ids, y, B, B_global, pack=True):
        """Backward with dL/dout = (out - y) / B_global.  Returns (grad_full [n+4] with this rank's loss-term sum at
        index n, rows [B*F, row_grad_width] = (id bits | dEi | dEo | dfb)) - the operands of ONE all-reduce and ONE
        all-gather.  pack=False leaves the row gradients in the workspace (rows is None): the row-sharded step packs
        them itself with the duplicates summed (pack_rows_dedup)."""
        ids = self._ids(ids)
        buf, _ = self.workspace(B)
        rows = self._cached(('rows', B), lambda: self._row_records(B)) if pack else None
        hip.check(self.lib.cffm_backward_unscaled(self._s, _ptr(self.theta), _ptr(ids), _ptr(y), int(B),
                                                  int(B_global), _ptr(buf), _ptr(self._grad_full), _ptr(rows),
                                                  self._stream()))
        return self._grad_full, rows

    def dp_local(self, ids, y, B, B_global):
        """forward + backward_unscaled in one library call (the local half of a data-parallel step).  Returns
        (grad_full, block): block is ONE flat buffer [B*F*row_grad_width packed rows | B*F sorted 64-bit keys], the unit
        DataParallelStep all-gathers; cffm_dp_apply merges the per-rank sorted runs instead of sorting again."""
        ids = self._ids(ids)
        buf, _ = self.workspace(B)
        block = self._cached(('block', B), lambda: torch.empty(B * self.cfg.F * (self.row_grad_width + 2), dtype=torch.float32,
                                                               device=self.device))
        hip.check(self.lib.cffm_dp_local(self._s, self._t, _ptr(self.theta), _ptr(ids), _ptr(y), int(B),
                                         int(B_global), _ptr(buf), _ptr(self._grad_full), _ptr(block), self._stream()))
        return self._grad_full, block

    def dp_apply(self, grad_full, rows_all, B_global, n_runs=0):
        """n_runs = 0: rows_all [n_rows, row_grad_width] in any order (cffm_backward_unscaled rows).  n_runs > 0: the flat
        concatenation of n_runs dp_local blocks."""
        W = self.row_grad_width
        # sorted runs: only where the single-launch forward left them, and while all ids fit the merge kernel's LDS
        runs_ok = n_runs > 0 and rows_all.dim() == 1 and (rows_all.numel() // (W + 2)) * 4 <= 150 * 1024 and \
            bool(self.lib.cffm_dp_runs_ok(self._s, int(rows_all.numel() // (W + 2) // n_runs // self.cfg.F)))
        if n_runs > 0 and not runs_ok:
            # the blocks carry no sorted runs (shape outside the single-launch forward): strip the key areas
            m = rows_all.numel() // (W + 2) // n_runs
            rows_all = rows_all.reshape(n_runs, m * (W + 2))[:, :m * W].reshape(n_runs * m, W).contiguous()
            n_runs = 0
        n_rows = rows_all.numel() // (W + 2) if n_runs > 0 else rows_all.shape[0]
        B_ws = max(1, -(-n_rows // self.cfg.F))       # an owner that received no rows still applies the dense update
        buf, _ = self.workspace(B_ws)
        # SGD / Momentum: the same arguments, theta_acc / tables_acc read as the first slot (they start at 0 for these optimizers)
        apply = self.lib.cffm_dp_apply if self.cfg.optimizer == 'AdagradOptimizer' else self.lib.cffm_dp_apply_opt
        hip.check(apply(self._s, self._t, self._ta,
                        _ptr(self.theta), _ptr(self.theta_acc), _ptr(grad_full), int(B_global),
                        _ptr(rows_all), int(n_rows), _ptr(buf), int(B_ws), _ptr(self.loss_buf),
                        int(n_runs), self._stream()))
        return self.loss_buf

    # ---- dense-table exchange (small vocabularies): ONE all-reduce per step ----------------------------------------
    def dp_dense_ok(self, B, world):
        """The dense image of the tables is at most twice what the ranks' row gradients add up to (it also saves the second
        collective and the merge + segment walk of the gathered rows: measured 133 vs 152 us per step at world size 1,
        frappe), and the single-launch forward (which leaves the sorted keys the scatter needs) covers this shape.  Adagrad only:
        an exact 0 in the all-reduced image cannot tell "row not looked up" from "gradients summed to 0", and Momentum must decay
        the accumulator in the second case and not in the first; SGD and Momentum always take the all-gather route."""
        W = self.cfg.K + self.cfg.D + 1
        return bool(self.lib.cffm_dp_runs_ok(self._s, int(B))) and \
            self.cfg.M * W <= 2 * world * B * self.cfg.F * (W + 3) and self.cfg.optimizer == 'AdagradOptimizer'

    def dp_local_dense(self, ids, y, B, B_global):
        ids = self._ids(ids)
        buf, _ = self.workspace(B)
        flat = self._cached('flat', lambda: torch.zeros(int(self.lib.cffm_dp_dense_floats(self._s)), dtype=torch.float32,
                                                        device=self.device))
        if self._flat_dirty:
            flat.zero_()                     # a step was abandoned between the two halves: the image contract is zero on entry
        self._flat_dirty = True
        hip.check(self.lib.cffm_dp_local_dense(self._s, self._t, _ptr(self.theta), _ptr(ids), _ptr(y),
                                               int(B), int(B_global), _ptr(buf), _ptr(flat), self._stream()))
        return flat

    def dp_apply_dense(self, flat_sum, B_global):
        hip.check(self.lib.cffm_dp_apply_dense(self._s, self._t, self._ta,
                                               _ptr(self.theta), _ptr(self.theta_acc), _ptr(flat_sum), int(B_global),
                                               _ptr(self.loss_buf), self._stream()))
        own = self._ws.get('flat')
        if own is not None and flat_sum.data_ptr() == own.data_ptr():
            self._flat_dirty = False         # cffm_dp_apply_dense cleared the image it consumed (zero on exit)
        return self.loss_buf

    def apply_dense(self):
        hip.check(self.lib.cffm_dense_adagrad(_ptr(self.theta), _ptr(self.theta_acc), _ptr(self.grad),
                                              int(self.tl.n), float(self.cfg.lr), self._stream()))

    def apply_sparse(self, ids, dEi, dEo, dfb, B_ws):
        ids = self._ids(ids.reshape(-1))
        buf, _ = self.workspace(B_ws)
        hip.check(self.lib.cffm_sparse_adagrad(self._s, self._t, self._ta,
                                               _ptr(ids), int(ids.numel()), _ptr(dEi), _ptr(dEo), _ptr(dfb),
                                               _ptr(buf), int(B_ws), self._stream()))

    # ---- views the data-parallel step needs (cffm_amd/dist.py) ----------------------------------------
    def row_grads(self, B):
        F = self.cfg.F
        dEi = self.ws_tensor(B, 'dEi', (B, F, self.cfg.K)) if self.cfg.inner_conv else None
        dEo = self.ws_tensor(B, 'dEo', (B, F, self.cfg.D)) if self.cfg.outer_conv else None
        return dEi, dEo, self.ws_tensor(B, 'dfb', (B, F))

    def gather(self, ids, want_inner=True, want_outer=True, want_bias=True):
        ids = self._ids(ids)
        B, F = ids.shape
        dev = self.device
        Ei = torch.empty((B, F, self.cfg.K), dtype=torch.float32, device=dev) if want_inner else None
        Eo = torch.empty((B, F, self.cfg.D), dtype=torch.float32, device=dev) if want_outer else None
        fb = torch.empty((B, F), dtype=torch.float32, device=dev) if want_bias else None
        hip.check(self.lib.cffm_gather(self._s, self._t, _ptr(ids), B, _ptr(Ei), _ptr(Eo),
                                       _ptr(fb), self._stream()))
        return Ei, Eo, fb
