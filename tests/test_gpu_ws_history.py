"""Every composite call gives the same bits whatever its workspace held on entry.

The composites run in one grow-only buffer that comes from torch.empty and is laid out anew for every B (tests/_ws_history.py);
the backward sums its gradients from gpart slabs that nothing clears (api.hip clears them only for a disabled branch), the head
sums pool partials, the input gradients read relu bits, the update walks sorted keys.  Correctness rests on each kernel writing
all of what a later one reads: workgroups without an example, the partial last slab of a layer, the quarters of the slab
reduction that hold fewer slabs.  A fresh process hands out zeroed memory and a second engine of the same shape inherits the
first one's correct intermediates, so neither the fp64 parity tests nor the run-twice tests can see a slab nobody wrote.

Here a SEQUENCE - the unit that is entered dirty; its later calls read what its earlier ones wrote - runs once per history of
_ws_history.HISTORIES on engines built from the same parameters, in the order zeros, leftover, nan, huge, and everything it
returns or updates is compared with the zeros run by np.testing.assert_array_equal: the project's reduction orders are fixed, so
there is no tolerance to choose.  The nan run of every Adagrad train-step case then also goes through test_gpu_parity.step_check,
which ties the dirty result to the fp64 oracle and not only to another device run.

The sequence "backward_unscaled(pack=False) then pack_rows_dedup" starts at the forward whose intermediates that backward reads:
dirtying the buffer between the two would destroy its input.

CFFM_WS_HISTORY_REPORT=<file>: one line per (case, history) is appended there (profiles/ws_history.md was made from it).
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cffm_amd import hip  # noqa: E402
from tests import _ws_history as H  # noqa: E402
from tests import test_gpu_branches as br  # noqa: E402
from tests import test_gpu_parity as par  # noqa: E402

pytestmark = pytest.mark.gpu

THETA_LIKE = ('theta', 'theta_acc', 'theta_acc2', 'grad', 'grad_full', 'flat')


def report(label, history, what):
    path = os.environ.get('CFFM_WS_HISTORY_REPORT')
    if path:
        with open(path, 'a') as fh:
            fh.write('%s | %s | %s\n' % (label, history, what))


def make(name, c=None, **kw):
    """par.make_case for a case of its CASES, or for the dict c (listed under `name` only for the length of the call)."""
    if c is None:
        return par.make_case(name, **kw)
    par.CASES[name] = c
    try:
        return par.make_case(name, **kw)
    finally:
        del par.CASES[name]


def other_batch(cfg, B, seed=1234):
    """Other ids and labels, for the leftover run."""
    rng = np.random.default_rng(seed + B)
    X = rng.integers(0, cfg.M, size=(B, cfg.F)).astype(np.int32)
    y = rng.choice([0.0, 1.0] if cfg.loss_type in ('log_loss', 'hybrid') else [-1.0, 1.0], size=(B,)).astype(np.float32)
    return torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()


def host(t):
    return t.detach().cpu().numpy().copy()


def state_of(eng):
    """Everything a step updates: the loss, theta / slots / gradient as they lie, and the exports by variable name."""
    out = {'loss': host(eng.loss_buf), 'theta': host(eng.theta), 'theta_acc': host(eng.theta_acc), 'grad': host(eng.grad)}
    if eng.theta_acc2 is not None:
        out['theta_acc2'] = host(eng.theta_acc2)
    exports = [('param', eng.export_params()), ('acc', eng.export_accumulators()), ('grad', eng.export_grad())]
    if eng.export_second_moments() is not None:
        exports.append(('second moment', eng.export_second_moments()))
    for prefix, d in exports:
        for k, v in d.items():
            out['%s %s' % (prefix, k)] = np.asarray(v)
    return out


def run_histories(label, cfg, p32, B, B_other, sequence, histories=H.HISTORIES, batches=()):
    """sequence(eng, history) -> {tensor name: array} once per history, each on an engine of its own; the first mismatch with the
    zeros run ends the case.  batches: further batch sizes the sequence lays the buffer out at (it must not grow inside it)."""
    from cffm_amd.engine import HipEngine
    ids2, y2 = other_batch(cfg, B_other)
    ref = None
    for h in histories:
        eng = HipEngine(cfg, params=p32)
        H.pool_buffer(eng, B, *batches)
        H.enter(h, eng, p32, B, B_other, lambda e: e.train_step(ids2, y2))
        ptr = eng._pool.buf.data_ptr()
        if h == 'nan':                 # the fill reached the first member and, where the buffer is longer than the layout, its last byte
            buf, wl = eng.workspace(B)
            assert bool(torch.isnan(eng.ws_tensor(B, 'gpart', (4,))).all()) and bool(torch.isnan(eng.ws_tensor(B, 'dout', (1,))).all())
            assert buf.numel() == int(wl.bytes) or int(buf[-1]) == 0xFF
        got = sequence(eng, h)
        torch.cuda.synchronize()
        assert eng._pool.buf.data_ptr() == ptr, '%s: the sequence re-allocated the workspace it was to find dirty' % label
        if ref is None:
            ref = got
            assert h == 'zeros'
        else:
            assert list(got) == list(ref)
            for k in ref:
                H.assert_same(h, '%s: %s' % (label, k), got[k], ref[k], eng.tl if k in THETA_LIKE else None)
        report(label, h, 'passed')
        del eng
    return ref


# ---- train steps -----------------------------------------------------------------------------------------------------------------
TRAIN = [(n, None, H.leftover_batch(par.CASES[n]['B'])) for n in H.TRAIN_CASES] + \
        [(H.pair_name(Bo, B), H.pair_case(B), Bo) for Bo, B in H.FRAPPE_PAIRS]


def train_sequence(X, y):
    ids, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()

    def seq(eng, history):
        eng.train_step(ids, yt)
        return state_of(eng)
    return seq


@pytest.mark.parametrize('name,c,B_other', TRAIN, ids=[t[0] for t in TRAIN])
def test_train_step(name, c, B_other):
    """cffm_train_step (Adagrad) at the smallest shape of every route, entered on each history; then the nan history once more,
    through the fp64 step check of the parity tests."""
    from cffm_amd.engine import HipEngine
    cfg, p32, X, y = make(name, c)
    B = X.shape[0]
    ref = run_histories(name, cfg, p32, B, B_other, train_sequence(X, y))
    assert not np.array_equal(ref['theta'], HipEngine(cfg, params=p32).theta.cpu().numpy()), 'the step did not move theta'
    eng = HipEngine(cfg, params=p32)
    ids2, y2 = other_batch(cfg, B_other)
    H.enter('nan', eng, p32, B, B_other, lambda e: e.train_step(ids2, y2))
    par.step_check(cfg, eng, p32, None, X, y, name)
    report(name, 'nan + step_check', 'passed')


@pytest.mark.parametrize('name,c,B_other', TRAIN, ids=[t[0] for t in TRAIN])
def test_predict(name, c, B_other):
    cfg, p32, X, y = make(name, c)
    ids = torch.from_numpy(X).cuda()
    ref = run_histories(name + ' predict', cfg, p32, X.shape[0], B_other, lambda eng, h: {'predictions': host(eng.predict(ids))})
    assert np.isfinite(ref['predictions']).all()


@pytest.mark.parametrize('opt', H.OPTIMIZERS)
@pytest.mark.parametrize('name', H.OPT_CASES)
def test_train_step_other_optimizers(name, opt):
    """cffm_train_step_opt; with Adam the dense images Gi | Go | Gfb are members of the workspace."""
    cfg, p32, X, y = make(name)
    cfg.optimizer, cfg.lr = opt, (0.01 if opt == 'AdamOptimizer' else 1e-4)          # as test_gpu_parity.test_other_optimizers
    B = X.shape[0]
    ref = run_histories('%s %s' % (name, opt), cfg, p32, B, H.leftover_batch(B), train_sequence(X, y))
    assert ('theta_acc2' in ref) == (opt == 'AdamOptimizer') and np.isfinite(ref['loss']).all()


@pytest.mark.parametrize('loss', H.LOSSES)
def test_train_step_other_losses(loss):
    """square_l2 (dense table gradients, cffm_tables_adagrad_l2), mae, log_loss and hybrid with Adagrad, prepared as
    test_gpu_parity.test_other_losses prepares them."""
    c = dict(H.LOSS_SHAPE)
    if loss != 'square_l2':
        c['loss'] = loss
    cfg, p32, X, y = make('tmp-' + loss, c, trained_like=(loss != 'hybrid'))
    if loss == 'square_l2':
        cfg.lamda_bilinear = 0.02
    if loss == 'log_loss':
        y = (y > 0).astype(np.float32)
    if loss == 'hybrid':               # log_loss on the raw out is finite only for 0 < out < 1
        p32['bias'] = np.float32(0.5)
    B = X.shape[0]
    ref = run_histories('loss ' + loss, cfg, p32, B, H.leftover_batch(B), train_sequence(X, y))
    assert np.isfinite(ref['loss']).all() and np.isfinite(ref['theta']).all()


# ---- the other sequences ---------------------------------------------------------------------------------------------------------
def ws_part(eng, B, member, n):
    return host(eng.ws_tensor(B, member, (16 if member == 'scalars' else n,))[:n])


def row_grads_of(eng, B, out):
    for k, t in zip(('dEi', 'dEo', 'dfb'), eng.row_grads(B)):
        if t is not None:
            out[k] = host(t)


@pytest.mark.parametrize('name', H.SEQUENCE_CASES)
def test_forward_then_backward(name):
    cfg, p32, X, y = make(name)
    B = X.shape[0]
    ids, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()

    def seq(eng, history):
        eng.forward(ids, yt)
        eng.backward(yt, B)
        out = {'predictions': host(eng.predictions(B)), 'loss sum and loss': ws_part(eng, B, 'scalars', 2), 'grad': host(eng.grad)}
        for k, v in eng.export_grad().items():
            out['grad ' + k] = v
        row_grads_of(eng, B, out)
        return out
    run_histories(name + ' forward, backward', cfg, p32, B, H.leftover_batch(B), seq)


@pytest.mark.parametrize('name', H.SEQUENCE_CASES)
def test_dp_local_then_dp_apply(name):
    cfg, p32, X, y = make(name)
    B, F = X.shape[0], cfg.F
    ids, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    W = 1 + cfg.K + cfg.D + 1

    def seq(eng, history):
        n = int(eng.tl.n)
        g, block = eng.dp_local(ids, yt, B, B)
        out = {'grad_full': host(g[:n + 1]), 'block rows': host(block[:B * F * W].view(torch.int32))}
        if eng.lib.cffm_dp_runs_ok(eng._s, B):                   # the sorted run behind the rows is only valid there
            out['block keys'] = host(block[B * F * W:].view(torch.int32))
        eng.dp_apply(g.clone(), block.clone(), B, 1)
        out.update(state_of(eng))
        return out
    ref = run_histories(name + ' dp_local, dp_apply', cfg, p32, B, H.leftover_batch(B), seq)
    assert np.isfinite(ref['loss']).all()


def test_dp_local_dense_then_dp_apply_dense():
    """The dense-image route, where cffm_dp_runs_ok holds: the frappe shape at B = 100.  The image `flat` is zero on entry by contract
    and no part of the workspace: it is not dirtied."""
    name = H.pair_name(300, 100)
    cfg, p32, X, y = make(name, H.pair_case(100))
    B = X.shape[0]
    ids, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()

    def seq(eng, history):
        assert eng.lib.cffm_dp_runs_ok(eng._s, B) == 1
        flat = eng.dp_local_dense(ids, yt, B, B)
        out = {'flat': host(flat)}
        eng.dp_apply_dense(flat, B)
        out['flat on return'] = host(flat)
        # (this route leaves its gradients in `flat`: the engine's own gradient buffer is no output of it)
        out.update({k: v for k, v in state_of(eng).items() if k != 'grad' and not k.startswith('grad ')})
        return out
    ref = run_histories('frappe-shape b100 dp_local_dense, dp_apply_dense', cfg, p32, B, 300, seq)
    image = ref['flat'].size - cfg.M * (cfg.K + cfg.D + 1)        # [theta.n gradients | loss sum | pad | image of the tables]
    assert image >= int(hip.theta_layout(hip.make_shape(cfg)).n) + 1
    assert not ref['flat on return'][image:].any() and ref['flat'][image:].any()


@pytest.mark.parametrize('name', H.SEQUENCE_CASES)
def test_backward_unscaled_then_pack_rows_dedup(name):
    cfg, p32, X, y = make(name)
    B = X.shape[0]
    ids, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()

    def seq(eng, history):
        n = int(eng.tl.n)
        eng.forward(ids, yt)
        g, rows = eng.backward_unscaled(ids, yt, B, 2 * B, pack=False)
        assert rows is None
        local_ids, order, uniq, _, _, counts = eng.shard_plan(ids, 1, cfg.M)
        packed = eng.pack_rows_dedup(local_ids, order, uniq, B)
        u = int(counts.sum())
        return {'grad_full': host(g[:n + 1]), 'rows': host(packed[:u].view(torch.int32)), 'predictions': host(eng.predictions(B))}
    run_histories(name + ' backward_unscaled, pack_rows_dedup', cfg, p32, B, H.leftover_batch(B), seq)


@pytest.mark.parametrize('name', H.PACKED_CASES)
def test_forward_packed_then_backward_unscaled_packed(name):
    cfg, p32, X, y = br.make_branch_case(name)
    B = X.shape[0]
    uniq, inv = np.unique(br.clamp_ids(X, cfg.M).reshape(-1), return_inverse=True)
    rows = torch.from_numpy(uniq.astype(np.int32)).cuda()
    pos = torch.from_numpy(inv.reshape(-1).astype(np.int32)).cuda()
    yt = torch.from_numpy(y).cuda()

    def seq(eng, history):
        n = int(eng.tl.n)
        assert eng.packed_ok()
        packed = eng.gather_packed(rows)
        eng.forward_packed(packed, pos, yt, B)
        gf = eng.backward_unscaled_packed(packed, pos, yt, B, 2 * B)
        out = {'predictions': host(eng.predictions(B)), 'grad_full': host(gf[:n + 1])}
        row_grads_of(eng, B, out)
        return out
    run_histories(name + ' packed', cfg, p32, B, H.leftover_batch(B), seq)


@pytest.mark.parametrize('name', H.SEQUENCE_CASES)
def test_eval_sums(name):
    """eval_sums sweeps blocks of rows through cffm_predict - here two blocks of different size, so two layouts of one buffer -
    and adds them up through the partials of cffm_eval_sums, which get the same histories."""
    cfg, p32, X, y = make(name)
    B = X.shape[0]
    block = B // 2 + 3
    ids, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()

    def seq(eng, history):
        nbytes = int(eng.lib.cffm_eval_scratch_bytes())
        eng._eval_scratch = torch.zeros(nbytes, dtype=torch.uint8, device=eng.device)
        if history != 'zeros':
            eng.eval_sums_add(torch.linspace(-3, 3, 777, device=eng.device), torch.ones(777, device=eng.device), -0.5, 0.25,
                              torch.zeros(3, dtype=torch.float64, device=eng.device))
        if history in ('nan', 'huge'):
            eng._eval_scratch.fill_(0xFF if history == 'nan' else 0x7F)
        return {'sums': host(eng.eval_sums(ids, yt, -0.75, 0.75, block=block))}
    ref = run_histories(name + ' eval_sums', cfg, p32, block, H.leftover_batch(B), seq, batches=(B - block,))
    assert np.isfinite(ref['sums']).all() and ref['sums'][0] > 0


# ---- the library's other scratch arenas -------------------------------------------------------------------------------------------
def arena_histories(label, scratch, call, leftover_call, fills):
    """call() on zeroed scratch, then after leftover_call(), then under each of fills = [(history, fn(scratch))] on top of that."""
    scratch.zero_()
    ref = call()
    report(label, 'zeros', 'passed')
    for h, fn in [('leftover', None)] + list(fills):
        leftover_call()
        if fn is not None:
            fn(scratch)
        got = call()
        for k in ref:
            H.assert_same(h, '%s: %s' % (label, k), got[k], ref[k])
        report(label, h, 'passed')
    return ref


def byte_fills():
    return [('nan', lambda s: s.fill_(0xFF)), ('huge', lambda s: s.fill_(0x7F))]


def test_shared_sweep_scratch():
    """cffm_score_sweep keeps per-context blocks of floats in its scratch (C = 3 contexts, N = 130 candidates: two chunks and a rest)."""
    from tests import test_gpu_sweep as sw
    from cffm_amd.engine import HipEngine
    name, C, N = 'f3-relu', 3, 130
    cfg, p = sw.params_of(name)
    eng = HipEngine(cfg, params=p)
    ctx, cand = (torch.from_numpy(a).cuda() for a in sw.inputs_of(name, C, N))
    ctx2, cand2 = (torch.from_numpy(a).cuda() for a in sw.inputs_of(name, C, N, seed=77))
    scratch = eng._sweep_scratch(C)
    ref = arena_histories('shared sweep', scratch, lambda: {'scores': host(eng.score_candidates_shared(ctx, 1, cand))},
                          lambda: eng.score_candidates_shared(ctx2, 2, cand2), byte_fills())
    assert eng._sweep_scratch(C) is scratch and np.isfinite(ref['scores']).all() and np.unique(ref['scores']).size > N


def test_topk_scratch():
    """cffm_topk keeps the survivors of its chunks in the scratch as 64-bit keys whose low word is a candidate position that the last
    level indexes the scores with (rank.hip).  So this scratch is integer content: it gets the leftover of another call and keys
    that are well formed but wrong (positions inside [0, N)), never 0xFF.. or 0x7F.. bytes.  cffm_rank_of takes no scratch; it runs
    along on the same scores.  N = 8193: the smallest row that takes a second chunk, and with it the scratch."""
    from cffm_amd.engine import HipEngine
    cfg, p32, _, _ = make('tiny-relu')
    eng = HipEngine(cfg, params=p32)
    C, N, k = 3, 8193, 7
    rng = np.random.default_rng(5)
    scores = torch.from_numpy(rng.standard_normal((C, N)).astype(np.float32)).cuda()
    other = torch.from_numpy(rng.standard_normal((C, N)).astype(np.float32)).cuda()
    target = torch.from_numpy(np.asarray([0, N - 1, 4097], dtype=np.int32)).cuda()
    nbytes = int(eng.lib.cffm_topk_scratch_bytes(C, N, k))
    assert nbytes > 0
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=eng.device)
    eng._ws[('topk', C, N, k)] = scratch

    def wrong_keys(s):
        n = s.numel() // 8
        keys = (rng.integers(1, 1 << 31, size=n).astype(np.int64) << 32) | (0xffffffff - rng.integers(0, N, size=n).astype(np.int64))
        s[:n * 8].copy_(torch.from_numpy(keys.view(np.uint8)))

    def call():
        idx, val, count = eng.topk(scores, k)
        return {'idx': host(idx), 'val': host(val.view(torch.int32)), 'count': host(count), 'rank_of': host(eng.rank_of(scores, target))}
    ref = arena_histories('topk, rank_of', scratch, call, lambda: eng.topk(other, k), [('valid wrong keys', wrong_keys)])
    assert eng._ws[('topk', C, N, k)] is scratch
    order = np.argsort(-scores.cpu().numpy(), axis=1, kind='stable')[:, :k]
    np.testing.assert_array_equal(ref['idx'], order)


def test_shard_plan_scratch():
    """cffm_shard_plan's scratch is all integer (keys, flags, scans): the leftover of a plan for other ids only."""
    from tests import test_gpu_rows as rows
    from cffm_amd.spec import CFFMConfig
    F, B, M = 10, 256, rows.M_TAB
    eng = rows.engine(CFFMConfig(M=M, F=F, K=32, D=32))
    rng = np.random.default_rng(B)
    ids = torch.from_numpy((rng.integers(0, 150, size=(B, F)) * (M // 150)).astype(np.int32)).cuda()
    ids2 = torch.from_numpy(rng.integers(0, M, size=(B, F)).astype(np.int32)).cuda()
    n = B * F
    scratch = torch.zeros(int(eng.lib.cffm_shard_plan_scratch_bytes(n)), dtype=torch.uint8, device=eng.device)
    eng._ws[('plan', n)] = scratch

    def call():
        plan = eng.shard_plan(ids, 2, M)
        u = int(plan[5].sum())
        out = {lab: host(t) for lab, t in zip(('local_ids', 'order', 'uniq', 'pos'), plan)}
        out['send_rows'], out['counts'] = host(plan[4][:u]), host(plan[5])
        return out
    ref = arena_histories('shard_plan', scratch, call, lambda: eng.shard_plan(ids2, 3, M), [])
    assert eng._ws[('plan', n)] is scratch and int(ref['counts'].sum()) == np.unique(ids.cpu().numpy()).size
