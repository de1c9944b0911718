"""The fused list step on the device: cffm_backward_dout_fused, HipEngine.train_step_lists_fused and CFFM.train_ranking(step=...).

1. The switch is exact.  The fused top of the backward takes dL/dout from the caller instead of forming it - the same kernel body, a
   compile-time switch.  Under loss_type='square_loss', cffm_backward_unscaled with B_global = 1 forms dL/dout = (out - y) * 1.f / 1.f
   (L = 1, invB = 1/1: exactly out - y) and runs the launches cffm_backward runs; cffm_backward_dout_fused with dout = out - y formed
   in torch float32 runs the same kernels in the same order.  Every tensor both leave is compared bit for bit: no tolerance.
2. One fused list step against float64, held exactly as tests/test_gpu_rank_train.py::test_one_list_step holds the stage step.
3. The step entered on dirty buffers (tests/_ws_history.py) returns and updates the bits of the step on zeroed ones.
4. The route: which kernels a fused step at the frappe shape launches, and that they are fewer than the stage step's.
5. Refusals, train_ranking(step=...), and thirty steps on one batch."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cffm_amd import hip  # noqa: E402
from cffm_amd.spec import CFFMConfig, init_params  # noqa: E402
from oracle import cffm_oracle as orc  # noqa: E402
from oracle import parity as T  # noqa: E402
from oracle import update_check as uc  # noqa: E402
from oracle.parity import adopt_device_kinks, close, inner_kink_slack, to64  # noqa: E402
from tests import _cand_ref as CR  # noqa: E402
from tests import _list_loss_ref as LR  # noqa: E402
from tests import _ws_history as H  # noqa: E402
from tests.test_gpu_backward_dout import _same_bits, _snapshot, _views  # noqa: E402
from tests.test_gpu_update import host, pads_unchanged, row_inputs, state  # noqa: E402

pytestmark = pytest.mark.gpu
assert 'cffm_train_step_lists' in hip.PROTOTYPES          # the entry points this file is about


def engine_for(cfg, p32):
    from cffm_amd.engine import HipEngine
    return HipEngine(cfg, params=p32)


def dev(a):
    return torch.from_numpy(a).cuda()


def scaled_params(cfg, seed, rng):
    """The parameters of tests/test_gpu_rank_train.py and tests/test_gpu_backward_dout.py: every term and every activation live."""
    p32 = init_params(cfg, seed=seed, dtype=np.float32)
    p32['feature_bias'] = (rng.standard_normal(p32['feature_bias'].shape) * 0.3).astype(np.float32)     # exactly 0 at init
    p32['outer_embeddings'] = (p32['outer_embeddings'] * 20.0).astype(np.float32)
    p32['inner_embeddings'] = (p32['inner_embeddings'] * 4.0).astype(np.float32)
    return p32


# ---- 1. the switch, bit for bit ---------------------------------------------------------------------------------------------------
# each (shape, B) lands on another route below the fused top
SWITCH = {
    'f10-d32-b256-selu': dict(F=10, D=32, B=256, act='selu'),      # the compiled frappe instances
    'f10-d32-b100-elu': dict(F=10, D=32, B=100, act='elu'),        # conv01_bwd, 156 workgroups without an example
    'f7-d32-b63-gelu': dict(F=7, D=32, B=63, act='gelu'),          # B < 64: pair route, the top weight gradients deferred
    'f11-d32-b64-relu': dict(F=11, D=32, B=64, act='relu'),        # Pp = 64
    'f6-d64-b70-elu': dict(F=6, D=64, B=70, act='elu'),            # D != 32
    'f4-d8-b24-relu': dict(F=4, D=8, B=24, act='relu'),            # live = 2
}


def switch_case(name):
    c = SWITCH[name]
    cfg = CFFMConfig(M=40 * c['F'], F=c['F'], K=c['D'], D=c['D'], activation=c['act'], lamda_att=1.3, loss_type='square_loss')
    rng = np.random.default_rng(11)
    p32 = scaled_params(cfg, 0, rng)
    X = rng.integers(0, cfg.M, size=(c['B'], cfg.F)).astype(np.int32)
    X[1] = X[0]                                                    # duplicate ids in every column
    y = rng.choice([-1.0, 1.0], size=c['B']).astype(np.float32)
    return cfg, p32, X, y


def switch_snapshot(eng, cfg, B, grad):
    snap = _snapshot(eng, cfg, B)
    snap['grad'] = host(grad)[:int(eng.tl.n)]
    return snap


def dirty_members(eng, cfg, B):
    """Everything in the workspace that the forward did not write and the backward writes or may read, and eng.grad."""
    _, wl = eng.workspace(B)
    d = [eng.ws_tensor(B, 'scalars', (16,)), eng.ws_tensor(B, 'gpart', (int(wl.gpart_floats),)), eng.ws_tensor(B, 'sqerr', (B,))]
    return d + list(_views(eng, cfg, B).values())


@pytest.mark.parametrize('name', list(SWITCH))
def test_the_switch_is_exact(name):
    cfg, p32, X, y = switch_case(name)
    B = X.shape[0]
    eng = engine_for(cfg, p32)
    assert eng.shape.loss == 0 and bool(eng.lib.cffm_list_step_ok(eng._s, B))
    ids, yt = dev(X), dev(y)
    eng.forward(ids, yt)
    grad_full, rows = eng.backward_unscaled(ids, yt, B, 1, pack=False)
    assert rows is None
    want = switch_snapshot(eng, cfg, B, grad_full)
    assert np.isfinite(want['grad']).all() and np.abs(want['grad']).max() > 0
    # the same forward again, then the caller's dL/dout through the fused launches
    eng.forward(ids, yt)
    dout = eng.predictions(B) - yt
    assert np.array_equal(host(dout).view(np.uint32), want['dout'].view(np.uint32)), 'out - y in torch is not the device\'s dL/dout'
    for t in dirty_members(eng, cfg, B):
        t.zero_()
    eng.backward_dout_fused(dout, B)
    got = switch_snapshot(eng, cfg, B, eng.grad)
    _same_bits(got, want, name + ': cffm_backward_dout_fused vs cffm_backward_unscaled')
    # twice the dout: twice every gradient, bit for bit
    tiny = min(float(np.abs(v[v != 0]).min()) for v in got.values() if (v != 0).any())
    assert tiny > 1e-35, 'the gradients reach down to denormals (%g): doubling would not be exact' % tiny
    eng.backward_dout_fused(2.0 * dout, B)
    _same_bits(switch_snapshot(eng, cfg, B, eng.grad), {k: 2.0 * v for k, v in got.items()}, name + ' doubled')
    # a workspace dirty outside what the forward wrote: the bits of the clean one
    for fill in (float('nan'), 3.39e38):
        for t in dirty_members(eng, cfg, B):
            t.fill_(fill)
        eng.backward_dout_fused(dout, B)
        _same_bits(switch_snapshot(eng, cfg, B, eng.grad), got, '%s dirty (%r)' % (name, fill))


def test_backward_dout_fused_refuses_where_the_fused_top_does_not_run():
    cfg = CFFMConfig(M=480, F=12, K=32, D=32, activation='relu')           # Pp = 80
    eng = engine_for(cfg, init_params(cfg, seed=0, dtype=np.float32))
    X = np.random.default_rng(0).integers(0, cfg.M, size=(6, cfg.F)).astype(np.int32)
    eng.forward(dev(X), None)
    pre = host(eng.grad)
    with pytest.raises(RuntimeError, match='unsupported'):
        eng.backward_dout_fused(torch.ones(6, device='cuda'), 6)
    torch.cuda.synchronize()
    assert np.array_equal(host(eng.grad).view(np.uint32), pre.view(np.uint32))


# ---- 2. one fused list step against float64 ---------------------------------------------------------------------------------------
STEP = {
    'f10-d32-g16x4': dict(F=10, D=32, G=16, Lg=4, fields=(2, 7), act='selu'),      # B = 64: conv01_bwd
    'f10-d32-g5x3': dict(F=10, D=32, G=5, Lg=3, fields=(2, 7), act='selu'),        # B = 15: pair route
    'f4-d8-g6x4': dict(F=4, D=8, G=6, Lg=4, fields=(1, 3), act='relu'),            # stage forward, live = 2
    'f11-d32-g16x4': dict(F=11, D=32, G=16, Lg=4, fields=(2, 10), act='relu'),     # stage forward, Pp = 64 top places the keys
}


def step_case(name, seed=0, **over):
    """tests/test_gpu_rank_train.py::make_case for the dict c: duplicate contexts, duplicate candidates within and across the lists,
    a target at position 0 and one at Lg - 1."""
    c = dict(STEP[name], **over)
    cfg = CFFMConfig(M=60 * c['F'], F=c['F'], K=c['D'], D=c['D'], activation=c['act'], lamda_att=1.3, **c.get('cfg', {}))
    rng = np.random.default_rng(seed + 3)
    p32 = scaled_params(cfg, seed, rng)
    G, Lg, nf = c['G'], c['Lg'], len(c['fields'])
    ctx = rng.integers(0, cfg.M, size=(G, cfg.F)).astype(np.int32)
    ctx[1] = ctx[0]
    cand = rng.integers(0, 12, size=(G, Lg, nf)).astype(np.int32) * 5
    cand[2] = cand[0]
    target = rng.integers(0, Lg, size=G).astype(np.int32)
    target[0], target[1] = 0, Lg - 1
    return cfg, p32, ctx, list(c['fields']), cand, target


@pytest.mark.parametrize('kind', LR.KINDS)
@pytest.mark.parametrize('name', list(STEP))
def test_one_fused_list_step(name, kind):
    cfg, p32, ctx, fields, cand, target = step_case(name)
    G, Lg = cand.shape[0], cand.shape[1]
    B = G * Lg
    X = CR.expand_tuples(ctx, fields, cand).astype(np.int32)
    p64 = to64(p32)
    out_ref, c = orc.forward(p64, X, cfg)
    loss_ref, dout_ref, _ = LR.list_loss_ref(kind, out_ref.reshape(G, Lg), target)
    eng = engine_for(cfg, p32)
    assert eng.list_step_ok(B)
    pre = state(eng)
    L = eng.train_step_lists_fused(dev(ctx), fields, dev(cand), dev(target), kind)
    post = state(eng)
    assert np.array_equal(host(eng._ws[('list_ids', B)]), X)
    close(host(eng.ws_tensor(B, 'out', (B,))), out_ref, 'fused list step out')
    close(host(L), np.array([loss_ref]), 'fused list step loss %s' % kind)
    print('%s: %d relu decisions adopted from the device' % (name, adopt_device_kinks(cfg, eng, B, c)))
    dout = dout_ref.reshape(-1)
    g = orc.backward(p64, c, dout, cfg)
    slack = inner_kink_slack(p64, c, dout, cfg)
    close(host(eng.ws_tensor(B, 'dout', (B,))), dout, 'fused list step dout %s' % kind)
    assert np.array_equal(host(eng.ws_tensor(B, 'dout', (B,))).view(np.uint32), host(eng._ws[('list_out', G, Lg)][0]).view(np.uint32))
    # the slack terms of test_one_list_step: dL/dout is the device's own, held to close(), and every gradient is linear in it
    dsl = T.TOL * (np.abs(dout) + float(np.sqrt(np.mean(dout * dout))))
    rel_b = np.repeat(dsl / np.maximum(np.abs(dout), 1e-300), cfg.F)[:, None]
    dgs = T.dense_grad_slack(p64, c, dsl, cfg)
    rows = row_inputs(eng, B)
    ref = g['d_outer_rows'].reshape(B * cfg.F, -1)
    close(rows['dEo'], ref, 'fused list step dEo', extra=rel_b * np.abs(ref))
    ref = g['d_inner_rows'].reshape(B * cfg.F, -1)
    close(rows['dEi'], ref, 'fused list step dEi',
          extra=rel_b * np.abs(ref) + (slack['d_inner_rows'].reshape(B * cfg.F, -1) if 'd_inner_rows' in slack else 0.0))
    ref = g['d_bias_rows'].reshape(-1)
    close(rows['dfb'], ref, 'fused list step dfb', extra=rel_b[:, 0] * np.abs(ref))
    for k, v in eng.export_grad().items():
        extra = np.asarray(dgs[k]).reshape(v.shape) + (slack[k].reshape(v.shape) if k in slack else 0.0)
        close(v, np.asarray(g[k]).reshape(v.shape), 'fused list step grad ' + k, extra=extra)
    label = 'fused list step %s %s' % (name, kind)
    rep = uc.replay('AdagradOptimizer', pre, host(eng.grad), X.reshape(-1), rows, cfg.M, cfg.lr)
    uc.check_update(label, pre, post, rep)
    pads_unchanged(label, eng, pre, post)


# ---- 3. dirty state ---------------------------------------------------------------------------------------------------------------
FILLS = {'zeros': 0.0, 'leftover': 7.0, 'nan': float('nan'), 'huge': 3.39e38}      # for the buffers outside the workspace


@pytest.mark.parametrize('name,G_other', [('f10-d32-g16x4', 33), ('f10-d32-g5x3', 16), ('f4-d8-g6x4', 13)])
def test_the_fused_step_on_dirty_buffers(name, G_other):
    """The workspace through the histories of tests/_ws_history.py (the leftover run is a fused list step on G_other other lists); the
    list-loss scratch and the ('list_out', G, Lg) buffers, which the engine keeps outside it, filled with the history's value."""
    from tests.test_gpu_ws_history import state_of
    kind = 'softmax' if 'g5x3' in name else 'bpr'
    cfg, p32, ctx, fields, cand, target = step_case(name)
    G, Lg = cand.shape[0], cand.shape[1]
    B = G * Lg
    _, _, ctx2, _, cand2, target2 = step_case(name, seed=5, G=G_other)
    args = (dev(ctx), fields, dev(cand), dev(target), kind)
    args2 = (dev(ctx2), fields, dev(cand2), dev(target2), kind)
    ref = None
    for h in H.HISTORIES:
        eng = engine_for(cfg, p32)
        H.pool_buffer(eng, B, G_other * Lg)
        H.enter(h, eng, p32, B, G_other * Lg, lambda e: e.train_step_lists_fused(*args2))
        ptr = eng._pool.buf.data_ptr()
        eng._list_scratch(max(G, G_other)).view(torch.float32).fill_(FILLS[h])
        eng._ws[('list_out', G, Lg)] = (torch.full((B,), FILLS[h], device='cuda'), torch.full((G,), FILLS[h], device='cuda'))
        if h == 'nan':
            assert bool(torch.isnan(eng.ws_tensor(B, 'gpart', (4,))).all()) and bool(torch.isnan(eng.ws_tensor(B, 'out', (1,))).all())
        loss = eng.train_step_lists_fused(*args)
        torch.cuda.synchronize()
        assert eng._pool.buf.data_ptr() == ptr, 'the step re-allocated the workspace it was to find dirty'
        got = state_of(eng)
        got['returned loss'] = host(loss)
        got['list_ids'] = host(eng._ws[('list_ids', B)])
        got['list dout'], got['list terms'] = (host(t) for t in eng._ws[('list_out', G, Lg)])
        if ref is None:
            ref = got
            assert np.isfinite(ref['returned loss']).all() and np.isfinite(ref['theta']).all()
        else:
            assert list(got) == list(ref)
            for k in ref:
                H.assert_same(h, '%s: %s' % (name, k), got[k], ref[k], eng.tl if k in ('theta', 'theta_acc', 'grad') else None)
        del eng


# ---- 4. the route -----------------------------------------------------------------------------------------------------------------
def kernels_of(fn):
    """{kernel name: launches} of one call of fn under torch.profiler (after a warm-up call)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = {}
    for ev in prof.events():
        if str(getattr(ev, 'device_type', '')).endswith('CUDA') and 'memcpy' not in ev.name.lower() and 'memset' not in ev.name.lower():
            names[ev.name] = names.get(ev.name, 0) + 1
    return names


def route_counts():
    """({kernel: launches} of one fused step, the same of one stage step) at f10-d32, G = 64 lists of 4 = 256 rows."""
    cfg = CFFMConfig(M=5382, F=10, K=32, D=32, activation='selu')
    eng = engine_for(cfg, init_params(cfg, seed=0, dtype=np.float32))
    rng = np.random.default_rng(3)
    G, Lg = 64, 4
    args = (dev(rng.integers(0, cfg.M, size=(G, 10)).astype(np.int32)), [1, 6],
            dev(rng.integers(0, cfg.M, size=(G, Lg, 2)).astype(np.int32)), dev(rng.integers(0, Lg, size=G).astype(np.int32)), 'bpr')
    return kernels_of(lambda: eng.train_step_lists_fused(*args)), kernels_of(lambda: eng.train_step_lists(*args))


def test_the_fused_step_runs_the_launches_of_the_pointwise_step():
    """The profiler runs in a process of its own, started fresh and under a time limit: a tracer cannot be bounded inside the process
    that runs the whole suite."""
    import json
    import subprocess
    code = ('import json, sys; sys.path.insert(0, %r); from tests import test_gpu_list_step as t; '
            'print("ROUTE " + json.dumps(t.route_counts()))' % ROOT)
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    row = [ln for ln in r.stdout.splitlines() if ln.startswith('ROUTE ')]
    assert r.returncode == 0 and row, (r.returncode, r.stderr[-600:])
    fused, stages = json.loads(row[0][6:])
    n_fused, n_stages = sum(fused.values()), sum(stages.values())
    print('kernels per step at f10-d32 B = 256: fused %d, stages %d' % (n_fused, n_stages))
    print('fused: %s' % sorted(fused))
    assert n_fused > 0 and n_stages > 0, 'the profiler recorded no kernel'
    for word in ('bwd_top_kernel', 'conv01_bwd_kernel', 'fwd_all_kernel', 'update_all_kernel'):
        assert any(word in n for n in fused), (word, sorted(fused))
    assert not any('head_bwd_dout_kernel' in n for n in fused), sorted(fused)
    assert any('head_bwd_dout_kernel' in n for n in stages), sorted(stages)
    assert n_fused == 7, fused
    assert n_fused < n_stages


# ---- 5. refusals, train_ranking(step=...), thirty steps ---------------------------------------------------------------------------
def test_the_fused_step_refuses_what_it_does_not_serve():
    cfg, p32, ctx, fields, cand, target = step_case('f10-d32-g16x4', G=65)          # B = 260
    eng = engine_for(cfg, p32)
    assert not eng.list_step_ok(260) and eng.list_step_ok(256)
    pre = state(eng)
    with pytest.raises(ValueError, match='260'):
        eng.train_step_lists_fused(dev(ctx), fields, dev(cand), dev(target), 'bpr')
    post = state(eng)
    for k in ('theta', 'inner', 'outer', 'fbias'):
        uc.check_exact('B = 260 ' + k, post[k], pre[k])
        uc.check_exact('B = 260 slot ' + k, post['s1'][k], pre['s1'][k])
    cfg, p32, ctx, fields, cand, target = step_case('f4-d8-g6x4')
    for kw, word in ((dict(optimizer='AdamOptimizer'), 'AdamOptimizer'), (dict(loss_type='log_loss'), 'log_loss'),
                     (dict(lamda_bilinear=0.01), 'list_step_ok')):
        other = CFFMConfig(M=cfg.M, F=cfg.F, K=cfg.K, D=cfg.D, activation='relu', **kw)
        eng = engine_for(other, init_params(other, seed=0, dtype=np.float32))
        assert not eng.list_step_ok(24)
        pre = state(eng)
        with pytest.raises(ValueError, match=word):
            eng.train_step_lists_fused(dev(ctx), fields, dev(cand), dev(target), 'bpr')
        post = state(eng)
        for k in ('theta', 'inner', 'outer', 'fbias'):
            uc.check_exact(word + ' ' + k, post[k], pre[k])
            uc.check_exact(word + ' slot ' + k, post['s1'][k], pre['s1'][k])
    eng = engine_for(cfg, p32)
    with pytest.raises(ValueError, match='list loss'):
        eng.train_step_lists_fused(dev(ctx), fields, dev(cand), dev(target), 'hinge')


@pytest.mark.parametrize('kind', LR.KINDS)
@pytest.mark.parametrize('name', list(STEP))
def test_thirty_fused_steps_on_one_batch_bring_the_loss_down(name, kind):
    cfg, p32, ctx, fields, cand, target = step_case(name)
    eng = engine_for(cfg, p32)
    args = (dev(ctx), fields, dev(cand), dev(target), kind)
    losses = [float(eng.train_step_lists_fused(*args).cpu()[0]) for _ in range(30)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


def ranking_model(tmp_path, tag):
    """The synthetic split of tests/test_gpu_rank_train.py: rows with a positive label carry their (field 1, field 3) tuple from a
    small popular set, so ranking the popular tuples first brings a list loss down.  160 positives."""
    from cffm_amd import CFFM as M
    F, Mf = 6, 400
    rng = np.random.default_rng(2)
    n = 320
    X = rng.integers(0, Mf, size=(n, F)).astype(np.int32)
    y = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32)
    popular = rng.integers(0, 50, size=(8, 2))
    others = rng.integers(50, Mf, size=(40, 2))
    pick = np.where((y > 0)[:, None], popular[rng.integers(0, 8, size=n)], others[rng.integers(0, 40, size=n)])
    X[:, 1], X[:, 3] = pick[:, 0], pick[:, 1]
    data = {'X': X.tolist(), 'Y': y.tolist()}
    m = M.CFFM(Mf, 0, str(tmp_path / tag), 8, 8, 'square_loss', 1, 64, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer', 0, 0, 0,
               F, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'relu')
    return m, data


@pytest.mark.parametrize('kind', LR.KINDS)
def test_train_ranking_fused_and_auto(kind, tmp_path):
    # 160 lists of 4 rows.  'fused': 40 lists a step, B = 160, every step served.  'auto': 70 lists a step - B = 280 is not served and
    # takes the stage step, the ragged last step of 20 lists (B = 80) is served and takes the fused one.
    m, data = ranking_model(tmp_path, 'fused')
    assert m.train_ranking(data, (1, 3), negatives=3, loss=kind, epochs=0) == []     # builds the engine
    assert m.engine.list_step_ok(160) and not m.engine.list_step_ok(280) and m.engine.list_step_ok(80)
    means = m.train_ranking(data, (1, 3), negatives=3, loss=kind, epochs=3, seed=4, lists_per_step=40, step='fused')
    assert len(means) == 3 and np.isfinite(means).all() and means[0] > means[1] > means[2], means
    with pytest.raises(ValueError, match='280'):
        m.train_ranking(data, (1, 3), negatives=3, loss=kind, epochs=1, seed=4, lists_per_step=70, step='fused')
    m, data = ranking_model(tmp_path, 'auto')
    means = m.train_ranking(data, (1, 3), negatives=3, loss=kind, epochs=3, seed=4, lists_per_step=70, step='auto')
    assert len(means) == 3 and np.isfinite(means).all() and means[0] > means[1] > means[2], means
    with pytest.raises(ValueError, match='step must be'):
        m.train_ranking(data, (1, 3), negatives=3, loss=kind, step='fast')


def test_train_ranking_stages_is_the_default(tmp_path):
    runs = []
    for tag, kw in (('a', {}), ('b', dict(step='stages'))):
        m, data = ranking_model(tmp_path, tag)
        means = m.train_ranking(data, (1, 3), negatives=3, loss='bpr', epochs=2, seed=4, **kw)
        torch.cuda.synchronize()
        runs.append((means, host(m.engine.theta), host(m.engine.inner), host(m.engine.outer), host(m.engine.fbias)))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
