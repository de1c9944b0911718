"""HipEngine.train_step_lists and CFFM.train_ranking on the device.  One list step: the loss and every gradient against
oracle.forward -> the float64 list loss (tests/_list_loss_ref.py) -> oracle.backward under oracle.parity.close, and the Adagrad
update against a float64 replay of the device's own gradients (oracle/update_check.py, as tests/test_gpu_update.py does).  Then 30
steps on one fixed batch bring the loss down, and train_ranking on a small synthetic split returns finite, falling epoch means."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cffm_amd.spec import CFFMConfig, init_params  # noqa: E402
from oracle import cffm_oracle as orc  # noqa: E402
from oracle import parity as T  # noqa: E402
from oracle import update_check as uc  # noqa: E402
from oracle.parity import adopt_device_kinks, close, inner_kink_slack, to64  # noqa: E402
from tests import _cand_ref as CR  # noqa: E402
from tests import _list_loss_ref as LR  # noqa: E402
from tests.test_gpu_update import host, pads_unchanged, row_inputs, state  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {
    'f4-d8': dict(F=4, D=8, G=6, Lg=4, fields=(1, 3), act='relu'),
    'f10-d32': dict(F=10, D=32, G=5, Lg=3, fields=(2, 7), act='selu'),
}


def make_case(name, seed=0):
    c = CASES[name]
    cfg = CFFMConfig(M=60 * c['F'], F=c['F'], K=c['D'], D=c['D'], activation=c['act'], lamda_att=1.3)
    p32 = init_params(cfg, seed=seed, dtype=np.float32)
    rng = np.random.default_rng(seed + 3)
    p32['feature_bias'] = (rng.standard_normal(p32['feature_bias'].shape) * 0.3).astype(np.float32)     # exactly 0 at init
    p32['outer_embeddings'] = (p32['outer_embeddings'] * 20.0).astype(np.float32)
    p32['inner_embeddings'] = (p32['inner_embeddings'] * 4.0).astype(np.float32)
    G, Lg, nf = c['G'], c['Lg'], len(c['fields'])
    ctx = rng.integers(0, cfg.M, size=(G, cfg.F)).astype(np.int32)
    ctx[1] = ctx[0]                                                     # two lists of one context
    cand = rng.integers(0, 12, size=(G, Lg, nf)).astype(np.int32) * 5   # few ids: duplicates within and across the lists
    cand[2] = cand[0]
    target = rng.integers(0, Lg, size=G).astype(np.int32)
    target[0], target[1] = 0, Lg - 1
    return cfg, p32, ctx, list(c['fields']), cand, target


def engine_for(cfg, p32):
    from cffm_amd.engine import HipEngine
    return HipEngine(cfg, params=p32)


def dev(a):
    return torch.from_numpy(a).cuda()


@pytest.mark.parametrize('kind', LR.KINDS)
@pytest.mark.parametrize('name', list(CASES))
def test_one_list_step(name, kind):
    cfg, p32, ctx, fields, cand, target = make_case(name)
    G, Lg = cand.shape[0], cand.shape[1]
    B = G * Lg
    X = CR.expand_tuples(ctx, fields, cand).astype(np.int32)           # [G * Lg, F] in the order cffm_expand_candidates_ex writes
    p64 = to64(p32)
    out_ref, c = orc.forward(p64, X, cfg)
    loss_ref, dout_ref, _ = LR.list_loss_ref(kind, out_ref.reshape(G, Lg), target)
    eng = engine_for(cfg, p32)
    pre = state(eng)
    L = eng.train_step_lists(dev(ctx), fields, dev(cand), dev(target), kind)
    post = state(eng)
    assert np.array_equal(host(eng._ws[('list_ids', B)]), X)
    close(host(eng.ws_tensor(B, 'out', (B,))), out_ref, 'list step out')
    close(host(L), np.array([loss_ref]), 'list step loss %s' % kind)
    # the gradients the step consumed: still in the workspace and in eng.grad
    print('%s: %d relu decisions adopted from the device' % (name, adopt_device_kinks(cfg, eng, B, c)))
    dout = dout_ref.reshape(-1)
    g = orc.backward(p64, c, dout, cfg)
    slack = inner_kink_slack(p64, c, dout, cfg)
    close(host(eng.ws_tensor(B, 'dout', (B,))), dout, 'list step dout %s' % kind)
    # Here dL/dout is the device's own (its forward, its list loss), just held to close(): dsl is that bound.  Every gradient is
    # linear in dL/dout, so it carries over as in oracle.parity.check_backward_stages - relative to example b's rows of the
    # per-example tensors, through dense_grad_slack to the batch sums.  It is what makes the gradients of the four additive biases
    # checkable at all: each is a multiple of sum_b dout_b, which a list loss makes 0 in exact arithmetic (the rows of dout sum to
    # 0), so the float64 reference is 1e-17 of rounding and the device's float32 sum 1e-8 of it.
    dsl = T.TOL * (np.abs(dout) + float(np.sqrt(np.mean(dout * dout))))
    rel_b = np.repeat(dsl / np.maximum(np.abs(dout), 1e-300), cfg.F)[:, None]
    dgs = T.dense_grad_slack(p64, c, dsl, cfg)
    rows = row_inputs(eng, B)
    ref = g['d_outer_rows'].reshape(B * cfg.F, -1)
    close(rows['dEo'], ref, 'list step dEo', extra=rel_b * np.abs(ref))
    ref = g['d_inner_rows'].reshape(B * cfg.F, -1)
    close(rows['dEi'], ref, 'list step dEi',
          extra=rel_b * np.abs(ref) + (slack['d_inner_rows'].reshape(B * cfg.F, -1) if 'd_inner_rows' in slack else 0.0))
    ref = g['d_bias_rows'].reshape(-1)
    close(rows['dfb'], ref, 'list step dfb', extra=rel_b[:, 0] * np.abs(ref))
    for k, v in eng.export_grad().items():
        extra = np.asarray(dgs[k]).reshape(v.shape) + (slack[k].reshape(v.shape) if k in slack else 0.0)
        close(v, np.asarray(g[k]).reshape(v.shape), 'list step grad ' + k, extra=extra)
    # the update: a float64 replay of Adagrad from the device's own gradients and its own state before the step
    label = 'list step %s %s' % (name, kind)
    rep = uc.replay('AdagradOptimizer', pre, host(eng.grad), X.reshape(-1), rows, cfg.M, cfg.lr)
    uc.check_update(label, pre, post, rep)
    pads_unchanged(label, eng, pre, post)


@pytest.mark.parametrize('kind', LR.KINDS)
@pytest.mark.parametrize('name', list(CASES))
def test_thirty_steps_on_one_batch_bring_the_loss_down(name, kind):
    cfg, p32, ctx, fields, cand, target = make_case(name)
    eng = engine_for(cfg, p32)
    args = (dev(ctx), fields, dev(cand), dev(target), kind)
    losses = [float(eng.train_step_lists(*args).cpu()[0]) for _ in range(30)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


def test_the_list_step_refuses_what_it_does_not_implement():
    cfg, p32, ctx, fields, cand, target = make_case('f4-d8')
    for kw, word in ((dict(optimizer='AdamOptimizer'), 'AdamOptimizer'), (dict(optimizer='MomentumOptimizer'), 'MomentumOptimizer'),
                     (dict(loss_type='log_loss'), 'log_loss')):
        other = CFFMConfig(M=cfg.M, F=cfg.F, K=cfg.K, D=cfg.D, activation='relu', **kw)
        eng = engine_for(other, init_params(other, seed=0, dtype=np.float32))
        pre = state(eng)
        with pytest.raises(ValueError, match=word):
            eng.train_step_lists(dev(ctx), fields, dev(cand), dev(target), 'bpr')
        post = state(eng)
        uc.check_exact(word + ' theta', post['theta'], pre['theta'])
    eng = engine_for(cfg, p32)
    with pytest.raises(ValueError, match='list loss'):
        eng.train_step_lists(dev(ctx), fields, dev(cand), dev(target), 'hinge')
    # list_loss on its own: the loss and dout of the scores handed in
    s = np.random.default_rng(1).standard_normal((6, 4)).astype(np.float32)
    for kind in LR.KINDS:
        loss, dout, terms = eng.list_loss(dev(s), dev(target), 6, 4, kind)
        ref = LR.list_loss_ref(kind, s, target)
        close(host(loss), np.array([ref[0]]), 'engine list_loss loss')
        close(host(dout).reshape(6, 4), ref[1], 'engine list_loss dout')
        close(host(terms), ref[2], 'engine list_loss terms')


@pytest.mark.parametrize('kind', LR.KINDS)
def test_train_ranking_on_a_synthetic_split(kind, tmp_path):
    """Rows with a positive label carry their (field 1, field 3) tuple from a small popular set, the others from a larger one: the
    list loss can be brought down by ranking the popular tuples first."""
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
    m = M.CFFM(Mf, 0, str(tmp_path / 'm'), 8, 8, 'square_loss', 1, 64, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer', 0, 0, 0,
               F, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'relu')
    means = m.train_ranking(data, (1, 3), negatives=3, loss=kind, epochs=3, seed=4)
    assert len(means) == 3 and np.isfinite(means).all()
    assert means[0] > means[1] > means[2], means
