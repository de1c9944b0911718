"""What oracle/update_check.py can catch, on the CPU: a float32 numpy evaluation of every update rule, summing the duplicates
of an id in REVERSE slot order (the device sums in slot order), passes the checker; each injected fault of the kind the
end-to-end checks let through fails it."""
import copy
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import update_check as uc  # noqa: E402

f = np.float32
M, N, K, D, NT = 40, 160, 8, 8, 50


def make_case(opt, seed=0):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 30, size=N).astype(np.int32)           # rows 30 .. 39 are never looked up
    ids[:12] = 3                                                  # one long segment
    ids[[20, 50, 90]] = [-1, M, M + 3]                            # out of range: skipped
    ids[[30, 31]] = [M - 1, 0]

    def grads(*shape):
        g = rng.standard_normal(shape) * 0.05
        g[rng.random(shape) < 0.1] = 0.0
        tiny = rng.random(shape) < 0.1
        g[tiny] *= 1e-4
        return g.astype(np.float32)
    rows = {'dEi': grads(N, K), 'dEo': grads(N, D), 'dfb': grads(N)}
    pre = {'theta': (rng.standard_normal(NT) * 0.5).astype(np.float32), 'inner': (rng.standard_normal((M, K)) * 0.5).astype(f),
           'outer': (rng.standard_normal((M, D)) * 0.5).astype(f), 'fbias': (rng.standard_normal(M) * 0.5).astype(f)}
    grad = grads(NT)
    if opt == 'AdagradOptimizer':
        s1 = {k: np.exp(rng.uniform(np.log(1e-4), 0, v.shape)).astype(f) for k, v in pre.items()}
        s1['inner'][:5] = f(1e-8)                                  # some rows still at the initial accumulator
    else:
        s1 = {k: (rng.standard_normal(v.shape) * 0.02).astype(f) for k, v in pre.items()}
    pre['s1'] = s1
    if opt == 'AdamOptimizer':
        pre['s2'] = {k: np.exp(rng.uniform(np.log(1e-6), np.log(1e-3), v.shape)).astype(f) for k, v in s1.items()}
    return pre, grad, ids, rows


def _order(ids):
    return np.arange(len(ids))[::-1]                              # reverse slot order


def seg_sum32(ids, r, skip=None):
    """fp32 duplicate sums, reverse slot order; rows [M, C] and the touched mask."""
    r = np.asarray(r, dtype=f).reshape(len(ids), -1)
    G = np.zeros((M, r.shape[1]), dtype=f)
    n = np.zeros(M, dtype=np.int64)
    for i in _order(ids):
        if skip is not None and skip[i]:
            continue
        if 0 <= ids[i] < M:
            G[ids[i]] = G[ids[i]] + r[i]
            n[ids[i]] += 1
    return G, n > 0


def emulate(opt, pre, grad, ids, rows, lr, lamda=0.0, lamda_att=0.0, late=None, t=None, fault=None):
    """The update in float32 numpy (every operation rounded), with an optional injected fault."""
    post = copy.deepcopy(pre)
    lr = f(lr)
    c = {k: f(v) for k, v in uc.DEVICE_CONSTS.items()}
    s = f(1)
    if late is not None:
        x = f(f(late[0]) * (f(1) / f(late[1]))) + f(1e-10)
        if late[2]:
            s = f(1) / np.sqrt(x)
        if fault == 'no_late':
            s = f(1)
        elif fault == 'late_twice':
            s = s * s
    if fault == 'swap_lam':
        lamda, lamda_att = lamda_att, lamda
    lam = {'inner': f(lamda), 'outer': f(lamda_att), 'fbias': f(0)}
    lr_t = f(uc.adam_lr_t(lr, t - 1 if fault == 'lr_t_prev' else t)) if opt == 'AdamOptimizer' else None

    def rule(name, sel, g):
        w = post[name].reshape(len(post[name]), -1) if name != 'theta' else post[name]
        a1 = post['s1'][name].reshape(w.shape)
        if opt == 'AdagradOptimizer':
            a = a1[sel] + g * g
            a1[sel] = a
            w[sel] = w[sel] - lr * g / np.sqrt(a)
        elif opt == 'GradientDescentOptimizer':
            w[sel] = w[sel] - lr * g
        elif opt == 'MomentumOptimizer':
            a = c['mom'] * a1[sel] + g
            a1[sel] = a
            w[sel] = w[sel] - lr * a
        else:
            a2 = post['s2'][name].reshape(w.shape)
            m = c['b1'] * a1[sel] + c['omb1'] * g
            v = c['b2'] * a2[sel] + c['omb2'] * g * g
            a1[sel], a2[sel] = m, v
            w[sel] = w[sel] - lr_t * m / (np.sqrt(v) + c['eps'])

    rule('theta', slice(None), grad * s)
    r = dict(rows)
    if fault == 'swap_bias':
        r['dEo'], r['dfb'] = r['dEo'].copy(), r['dfb'].copy()
        r['dEo'][:, -1], r['dfb'] = rows['dfb'], rows['dEo'][:, -1].copy()
    skip = None
    if fault == 'drop_dup':
        skip = np.zeros(len(ids), dtype=bool)
        skip[int(np.flatnonzero(ids == 3)[-1])] = True
    for name, _, rkey, _ in uc.TABLES:
        if r.get(rkey) is None:
            continue
        if fault == 'split':                  # the long segment of id 3 as two sequential updates: slots 0..5, then 6..11
            first = np.zeros(len(ids), dtype=bool)
            first[np.flatnonzero(ids == 3)[6:]] = True
            G, touched = seg_sum32(ids, r[rkey], skip=first)
            rule(name, touched, G[touched] * s)
            G, _ = seg_sum32(ids, r[rkey], skip=~first)
            rule(name, np.arange(M) == 3, G[3:4] * s)
            continue
        G, touched = seg_sum32(ids, r[rkey], skip=skip)
        G = G * s
        w = post[name].reshape(M, -1)
        if lamda > 0 and name != 'fbias':
            rule(name, slice(None), G + lam[name] * w)
        elif opt == 'AdamOptimizer' and fault != 'lazy_adam':
            rule(name, slice(None), G)
        else:
            if fault == 'mom_untouched':
                a1 = post['s1'][name].reshape(M, -1)
                a1[~touched] = c['mom'] * a1[~touched]
            rule(name, touched, G[touched])
    loss = None
    if late is not None:
        x = f(f(late[0]) * (f(1) / f(late[1]))) + f(1e-10)
        loss = float(np.sqrt(x)) if late[2] else float(f(late[0]) * (f(1) / f(late[1])))
    return post, loss


RULES = [('AdagradOptimizer', {}), ('AdagradOptimizer', dict(late=(7.31, 20, True))), ('AdagradOptimizer', dict(late=(7.31, 20, False))),
         ('AdagradOptimizer', dict(late=(0.0, 20, True))), ('AdagradOptimizer', dict(lamda=0.02, lamda_att=0.3)),
         ('GradientDescentOptimizer', {}), ('GradientDescentOptimizer', dict(lamda=0.02, lamda_att=0.3)),
         ('MomentumOptimizer', {}), ('MomentumOptimizer', dict(lamda=0.02, lamda_att=0.3)),
         ('AdamOptimizer', dict(t=1)), ('AdamOptimizer', dict(t=10)), ('AdamOptimizer', dict(t=12, lamda=0.02, lamda_att=0.3))]


def _run(opt, kw, fault=None, seed=0, rows_drop=None):
    pre, grad, ids, rows = make_case(opt, seed)
    if rows_drop:
        rows = dict(rows, **{rows_drop: None})
    lr = 0.05 if opt != 'AdamOptimizer' else 0.01
    post, loss = emulate(opt, pre, grad, ids, rows, lr, fault=fault, **kw)
    rep = uc.replay(opt, pre, grad, ids, rows, M, lr, **kw)
    uc.check_update('%s %s' % (opt, kw), pre, post, rep, loss=loss)


@pytest.mark.parametrize('opt,kw', RULES)
@pytest.mark.parametrize('seed', [0, 1])
def test_a_float32_evaluation_in_another_order_passes(opt, kw, seed):
    _run(opt, kw, seed=seed)


@pytest.mark.parametrize('opt', ['AdagradOptimizer', 'MomentumOptimizer', 'AdamOptimizer'])
def test_a_disabled_branch_is_left_alone(opt):
    _run(opt, dict(t=3) if opt == 'AdamOptimizer' else {}, rows_drop='dEi')


FAULTS = [('drop_dup', 'AdagradOptimizer', {}), ('drop_dup', 'AdagradOptimizer', dict(late=(7.31, 20, True))),
          ('drop_dup', 'MomentumOptimizer', {}), ('drop_dup', 'AdamOptimizer', dict(t=10)),
          ('split', 'AdagradOptimizer', {}), ('split', 'MomentumOptimizer', {}),
          ('no_late', 'AdagradOptimizer', dict(late=(7.31, 20, True))), ('late_twice', 'AdagradOptimizer', dict(late=(7.31, 20, True))),
          ('lr_t_prev', 'AdamOptimizer', dict(t=10)), ('lr_t_prev', 'AdamOptimizer', dict(t=12, lamda=0.02, lamda_att=0.3)),
          ('lazy_adam', 'AdamOptimizer', dict(t=10)), ('mom_untouched', 'MomentumOptimizer', {}),
          ('swap_bias', 'AdagradOptimizer', {}), ('swap_bias', 'AdamOptimizer', dict(t=10)),
          ('swap_lam', 'AdagradOptimizer', dict(lamda=0.02, lamda_att=0.3)), ('swap_lam', 'MomentumOptimizer', dict(lamda=0.02, lamda_att=0.3)),
          ('swap_lam', 'AdamOptimizer', dict(t=12, lamda=0.02, lamda_att=0.3))]


@pytest.mark.parametrize('fault,opt,kw', FAULTS)
def test_an_injected_fault_is_caught(fault, opt, kw):
    with pytest.raises(AssertionError):
        _run(opt, kw, fault=fault)


def test_adam_lr_t_moves_less_than_one_percent_late_but_the_bound_is_ulps():
    """Why lr_t of step t-1 is a fault the bound must see: near t = 10 it moves lr_t by under 1 %, while the bound on a
    parameter's move is a few ulps of it (plus 2 u of |w|)."""
    lr = 0.01
    assert abs(uc.adam_lr_t(lr, 10) / uc.adam_lr_t(lr, 9) - 1) < 0.01
    assert abs(uc.adam_lr_t(lr, 2) / uc.adam_lr_t(lr, 1) - 1) > 0.2
    w, m, v = np.array([0.3]), np.array([2e-3]), np.array([1e-5])
    bw, _, _ = uc.adam_bounds(w, m, v, m, v, np.array([0.0]), np.array([0.0]), uc.adam_lr_t(lr, 10), uc.DEVICE_CONSTS)
    q = uc.adam_lr_t(lr, 10) * m / (np.sqrt(v) + 1e-8)
    assert bw[0] < 1e-4 * q[0]


def test_theta_pad_mask_covers_exactly_the_channel_pads():
    class TL:
        n, P, Pp, live = 200, 3, 4, 2
        conv_w = [10, 100]
        conv_b = [80, 170]
    mask = uc.theta_pad_mask(TL)
    assert mask.sum() == 2 * (4 * (16 - 9) + 1)
    assert not mask[10:10 + 3].any() and mask[13] and mask[83] and not mask[82]
