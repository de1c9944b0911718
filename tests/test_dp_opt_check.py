"""What tests/_dp_opt_check.py can catch, on the CPU, in the manner of tests/test_update_check.py: a float32 numpy evaluation of
the multi-GPU SGD / Momentum apply with the late 1/L (duplicates summed in REVERSE slot order - the device sums in slot order)
passes the check; each planted fault is named by it."""
import copy

import numpy as np
import pytest

from oracle import update_check as uc
from tests import _dp_opt_check as dc
from tests import test_update_check as T

f = np.float32
M = T.M
OPTS = ['GradientDescentOptimizer', 'MomentumOptimizer']
LATE = [(7.31, 20, True), (913.2, 1000, True), (0.0, 20, True), (7.31, 20, False)]


def emulate(opt, pre, grad, ids, rows, lr, late, fault=None):
    """The device rule in float32: s = 1 / sqrtf(sum * (1 / Bg) + 1e-10f), g = fl(sum of duplicates) * s, then opt_update."""
    post = copy.deepcopy(pre)
    lr, mom = f(lr), f(uc.DEVICE_CONSTS['mom'])
    x = f(f(late[0]) * (f(1) / f(late[1]))) + f(1e-10)
    s = f(1) / np.sqrt(x) if late[2] else f(1)
    if fault == 'no_late':
        s = f(1)
    elif fault == 'late_twice':
        s = s * s

    def rule(name, sel, g):
        w = post[name].reshape(len(post[name]), -1) if name != 'theta' else post[name]
        if opt == 'GradientDescentOptimizer':
            w[sel] = w[sel] - lr * g
            return
        a1 = post['s1'][name].reshape(w.shape)
        a = a1[sel] + mom * g if fault == 'mom_on_g' else mom * a1[sel] + g
        a1[sel] = a
        w[sel] = w[sel] - lr * a

    rule('theta', slice(None), grad * s)
    skip = None
    if fault == 'drop_dup':
        skip = np.zeros(len(ids), dtype=bool)
        skip[int(np.flatnonzero(ids == 3)[-1])] = True
    for name, _, rkey, _ in uc.TABLES:
        if rows.get(rkey) is None:
            continue
        if fault == 'split':                  # the long segment of id 3 as two sequential updates: slots 0..5, then 6..11
            first = np.zeros(len(ids), dtype=bool)
            first[np.flatnonzero(ids == 3)[6:]] = True
            G, touched = T.seg_sum32(ids, rows[rkey], skip=first)
            rule(name, touched, G[touched] * s)
            G, _ = T.seg_sum32(ids, rows[rkey], skip=~first)
            rule(name, np.arange(M) == 3, G[3:4] * s)
            continue
        G, touched = T.seg_sum32(ids, rows[rkey], skip=skip)
        if fault == 'mom_untouched':
            a1 = post['s1'][name].reshape(M, -1)
            a1[~touched] = mom * a1[~touched]
        rule(name, touched, G[touched] * s)
    loss = float(np.sqrt(x)) if late[2] else float(f(late[0]) * (f(1) / f(late[1])))
    return post, loss


def _run(opt, late, fault=None, seed=0, rows_drop=None):
    pre, grad, ids, rows = T.make_case(opt, seed)
    if rows_drop:
        rows = dict(rows, **{rows_drop: None})
    post, loss = emulate(opt, pre, grad, ids, rows, 0.05, late, fault=fault)
    rep = dc.replay_late(opt, pre, grad, ids, rows, M, 0.05, *late)
    uc.check_update('%s %s' % (opt, late), pre, post, rep, loss=loss)


@pytest.mark.parametrize('late', LATE)
@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('seed', [0, 1])
def test_a_float32_evaluation_in_another_order_passes(opt, late, seed):
    _run(opt, late, seed=seed)


@pytest.mark.parametrize('opt', OPTS)
def test_a_disabled_branch_is_left_alone(opt):
    _run(opt, LATE[0], rows_drop='dEi')


# fault, optimizer, what the check must name.  A segment split in two is a fault of Momentum only: SGD's rule is additive, two
# updates of one row are the same real number as one update by the sum (and within the bound of either).
FAULTS = [('no_late', 'GradientDescentOptimizer', 'theta'), ('no_late', 'MomentumOptimizer', 'theta'),
          ('late_twice', 'GradientDescentOptimizer', 'theta'), ('late_twice', 'MomentumOptimizer', 'theta'),
          ('drop_dup', 'GradientDescentOptimizer', 'inner'), ('drop_dup', 'MomentumOptimizer', 'inner'),
          ('split', 'MomentumOptimizer', 'inner'), ('mom_untouched', 'MomentumOptimizer', r'inner\.s1 \(not moved\)'),
          ('mom_on_g', 'MomentumOptimizer', 'theta')]


@pytest.mark.parametrize('fault,opt,named', FAULTS)
def test_a_planted_fault_is_named(fault, opt, named):
    with pytest.raises(AssertionError, match=named):
        _run(opt, LATE[0], fault=fault)


def test_the_scale_faults_reach_the_tables_too():
    """With the dense gradient left out the table rows alone must show a scale left out or applied twice (this is what
    update_check.replay(late=...) itself would not see for these optimizers: it hands the rows to the rule unscaled)."""
    for opt in OPTS:
        for fault in ('no_late', 'late_twice'):
            pre, grad, ids, rows = T.make_case(opt, 0)
            post, loss = emulate(opt, pre, grad, ids, rows, 0.05, LATE[0], fault=fault)
            post['theta'], post['s1']['theta'] = pre['theta'], pre['s1']['theta']
            rep = dc.replay_late(opt, pre, None, ids, rows, M, 0.05, *LATE[0])
            with pytest.raises(AssertionError, match='inner'):
                uc.check_update('%s %s' % (opt, fault), pre, post, rep, loss=loss)
