"""oracle/branch_check.py on the CPU: the checker must be able to fail.

A numpy "device" evaluates the inner branch and the head in float32.  Evaluated in plain sequential order, with numpy's pairwise
sums and in reverse order it passes every tier on every case; with one of the listed faults it fails, and each fault names the tier
and the tensor that must catch it.  The floor constants are held to the gap they were chosen in: the smallest floor statistic of a
fault that only the floor tier can see is at least 3x the largest of the passing evaluations (both relative to the floor limit).
The ambiguity cap (at most 1e-4 of the units of a case) is checked here for every case of tests/test_gpu_branches.py, from the
float64 reference alone."""
import numpy as np
import pytest

from oracle import branch_check as bc
from oracle import cffm_oracle as orc
from tests import test_gpu_branches as G

f32 = np.float32
CPU_CASES = {      # the GPU cases' parameters at CPU-sized batches
    'relu-f32-k64': dict(M=600, F=32, K=64, D=64, act='relu', B=3, family=(32, 16, 'circ')),
    'gelu-f20-k64': dict(M=600, F=20, K=64, D=64, act='gelu', B=4, family=(32, 8, 'generic')),
    'elu-f28-k32': dict(M=600, F=28, K=32, D=32, act='elu', B=4, family=(16, 8, 'generic')),
    'selu-f10-k32': dict(M=600, F=10, K=32, D=32, act='selu', B=24, family=None),
    'prelu-f5-k32-b300': dict(M=400, F=5, K=32, D=32, act='prelu', B=300, family=None),        # B >= 256: the floor tier of the batch sums
    'tie-elu-f6-k32': dict(M=700, F=6, K=32, D=32, act='elu', B=16, family=None, tie=True),
    'tie-gelu-f7-k16': dict(M=700, F=7, K=16, D=32, act='gelu', B=16, family=None, tie=True),
}
ORDERS = ('seq', 'pair', 'rev')


def _case(name, **over):
    G.CASES['cpu-' + name] = dict(CPU_CASES[name], **over)
    try:
        return G.make_branch_case('cpu-' + name)
    finally:
        G.CASES.pop('cpu-' + name)


def inner_device(cfg, p32, X, dout, order='seq', fault=None):
    """The inner branch as a float32 numpy device; fault: see FAULTS_INNER."""
    E, cw, cb, dw, db = G.inner_inputs(cfg, p32, X)
    P, K2 = cfg.P, cfg.K // 2
    kw = {}
    d3 = dw.reshape(P, K2, 2).copy()
    if fault == 'drop_last_unit':
        d3[P - 1, K2 - 1, :] = 0
        kw['dw_fwd'] = d3
    elif fault == 'drop_group_last':              # p = UPT * g + UPT - 1 of thread group g = 3 (UPT = 8)
        d3[8 * 3 + 7, K2 // 2, :] = 0
        kw['dw_fwd'] = d3
    elif fault == 'unit_twice':
        d3[P // 2, 1, :] *= 2
        kw['dw_fwd'] = d3
    elif fault == 'dense_weights_swapped':        # s0 * w.y + s1 * w.x
        d3[P // 3, 2, :] = d3[P // 3, 2, ::-1].copy()
        kw['dw_fwd'] = d3
    elif fault == 'cw_transposed':
        cw = cw[[0, 2, 1, 3]]
    elif fault == 'cb_swapped':
        cb = cb[::-1]
    elif fault == 'no_dense_bias':
        db = np.zeros(1, f32)
    elif fault in ('no_relu', 'tie_second', 'grad_from_x'):
        kw['fault'] = fault
    out, _ = bc.inner_eval(E, cw, cb, dw, db, cfg.activation, dout, dtype=f32, order=order, **kw)
    out.pop('units')
    return out


# fault -> (tensor, tier) that must report it
FAULTS_INNER = {
    'drop_last_unit': ('inner_out', 'floor'), 'drop_group_last': ('inner_out', 'floor'), 'unit_twice': ('inner_out', 'floor'),
    'dense_weights_swapped': ('inner_out', 'floor'), 'cw_transposed': ('inner_out', 'floor'), 'cb_swapped': ('inner_out', 'floor'),
    'no_dense_bias': ('inner_out', 'floor'), 'no_relu': ('inner_out', 'floor'), 'grad_from_x': ('dEi', 'hard'),
}
FLOOR_ONLY = ('drop_last_unit', 'drop_group_last', 'unit_twice', 'dense_weights_swapped')
PASSING, FAILING = {}, {}          # floor statistic / limit of the passing evaluations and of the floor-only faults


def _floor_ratio(st):
    return st['q'] / (bc.FLOOR_FACTOR * st['q_replay'] + bc.FLOOR_SLACK)


def _dout(B, seed=3):
    return (np.random.default_rng(seed).standard_normal(B) * 0.02).astype(f32)


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('name', list(CPU_CASES))
def test_inner_float32_evaluations_pass(name, order):
    cfg, p32, X, y = _case(name)
    dout = _dout(X.shape[0])
    st = bc.check_inner(name, inner_device(cfg, p32, X, dout, order), *G.inner_inputs(cfg, p32, X), cfg.activation, dout=dout)
    for k, v in st.items():
        if isinstance(v, dict) and 'q_replay' in v:
            PASSING[(name, order, k)] = _floor_ratio(v)
            print(name, order, k, 'q %.3g q_replay %.3g hard %.3g' % (v['q'], v['q_replay'], v['hard']))


# relu'(relu(I)) == relu'(I) and relu(relu(z)) == relu(z): those two are not faults of the relu case
INNER_FAULT_PARAMS = [(n, f) for n in ('relu-f32-k64', 'gelu-f20-k64', 'elu-f28-k32', 'selu-f10-k32') for f in FAULTS_INNER
                      if not (n.startswith('relu') and f in ('grad_from_x', 'no_relu'))]


@pytest.mark.parametrize('name,fault', INNER_FAULT_PARAMS)
def test_inner_faults_fail(name, fault):
    cfg, p32, X, y = _case(name)
    dout = _dout(X.shape[0])
    sink = {}
    with pytest.raises(AssertionError) as e:
        bc.check_inner(name, inner_device(cfg, p32, X, dout, 'seq', fault), *G.inner_inputs(cfg, p32, X), cfg.activation, dout=dout, sink=sink)
    tensor, tier = FAULTS_INNER[fault]
    assert any(tensor in ln and '[' + tier + ']' in ln for ln in str(e.value).splitlines()), (fault, str(e.value))
    if fault in FLOOR_ONLY:
        if sink['inner_out']['n_terms'] > 10000:        # one unit among tens of thousands: below the hard bound, the floor tier alone sees it
            assert sink['inner_out']['fails'] == ['floor']
        FAILING[(name, fault)] = _floor_ratio(sink['inner_out'])
        print(name, fault, 'q %.3g q_replay %.3g' % (sink['inner_out']['q'], sink['inner_out']['q_replay']))


@pytest.mark.parametrize('name', ['tie-elu-f6-k32', 'tie-gelu-f7-k16'])
def test_second_on_tie_fails(name):
    """Exact ties are not ambiguous: a max-pool gradient that goes to x1 on a tie fails the hard tier of dEi."""
    cfg, p32, X, y = _case(name)
    dout = _dout(X.shape[0])
    ref, _ = bc.inner_eval(*G.inner_inputs(cfg, p32, X), cfg.activation)
    u = ref['units']
    assert int((u['x0'] == u['x1']).sum()) >= u['x0'].size // 4 and not u['tie'][u['x0'] == u['x1']].any()
    with pytest.raises(AssertionError) as e:
        bc.check_inner(name, inner_device(cfg, p32, X, dout, 'seq', 'tie_second'), *G.inner_inputs(cfg, p32, X), cfg.activation, dout=dout)
    assert any('dEi [hard]' in ln for ln in str(e.value).splitlines()), str(e.value)


@pytest.mark.parametrize('name', [k for k, c in G.CASES.items() if c.get('inner_conv', 1)])
def test_ambiguity_cap_of_the_gpu_cases(name):
    cfg, p32, X, y = G.make_branch_case(name)
    assert G.giw_family(cfg.F, cfg.K, cfg.D) == G.CASES[name]['family']
    ref, _ = bc.inner_eval(*G.inner_inputs(cfg, p32, X), cfg.activation)
    n, units = bc.ambiguous_units(ref['units'])
    assert n <= bc.AMBIG_MAX * units, (name, n, units)
    if G.CASES[name].get('probe'):
        p, t, ch = G.CASES[name]['probe']
        assert p < cfg.P and t < cfg.K // 2


# ---- head ----------------------------------------------------------------------------------------------------------------------
def head_device(cfg, p32, X, y, loss, order='seq', fault=None, B_global=None, unscaled=False):
    """The head as a float32 numpy device, each stage fed by the device's own output of the stage before; fault: see FAULTS_HEAD."""
    B = X.shape[0]
    Bg = B if B_global is None else B_global
    Xc = G.clamp_ids(X, cfg.M)
    p = {k: np.asarray(v, f32) for k, v in p32.items()}
    _, c = orc.forward(p, Xc, cfg)
    dev = {'fb': p['feature_bias'][Xc][:, :, 0], 'Eo': p['outer_embeddings'][Xc], 'C': [r for r in c['rs']], 'pool': None}
    dev['inner_out'] = np.asarray(c['inner_out'], f32)
    D = cfg.D
    t1 = np.zeros((B, 2 * D - 2), f32)
    t1[:, :D] = bc.s0_stage(dev['Eo'], f32, order)[0]
    for l, C in enumerate(dev['C']):
        slot = l + 1
        if fault == 'pool_slot' and l < 2:        # the pool of layer l written to the slot of layer l + 1 (and back)
            slot = 2 - l
        v = bc.pool_stage(C, cfg.activation, f32, order)[0]
        o = bc._t1_off(D, slot)
        n = min(v.shape[1], D >> slot)
        t1[:, o:o + n] = v[:, :n]
    dev['t1'] = t1
    dev['h1'] = bc.dense_stage(t1, p['dense_1_kernel'], p['dense_1_bias'], f32, order)[0]
    dev['att'] = bc.att_stage(dev['fb'], p['bias_W'], p['bias_b'], cfg.lamda_att, f32, order, fault if fault == 'no_lamda' else None)[0]
    raw = bc.out_stage(dev['inner_out'], dev['h1'], dev['att'], dev['fb'], p, cfg, f32, order, fault)[0]
    dev['out'] = (f32(1) / (f32(1) + np.exp(-raw))).astype(f32) if loss == 'log_loss' else raw
    loss_stage(dev, y, loss, Bg, order, fault, unscaled)
    v, _, _ = bc.head_bwd_stage(dev['dout'], dev, p, cfg, f32, order)
    dev.update(v)
    return dev


def loss_stage(dev, y, loss, Bg, order='seq', fault=None, unscaled=False, B_dout=None):
    v, _ = bc.loss_stage(dev['out'], y, loss, Bg, f32, order, unscaled=unscaled, fault=fault)
    dev['sqerr'], dev['sum'], dev['L'] = v['sqerr'], v['sum'], v['L']
    L = dev['L']
    late = fault == 'late_scale'                 # the 1/L of the single-GPU route applied on the unscaled route as well
    if late:
        L = bc.loss_stage(dev['out'], y, loss, Bg, f32, order)[0]['L']
    d = bc.dout_stage(dev['out'], y, L, loss, Bg if B_dout is None else B_dout, f32, unscaled=unscaled and not late)[0]
    if fault == 'mse_no_2':
        d = d * f32(0.5)
    dev['dout'] = d.astype(f32)
    if unscaled:
        dev['L'] = f32(1)
        dev.pop('sum'), dev.pop('sqerr')


HEAD_CASES = ['selu-f10-k32', 'prelu-f5-k32-b300', 'elu-f28-k32']


# every shape in the three orders with square_loss; the other losses on one shape, sequential and reverse
HEAD_PARAMS = [(n, 'square_loss', o) for n in HEAD_CASES for o in ORDERS] + [('selu-f10-k32', l, o) for l in G.LOSSES[1:] for o in ('seq', 'rev')]


@pytest.mark.parametrize('name,loss,order', HEAD_PARAMS)
def test_head_float32_evaluations_pass(name, loss, order):
    cfg, p32, X, y = _case(name, loss=loss)
    st = bc.check_head(name, head_device(cfg, p32, X, y, loss, order), p32, cfg, loss, y=y)
    for k, v in st.items():
        if 'q_replay' in v:
            PASSING[(name, loss, order, k)] = _floor_ratio(v)
            print(name, loss, order, k, 'q %.3g q_replay %.3g hard %.3g' % (v['q'], v['q_replay'], v['hard']))
    if loss == 'hybrid':
        assert float(dev_out_min(cfg, p32, X)) > 0.05
    dev = head_device(cfg, p32, X, y, loss, order, B_global=3 * X.shape[0], unscaled=True)
    if loss not in ('hybrid', 'square_l2'):
        bc.check_head(name + ' unscaled', dev, p32, cfg, loss, y=y, B_global=3 * X.shape[0], unscaled=True)


FAULTS_HEAD = {     # fault -> (loss, tensor, tier)
    'pool_slot': ('square_loss', 't1 pool', 'hard'), 'no_lamda': ('square_loss', 'att', 'hard'), 'd2b_twice': ('square_loss', 'out', 'hard'),
    'no_beta': ('square_loss', 'out', 'hard'),
}


@pytest.mark.parametrize('fault', list(FAULTS_HEAD))
def test_head_faults_fail(fault):
    loss, tensor, tier = FAULTS_HEAD[fault]
    cfg, p32, X, y = _case('selu-f10-k32')
    cfg.beta_outer = 0.7                           # beta_outer = 1 would hide a dropped beta
    with pytest.raises(AssertionError) as e:
        bc.check_head(fault, head_device(cfg, p32, X, y, loss, 'seq', fault), p32, cfg, loss, y=y)
    assert any(tensor in ln and '[' + tier + ']' in ln for ln in str(e.value).splitlines()), (fault, str(e.value))


def _loss_inputs(loss, B=300):
    rng = np.random.default_rng(5)
    if loss == 'log_loss':                         # ws.out holds the sigmoid: logits from -8 to 8
        out = (1.0 / (1.0 + np.exp(-np.linspace(-8, 8, B)))).astype(f32)
    elif loss == 'hybrid':
        out = rng.uniform(0.02, 0.98, B).astype(f32)
    else:
        out = rng.standard_normal(B).astype(f32)
    y = rng.choice([0.0, 1.0] if loss in ('log_loss', 'hybrid') else [-1.0, 1.0], size=B).astype(f32)
    return out, y


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('loss', G.LOSSES)
def test_loss_stages_pass(loss, order):
    out, y = _loss_inputs(loss)
    for unscaled, Bg in ((False, 300), (True, 900)):
        if unscaled and loss in ('hybrid', 'square_l2'):
            continue
        dev = {'out': out}
        loss_stage(dev, y, loss, Bg, order, unscaled=unscaled)
        assert not _check_loss(dev, y, loss, Bg, unscaled, (loss, order, unscaled))


def dev_out_min(cfg, p32, X):
    out, _ = orc.forward({k: np.asarray(v, np.float64) for k, v in p32.items()}, G.clamp_ids(X, cfg.M), cfg)
    assert out.max() < 0.95
    return out.min()


def _check_loss(dev, y, loss, Bg, unscaled, record=None):
    """check_head's loss and dout tiers alone (no head gradients): returns the failure lines."""
    fails = []
    v, S = bc.loss_stage(dev['out'], y, loss, Bg, unscaled=unscaled)
    rep, _ = bc.loss_stage(dev['out'], y, loss, Bg, f32, unscaled=unscaled)
    B = y.shape[0]
    todo = [('dout', dev['dout'], bc.dout_stage(dev['out'], y, dev['L'], loss, Bg, unscaled=unscaled), 3, bc.C_DOUT, None)]
    if 'sqerr' in dev:
        todo += [('sqerr', dev['sqerr'], (v['sqerr'], S['sqerr']), 2, bc.C_LOSS, None),
                 ('loss sum', dev['sum'], (v['sum'], S['sum']), B, bc.C_LOSS, rep['sum']),
                 ('L', dev['L'], (v['L'], S['L']), B + 2, bc.C_LOSS + 3, rep['L'])]
    for k, got, (ref, s), n, c, r in todo:
        try:
            st = bc.check(k, got, ref, s, n, c, replay=r)
            if record is not None and 'q_replay' in st:
                PASSING[record + (k,)] = _floor_ratio(st)
        except AssertionError as e:
            fails += str(e).splitlines()
    return fails


FAULTS_LOSS = {     # fault -> (loss, unscaled, tensor)
    'local_batch': ('square_loss', False, 'dout'), 'mse_no_2': ('mse', False, 'dout'), 'no_eps': ('log_loss', False, 'sqerr'),
    'hybrid_norms': ('hybrid', False, 'L'), 'late_scale': ('square_loss', True, 'dout'),
}


@pytest.mark.parametrize('fault', list(FAULTS_LOSS))
def test_loss_faults_fail(fault):
    loss, unscaled, tensor = FAULTS_LOSS[fault]
    out, y = _loss_inputs(loss)
    Bg = 900 if (unscaled or fault == 'local_batch') else 300
    dev = {'out': out}
    loss_stage(dev, y, loss, Bg, 'seq', fault, unscaled, B_dout=300 if fault == 'local_batch' else None)
    fails = _check_loss(dev, y, loss, Bg, unscaled)
    assert any(ln.startswith(tensor + ' [') for ln in fails), (fault, fails)


def test_floor_gap():
    """Largest passing against smallest failing floor statistic, over every evaluation of this file (collected here again, so the
    test stands on its own)."""
    PASSING.clear()
    FAILING.clear()
    for n in CPU_CASES:
        for o in ORDERS:
            test_inner_float32_evaluations_pass(n, o)
    for n, f in INNER_FAULT_PARAMS:
        test_inner_faults_fail(n, f)
    for prm in HEAD_PARAMS:
        test_head_float32_evaluations_pass(*prm)
    for l in G.LOSSES:
        for o in ORDERS:
            test_loss_stages_pass(l, o)
    worst_pass, best_fail = max(PASSING.values()), min(FAILING.values())
    print('largest passing %.3g (%s), smallest failing %.3g (%s)' % (worst_pass, max(PASSING, key=PASSING.get), best_fail,
                                                                     min(FAILING, key=FAILING.get)))
    assert worst_pass <= 1.0 < best_fail and best_fail >= 3.0 * worst_pass
