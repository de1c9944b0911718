"""GPU: the inner branch and every stage of the head against float64 references of their own device inputs (oracle/branch_check.py).

Per case, on the same seeded inputs:
  product   eng.forward + eng.backward (the materialising route: inner_fwd / head_fwd, then the fused bwd_top launch where the shape
            takes it, else head_bwd + inner_bwd / inner_bwd_wide from ws.Ei)
  stage     cffm_inner_fwd (and cffm_gather_inner_fwd on the wide shapes), cffm_head_fwd, cffm_head_bwd, cffm_inner_bwd and
            cffm_reduce_slabs one at a time on the product workspace, every output poisoned beforehand
  unscaled  cffm_backward_unscaled: dL/dout = (out - y) / B_global without the 1/L (the data-parallel route, L left at 1)
  step      eng.train_step on a fresh engine: fwd_all + bwd_top (+ conv01_bwd) on the narrow shapes, gather_inner_fwd_wide +
            inner_bwd_wide from the tables on the wide ones with ws.Ei / ws.Eo poisoned; the workspace still holds every
            intermediate of the pre-update parameters
  packed    cffm_forward_packed / cffm_backward_unscaled_packed over records of stride K + D + 4 (two wide cases)
Every case names the kernel family it is there for; the test derives the family from (F, K, D) the way the dispatch does and asserts
it, so a dispatch change cannot silently empty a case.  tests/test_branch_check.py checks the ambiguity cap of every case on the CPU.
Every case prints its family, the ambiguous-unit count and, per tensor, the worst err / bound of the hard tier and q against q_replay;
CFFM_BRANCH_STATS=FILE appends the same lines to FILE."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cffm_amd.spec import CFFMConfig, init_params  # noqa: E402
from oracle import branch_check as bc  # noqa: E402

pytestmark = pytest.mark.gpu

# family: None = narrow (inner_fwd_body / inner_bwd_body; Pp <= 64), else (K2, UPT, 'generic' | 'circ') of
# gather_inner_fwd_wide_kernel; the backward of a wide case is inner_bwd_wide_kernel<K2, relu | -1>
CASES = {
    # narrow: the compiled-in activation of the README shapes (fwd_all / bwd_top / conv01_bwd), the generic-activation builds
    'frappe-f10-k32-b256-selu': dict(M=5382, F=10, K=32, D=32, act='selu', B=256, family=None),
    'mltag-f3-k32-b1024-elu': dict(M=90445, F=3, K=32, D=32, act='elu', B=1024, family=None),
    'bookx-f6-k32-b512-relu': dict(M=226336, F=6, K=32, D=32, act='relu', B=512, family=None),
    'f7-k16-b100-gelu': dict(M=600, F=7, K=16, D=32, act='gelu', B=100, family=None),
    'f5-k32-b200-prelu': dict(M=400, F=5, K=32, D=32, act='prelu', B=200, family=None),
    'f10-k32-b1-selu': dict(M=5382, F=10, K=32, D=32, act='selu', B=1, family=None),
    'f10-k32-b257-selu': dict(M=5382, F=10, K=32, D=32, act='selu', B=257, family=None),
    'f10-k32-b63-elu': dict(M=900, F=10, K=32, D=32, act='elu', B=63, family=None),
    'f10-k32-b64-elu': dict(M=900, F=10, K=32, D=32, act='elu', B=64, family=None, bad_ids=True),
    # wide: one relu and one non-relu case per reachable <K2, UPT> family; ragged last phase (B % 4 != 0), B < 4
    'f13-k64-b9-relu': dict(M=900, F=13, K=64, D=64, act='relu', B=9, family=(32, 4, 'generic')),
    'f13-k64-b6-gelu': dict(M=900, F=13, K=64, D=64, act='gelu', B=6, family=(32, 4, 'generic')),
    'f20-k64-b10-relu': dict(M=2000, F=20, K=64, D=64, act='relu', B=10, family=(32, 8, 'generic')),
    'f20-k64-b7-gelu': dict(M=2000, F=20, K=64, D=64, act='gelu', B=7, family=(32, 8, 'generic'), packed=True),
    'f28-k64-b6-relu': dict(M=2000, F=28, K=64, D=64, act='relu', B=6, family=(32, 16, 'generic')),
    'f28-k64-b3-elu': dict(M=2000, F=28, K=64, D=64, act='elu', B=3, family=(32, 16, 'generic')),
    'f28-k32-b13-relu': dict(M=2000, F=28, K=32, D=32, act='relu', B=13, family=(16, 8, 'generic')),
    'f28-k32-b10-elu': dict(M=2000, F=28, K=32, D=32, act='elu', B=10, family=(16, 8, 'generic'), packed=True, bad_ids=True),
    'f32-k32-b5-selu': dict(M=2000, F=32, K=32, D=32, act='selu', B=5, family=(16, 8, 'generic')),
    'f20-k32-b2-relu': dict(M=2000, F=20, K=32, D=32, act='relu', B=2, family=(16, 4, 'generic')),
    'f20-k32-b21-gelu': dict(M=2000, F=20, K=32, D=32, act='gelu', B=21, family=(16, 4, 'generic')),
    # more examples than slabs (small_slabs(B) = 1024 < B): inner_bwd_wide_kernel walks b = slab, slab + 1024
    'f12-k32-b1030-prelu': dict(M=3000, F=12, K=32, D=32, act='prelu', B=1030, family=(16, 4, 'generic')),
    'f32-k64-b14-relu': dict(M=3000, F=32, K=64, D=64, act='relu', B=14, family=(32, 16, 'circ')),
    'f32-k64-b7-selu': dict(M=3000, F=32, K=64, D=64, act='selu', B=7, family=(32, 16, 'circ')),
    # tie rows: every other example pairs rows with e[2t] == e[2t+1]: x0 == x1 exactly, non-zero gradient, first-on-tie decides dEi
    'tie-f6-k32-b64-elu': dict(M=700, F=6, K=32, D=32, act='elu', B=64, family=None, tie=True),
    'tie-f6-k32-b64-selu': dict(M=700, F=6, K=32, D=32, act='selu', B=64, family=None, tie=True),
    'tie-f7-k16-b40-gelu': dict(M=700, F=7, K=16, D=32, act='gelu', B=40, family=None, tie=True),
    'tie-f20-k64-b6-elu': dict(M=700, F=20, K=64, D=64, act='elu', B=6, family=(32, 8, 'generic'), tie=True),
    'tie-f28-k32-b6-gelu': dict(M=700, F=28, K=32, D=32, act='gelu', B=6, family=(16, 8, 'generic'), tie=True),
    'tie-f32-k64-b5-selu': dict(M=700, F=32, K=64, D=64, act='selu', B=5, family=(32, 16, 'circ'), tie=True),
    # unit probes: dense_kernel zero except one entry, dense_bias 0: inner_out[b] IS that unit's s value times one weight
    'probe-first-f10-selu': dict(M=900, F=10, K=32, D=32, act='selu', B=16, family=None, probe=(0, 0, 0)),
    'probe-last-f10-selu': dict(M=900, F=10, K=32, D=32, act='selu', B=16, family=None, probe=(44, 15, 1)),
    'probe-last-f20-k64-gelu': dict(M=900, F=20, K=64, D=64, act='gelu', B=6, family=(32, 8, 'generic'), probe=(189, 31, 1)),
    # the last unit of a thread group: p = UPT * g + UPT - 1
    'probe-group-f20-k64-relu': dict(M=900, F=20, K=64, D=64, act='relu', B=6, family=(32, 8, 'generic'), probe=(8 * 3 + 7, 5, 0)),
    'probe-group-f28-k32-elu': dict(M=900, F=28, K=32, D=32, act='elu', B=6, family=(16, 8, 'generic'), probe=(8 * 40 + 7, 15, 1)),
    'probe-last-f32-k64-relu': dict(M=900, F=32, K=64, D=64, act='relu', B=5, family=(32, 16, 'circ'), probe=(495, 31, 1)),
    # pair {3, 19} sits on the circulant diameter d = 16: p = 3 * (64 - 3 - 1) / 2 + (19 - 3 - 1)
    'probe-diam-f32-k64-selu': dict(M=900, F=32, K=64, D=64, act='selu', B=5, family=(32, 16, 'circ'), probe=(3 * 60 // 2 + 15, 9, 0)),
    # disabled branches and the plain first-order term
    'no-inner-f6-elu': dict(M=700, F=6, K=32, D=32, act='elu', B=33, family=None, inner_conv=0),
    'no-outer-f6-selu': dict(M=700, F=6, K=32, D=32, act='selu', B=33, family=None, outer_conv=0),
    'nolinatt-f10-gelu': dict(M=700, F=10, K=32, D=32, act='gelu', B=40, family=None, linear_att=0),
    # the K and F edges of the accepted domain ("Shape domain"), all on inner_fwd_body / inner_bwd_body.  K no power of two,
    # very small or large: the unit split p = u / K2, t = u % K2 (fast_div) and the 16-byte pieces of a row
    'k4-f3-b9-prelu': dict(M=400, F=3, K=4, D=32, act='prelu', B=9, family=None),
    'k12-f7-b40-gelu': dict(M=600, F=7, K=12, D=32, act='gelu', B=40, family=None),
    'k20-f10-b33-selu': dict(M=900, F=10, K=20, D=32, act='selu', B=33, family=None, bad_ids=True),
    'tie-k36-f6-b64-elu': dict(M=700, F=6, K=36, D=32, act='elu', B=64, family=None, tie=True),
    'k100-f5-b17-relu': dict(M=400, F=5, K=100, D=32, act='relu', B=17, family=None),
    'probe-last-f10-k128-selu': dict(M=900, F=10, K=128, D=32, act='selu', B=6, family=None, probe=(44, 63, 1)),
    # F > 32: K == D in {32, 64} no longer takes the non-materialising route (cffm_wide_regather_ok wants F <= 32); the LDS of
    # inner_bwd_body (5 F K floats) at its largest in the suite; F = CFFM_MAX_FIELDS with P = 2016 pairs
    'f34-k32-d32-b3-relu': dict(M=2000, F=34, K=32, D=32, act='relu', B=3, family=None),
    'f40-k64-d8-b3-elu': dict(M=2000, F=40, K=64, D=8, act='elu', B=3, family=None),
    'f64-k8-d4-b3-gelu': dict(M=2000, F=64, K=8, D=4, act='gelu', B=3, family=None),
}
LOSSES = ('square_loss', 'mse', 'mae', 'log_loss', 'hybrid', 'square_l2')
for _l in LOSSES[1:]:
    CASES['loss-%s-f10-selu' % _l] = dict(M=900, F=10, K=32, D=32, act='selu', B=48, family=None, loss=_l)
    CASES['loss-%s-f20-k32-elu' % _l] = dict(M=900, F=20, K=32, D=32, act='elu', B=9, family=(16, 4, 'generic'), loss=_l)


def giw_family(F, K, D):
    """(K2, UPT, kind) of gather_inner_fwd_wide_kernel for a shape as cffm_gather_inner_fwd_wide picks it, None for the shapes the
    non-materialising route does not take (cffm_wide_regather_ok: Pp > 64, K == D in {32, 64}, F <= 32)."""
    P = F * (F - 1) // 2
    Pp = (P + 15) // 16 * 16
    if not (Pp > 64 and K == D and K in (32, 64) and F <= 32):
        return None
    K2 = K // 2
    upt = -(-P // (1024 // K2))
    return (K2, 4 if upt <= 4 else (8 if upt <= 8 else 16), 'circ' if (F == 32 and K == 64) else 'generic')


def make_branch_case(name, seed=0):
    c = CASES[name]
    loss = c.get('loss', 'square_loss')
    cfg = CFFMConfig(M=c['M'], F=c['F'], K=c['K'], D=c['D'], activation=c['act'], lamda_att=1.3, linear_att=c.get('linear_att', 1),
                     inner_conv=c.get('inner_conv', 1), outer_conv=c.get('outer_conv', 1),
                     loss_type='square_loss' if loss == 'square_l2' else loss, lamda_bilinear=0.01 if loss == 'square_l2' else 0.0)
    p32 = init_params(cfg, seed=seed, dtype=np.float32)
    rng = np.random.default_rng(seed + 7)
    scaled = loss != 'hybrid'          # hybrid takes log(out): 0 < out < 1 needs the small initial tables and bias = 0.5
    p32['feature_bias'] = (rng.standard_normal(p32['feature_bias'].shape) * (0.3 if scaled else 0.03)).astype(np.float32)
    if scaled:
        p32['outer_embeddings'] = (p32['outer_embeddings'] * 20.0).astype(np.float32)
        p32['inner_embeddings'] = (p32['inner_embeddings'] * 4.0).astype(np.float32)
    # every bias non-zero and of either sign: a bias that is left out or added twice must show
    p32['inner_layer_conv_bias_0'] = np.asarray([0.03, -0.02], np.float32)
    p32['dense_bias'] = np.asarray([0.05], np.float32)
    p32['dense_2_bias'] = np.asarray([-0.04], np.float32)
    p32['dense_3_bias'] = np.asarray([0.02], np.float32)
    p32['bias_b'] = (rng.standard_normal(p32['bias_b'].shape) * 0.1).astype(np.float32)
    p32['bias'] = np.float32(0.5 if loss == 'hybrid' else 0.01)
    if loss == 'hybrid':               # the pools of 2D - 2 rows add up to hundreds: keep the outer branch's share of out small
        p32['dense_2_kernel'] = (p32['dense_2_kernel'] * 1e-4).astype(np.float32)
    B, F, K = c['B'], cfg.F, cfg.K
    X = rng.integers(0, cfg.M, size=(B, F)).astype(np.int32)
    if c.get('tie'):
        rows = np.arange(0, cfg.M, 5)
        p32['inner_embeddings'][rows, 1::2] = p32['inner_embeddings'][rows, 0::2]
        X[0::2] = rows[rng.integers(0, rows.size, size=X[0::2].shape)]
    if c.get('probe'):
        p, t, ch = c['probe']
        dk = np.zeros((cfg.P, K // 2, 2), np.float32)
        dk[p, t, ch] = 0.7
        p32['dense_kernel'] = dk.reshape(-1, 1)
        p32['dense_bias'] = np.zeros(1, np.float32)
    if c.get('bad_ids'):
        X[0, 0], X[B // 2, F - 1], X[B - 1, 1] = -3, cfg.M, cfg.M + 77
    y = rng.choice([-1.0, 1.0], size=(B,)).astype(np.float32)
    if loss in ('log_loss', 'hybrid'):
        y = (y > 0).astype(np.float32)
    return cfg, p32, X, y


def clamp_ids(X, M):
    return np.clip(X, 0, M - 1)


def inner_inputs(cfg, p32, X):
    return (p32['inner_embeddings'][clamp_ids(X, cfg.M)], p32['inner_layer_conv_weight_0'].reshape(-1), p32['inner_layer_conv_bias_0'],
            p32['dense_kernel'].reshape(-1), p32['dense_bias'])


# ---- reading the device ------------------------------------------------------------------------------------------------------
HEAD_GRADS = ('bias', 'bias_W', 'bias_b', 'dense_1_kernel', 'dense_1_bias', 'dense_2_kernel', 'dense_2_bias', 'dense_3_kernel',
              'dense_3_bias')
INNER_GRADS = ('inner_layer_conv_weight_0', 'inner_layer_conv_bias_0', 'dense_kernel', 'dense_bias')
POOL_SAMPLE = 1 << 23          # elements of one conv output above which the pools are checked on the first 8 examples only


def collect(eng, cfg, B, grads):
    """The device tensors of the last forward + backward as numpy arrays, keyed as branch_check.check_head / check_inner name them."""
    g = lambda m, shape, **kw: eng.ws_tensor(B, m, shape, **kw).cpu().numpy()
    D, F, P, Pp = cfg.D, cfg.F, cfg.P, eng.tl.Pp
    _, wl = eng.workspace(B)
    dev = {'fb': g('fb', (B, F)), 'out': g('out', (B,)), 'sqerr': g('sqerr', (B,))}
    sc = g('scalars', (16,))
    dev['sum'], dev['L'] = sc[0], sc[1]
    if cfg.inner_conv:
        dev['inner_out'] = g('inner_out', (B,))
    if cfg.linear_att:
        dev['att'] = g('att', (B, F))
    if cfg.outer_conv:
        dev['t1'], dev['h1'] = g('t1', (B, 2 * D - 2)), g('h1', (B, 32))
        dev['C'], dev['pool'], dev['n_pool'] = [], [], B
        for l in range(cfg.live_layers):
            S = D >> (l + 1)
            if B * S * S * P > POOL_SAMPLE:
                dev['n_pool'] = min(B, 8)
        for l in range(cfg.live_layers):
            S, nb = D >> (l + 1), dev['n_pool']
            dev['C'].append(eng.ws_tensor(B, 'C', (B, S, S, Pp), index=l)[:nb, ..., :P].cpu().numpy())
            npl = int(wl.pool_np[l])
            dev['pool'].append(eng.ws_tensor(B, 'pool', (B, S, npl), index=l)[:nb].cpu().numpy() if npl > 0 else None)
    dev['dout'], dev['dfb'] = g('dout', (B,)), g('dfb', (B, F))
    if cfg.outer_conv:
        dev['dt1'] = g('dt1', (B, 2 * D - 2))
    if cfg.inner_conv:
        dev['dEi'] = g('dEi', (B, F, cfg.K))
    for k in HEAD_GRADS + INNER_GRADS:
        dev[k] = np.asarray(grads[k], np.float32).reshape(-1) if k in INNER_GRADS else np.asarray(grads[k], np.float32)
    return dev


def check_case(path, dev, cfg, p32, X, y, loss, report, fails, B_global=None, unscaled=False, Eo=None):
    """Inner branch and head of one path; appends to report (lines) and fails (messages)."""
    B = X.shape[0]
    Xc = clamp_ids(X, cfg.M)
    np.testing.assert_array_equal(dev['fb'], p32['feature_bias'][Xc][:, :, 0], err_msg=path + ': fb is not a copy of the table rows')
    stats = {}
    if cfg.inner_conv:
        got = {k: dev[k] for k in bc.INNER_TERMS if k in dev}
        try:
            bc.check_inner(path, got, *inner_inputs(cfg, p32, X), cfg.activation, dout=dev.get('dout'), sink=stats)
        except AssertionError as e:
            fails.append(str(e))
    else:
        for k in INNER_GRADS:
            assert not np.any(dev[k]), '%s: gradient of %s is not 0 with the inner branch disabled' % (path, k)
    hd = dict(dev)
    if cfg.outer_conv:
        if Eo is not None:
            hd['Eo'] = Eo
        nb = dev['n_pool']
        if nb < B:                 # pools of the first nb examples only (the conv outputs of the rest were not copied)
            try:
                bc.check_head(path + ' (first %d)' % nb, dict(t1=dev['t1'][:nb], C=dev['C'], pool=dev['pool']), p32, cfg, loss, sink=stats)
            except AssertionError as e:
                fails.append(str(e))
            hd.pop('C'), hd.pop('pool')
    else:
        for k in ('dense_1_kernel', 'dense_1_bias', 'dense_2_kernel', 'dense_2_bias'):
            assert not np.any(dev[k]), '%s: gradient of %s is not 0 with the outer branch disabled' % (path, k)
    if not cfg.linear_att:
        for k in ('bias_W', 'bias_b', 'dense_3_kernel', 'dense_3_bias'):
            assert not np.any(dev[k]), '%s: gradient of %s is not 0 without the attention term' % (path, k)
    try:
        bc.check_head(path, hd, p32, cfg, loss, y=y, B_global=B_global, unscaled=unscaled, sink=stats)
    except AssertionError as e:
        fails.append(str(e))
    report.append('%s: ambiguous units %s of %s' % (path, stats.get('ambiguous', '-'), stats.get('units', '-')))
    for k, st in stats.items():
        if isinstance(st, dict) and 'hard' in st:
            report.append('  %-36s hard %-9.3g q %-9.3g%s' % (k, st['hard'], st['q'], 'q_replay %.3g' % st['q_replay'] if 'q_replay' in st else ''))
    return stats


def flat_grads(eng, flat):
    z = torch.zeros(1, device=eng.device)
    return eng._export(flat, z, z, z)


def _poison(eng, B, members):
    for m, shape in members:
        eng.ws_tensor(B, m, shape).fill_(float('nan'))


def run_case(name, report, fails):
    from cffm_amd import hip
    from cffm_amd.engine import HipEngine
    c = CASES[name]
    cfg, p32, X, y = make_branch_case(name)
    loss = c.get('loss', 'square_loss')
    B, F, K, D = X.shape[0], cfg.F, cfg.K, cfg.D
    fam = giw_family(F, K, D) if (cfg.inner_conv and cfg.outer_conv) else None
    assert fam == c['family'], '%s: the shape now dispatches to %s, the case is there for %s' % (name, fam, c['family'])
    eng = HipEngine(cfg, params=p32)
    assert eng.gather_inner_fwd_ok() == (fam is not None), name
    report.append('%s: gather_inner_fwd_wide family %s, inner backward %s' % (
        name, fam, 'inner_bwd_body' if fam is None else 'inner_bwd_wide_kernel<%d, %s>' % (fam[0], 'relu' if cfg.activation == 'relu' else '-1')))
    ids, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    Xc = clamp_ids(X, cfg.M)
    Eo = p32['outer_embeddings'][Xc]
    members = [('inner_out', (B,)), ('t1', (B, 2 * D - 2)), ('h1', (B, 32)), ('att', (B, F)), ('out', (B,)), ('sqerr', (B,)),
               ('dout', (B,)), ('dt1', (B, 2 * D - 2)), ('dEi', (B, F, K)), ('dfb', (B, F))]
    # ---- product: forward + backward --------------------------------------------------------------------------------------
    eng.workspace(B)
    _poison(eng, B, members)
    eng.forward(ids, yt)
    eng.backward(yt, B)
    torch.cuda.synchronize()
    if cfg.inner_conv:
        np.testing.assert_array_equal(eng.ws_tensor(B, 'Ei', (B, F, K)).cpu().numpy(), p32['inner_embeddings'][Xc])
    if cfg.outer_conv:
        np.testing.assert_array_equal(eng.ws_tensor(B, 'Eo', (B, F, D)).cpu().numpy(), Eo)
    check_case('product', collect(eng, cfg, B, eng.export_grad()), cfg, p32, X, y, loss, report, fails, Eo=Eo)
    # ---- stage: one entry point at a time on the same workspace -------------------------------------------------------------
    buf, wl = eng.workspace(B)
    lib, s, th, st = eng.lib, eng._s, eng.theta.data_ptr(), eng._stream()
    _poison(eng, B, members)
    if fam is not None:
        eng.ws_tensor(B, 'sort_keys', (B * F,), dtype=torch.int64).fill_(-1)
        eng.gather_inner_fwd(ids)                   # inner_out, t1[:, :D], fb, keys; cffm_inner_fwd below redoes inner_out from ws.Ei
        torch.cuda.synchronize()
        st_g = {}
        try:
            bc.check_inner('stage gather_inner_fwd', {'inner_out': eng.ws_tensor(B, 'inner_out', (B,)).cpu().numpy()},
                           *inner_inputs(cfg, p32, X), cfg.activation, sink=st_g)
            bc.check_head('stage gather_inner_fwd', dict(t1=eng.ws_tensor(B, 't1', (B, 2 * D - 2)).cpu().numpy(), Eo=Eo), p32, cfg, loss,
                          sink=st_g)
        except AssertionError as e:
            fails.append(str(e))
        report.append('stage gather_inner_fwd: inner_out q %.3g (q_replay %.3g), s0 hard %.3g' % (
            st_g.get('inner_out', {}).get('q', -1), st_g.get('inner_out', {}).get('q_replay', -1), st_g.get('t1 s0', {}).get('hard', -1)))
        np.testing.assert_array_equal(eng.ws_tensor(B, 'fb', (B, F)).cpu().numpy(), p32['feature_bias'][Xc][:, :, 0])
        keys = eng.ws_tensor(B, 'sort_keys', (B * F,), dtype=torch.int64).cpu().numpy()
        np.testing.assert_array_equal(keys >> 32, np.where((X < 0) | (X >= cfg.M), cfg.M, X).reshape(-1))     # a bad id: key M
        np.testing.assert_array_equal(keys & 0xffffffff, np.arange(B * F))
        eng.ws_tensor(B, 'inner_out', (B,)).fill_(float('nan'))
    hip.check(lib.cffm_inner_fwd(s, th, buf.data_ptr(), B, st))
    hip.check(lib.cffm_head_fwd(s, th, buf.data_ptr(), yt.data_ptr(), B, st))
    hip.check(lib.cffm_head_bwd(s, th, buf.data_ptr(), yt.data_ptr(), B, B, st))
    hip.check(lib.cffm_inner_bwd(s, th, buf.data_ptr(), B, st))
    flat = torch.full((int(eng.tl.n),), float('nan'), dtype=torch.float32, device=eng.device)
    hip.check(lib.cffm_reduce_slabs(s, buf.data_ptr(), B, flat.data_ptr(), st))
    torch.cuda.synchronize()
    check_case('stage', collect(eng, cfg, B, flat_grads(eng, flat)), cfg, p32, X, y, loss, report, fails, Eo=Eo)
    # ---- the data-parallel dout: dL/dout = (out - y) / B_global without the 1/L, L left at 1 ---------------------------------------
    if loss not in ('hybrid', 'square_l2'):
        _poison(eng, B, members[6:])
        eng.backward_unscaled(ids, yt, B, 3 * B, pack=False)
        torch.cuda.synchronize()
        dev = collect(eng, cfg, B, flat_grads(eng, eng._grad_full[:int(eng.tl.n)]))
        dev.pop('sum'), dev.pop('sqerr')            # the unscaled route leaves the loss to the caller's all-reduce
        dev['L'] = np.float32(1.0)
        check_case('unscaled', dev, cfg, p32, X, y, loss, report, fails, B_global=3 * B, unscaled=True, Eo=Eo)
    del eng
    # ---- step: the fused / non-materialising launches of train_step ------------------------------------------------------------
    if loss != 'square_l2' or (cfg.inner_conv and cfg.outer_conv):
        eng2 = HipEngine(cfg, params=p32)
        eng2.workspace(B)
        _poison(eng2, B, members)
        if fam is not None:
            eng2.ws_tensor(B, 'Ei', (B, F, K)).fill_(float('nan'))
            eng2.ws_tensor(B, 'Eo', (B, F, D)).fill_(float('nan'))
        eng2.train_step(ids, yt)
        torch.cuda.synchronize()
        if fam is not None and loss != 'square_l2':
            assert bool(torch.isnan(eng2.ws_tensor(B, 'Ei', (B, F, K))).all()) and bool(torch.isnan(eng2.ws_tensor(B, 'Eo', (B, F, D))).all()), \
                'the non-materialising route wrote ws.Ei / ws.Eo'
        dev = collect(eng2, cfg, B, flat_grads(eng2, eng2.grad))
        if loss == 'hybrid':
            dev.pop('sum')          # the fused step's scalars[0] is the first of the hybrid loss's two sums, not the sum of ws.sqerr
        check_case('step', dev, cfg, p32, X, y, loss, report, fails, Eo=Eo)
        del eng2
    # ---- the row-sharded step's packed records (stride K + D + 4) --------------------------------------------------------------
    if c.get('packed'):
        eng3 = HipEngine(cfg, params=p32)
        uniq, inv = np.unique(Xc.reshape(-1), return_inverse=True)
        packed = eng3.gather_packed(torch.from_numpy(uniq.astype(np.int32)).cuda())
        assert packed.shape[1] == K + D + 4
        pos = torch.from_numpy(inv.reshape(-1).astype(np.int32)).cuda()
        eng3.workspace(B)
        _poison(eng3, B, members + [('Ei', (B, F, K)), ('Eo', (B, F, D))])
        eng3.forward_packed(packed, pos, yt, B)
        gf = eng3.backward_unscaled_packed(packed, pos, yt, B, 2 * B)
        torch.cuda.synchronize()
        assert bool(torch.isnan(eng3.ws_tensor(B, 'Ei', (B, F, K))).all()) and bool(torch.isnan(eng3.ws_tensor(B, 'Eo', (B, F, D))).all())
        dev = collect(eng3, cfg, B, flat_grads(eng3, gf[:int(eng3.tl.n)]))
        dev.pop('sum'), dev.pop('sqerr')
        dev['L'] = np.float32(1.0)
        check_case('packed', dev, cfg, p32, Xc, y, loss, report, fails, B_global=2 * B, unscaled=True, Eo=Eo)
        del eng3
    torch.cuda.empty_cache()


@pytest.mark.parametrize('name', list(CASES))
def test_branches(name):
    report, fails = [], []
    try:
        run_case(name, report, fails)
    finally:
        print('\n'.join(report))
        path = os.environ.get('CFFM_BRANCH_STATS')
        if path:
            with open(path, 'a') as fh:
                fh.write('\n'.join(report) + '\n')
    assert not fails, '\n'.join(fails)
