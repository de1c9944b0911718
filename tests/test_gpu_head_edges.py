"""GPU: the head alone at the D and F edges of the accepted shape domain ("Shape domain"), no conv or inner-branch launch.

The test writes every input of the head into the workspace itself, from seeded host data: ws.Eo, ws.fb, ws.inner_out, every ws.C[l]
(non-negative, about a third exact zeros, pad channels 0) and, where the layout has them (ws_layout.pool_np[l] > 0), the pool partials
ws.pool[l] of that C[l].  Every output is poisoned with NaN.  Then only cffm_head_fwd, cffm_head_bwd and cffm_reduce_slabs run, and
oracle/branch_check.check_head holds t1, h1, att, out, sqerr, the loss scalars, dout, dt1, dfb and the nine head gradients to the
float64 evaluation of those inputs, with the tiers and constants the whole-model cases of tests/test_gpu_branches.py use.  dC of the
top layer is checked here: its exact zeros against Ctop == 0, its values against dt1 * act'(Ctop).

What each case is there for is in CASES; the sizes are the smallest that reach the path (B <= 5)."""
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
from tests.test_gpu_branches import HEAD_GRADS, LOSSES, flat_grads  # noqa: E402

pytestmark = pytest.mark.gpu

HEAD_KPP = 16            # head_body.hpp: dense(32) rows a thread preloads; beyond it (D >= 128) the kernel loops over global memory

CASES = {
    # kpp = (2 D - 2 + 7) / 8 = 32 > HEAD_KPP: the dense(32) loop that is not preloaded
    'd128-f3-b5-gelu': dict(D=128, F=3, B=5, act='gelu'),
    # P = 1 (one pair), seven layers
    'd256-f2-b3-selu': dict(D=256, F=2, B=3, act='selu'),
    # t1w = 1022 of the 1024 floats of t1s / dt1s, live = 8 = CFFM_MAX_LAYERS: every [CFFM_MAX_LAYERS] array full, eight terms in off_top
    'd512-f2-b2-relu': dict(D=512, F=2, B=2, act='relu'),
    # the softmax and its backward over all 64 lanes of the wavefront; live = 1
    'd4-f64-b5-elu': dict(D=4, F=64, B=5, act='elu'),
    # one idle lane
    'd4-f63-b5-selu': dict(D=4, F=63, B=5, act='selu'),
    # the first F above the tiled range of layer 0
    'd8-f34-b3-relu': dict(D=8, F=34, B=3, act='relu'),
    # outer_conv = 0: the first-order term and the inner branch's output only
    'd32-f64-b2-selu-no-outer': dict(D=32, F=64, B=2, act='selu', outer_conv=0),
    # wide filters: the pools of layers whose conv epilogue leaves partials are read from ws.pool
    'd128-f20-b2-elu': dict(D=128, F=20, B=2, act='elu'),
    # F D + F F = 15,120 > 15,032: the forward asks for more than the default 64 KB of dynamic LDS (set_lds), first F that does at D = 512
    'd512-f28-b1-relu': dict(D=512, F=28, B=1, act='relu'),
}
for _l in LOSSES:
    CASES['loss-%s-d128-f3' % _l] = dict(D=128, F=3, B=5, act='selu', loss=_l)


def make_head_case(name, seed=0):
    c = CASES[name]
    loss = c.get('loss', 'square_loss')
    cfg = CFFMConfig(M=50, F=c['F'], K=4, D=c['D'], activation=c['act'], lamda_att=1.3, outer_conv=c.get('outer_conv', 1),
                     loss_type='square_loss' if loss == 'square_l2' else loss, lamda_bilinear=0.01 if loss == 'square_l2' else 0.0)
    p32 = init_params(cfg, seed=seed, dtype=np.float32)
    rng = np.random.default_rng(seed + 11)
    small = loss == 'hybrid'             # hybrid takes log(out) and log(1 - out): 0 < out < 1
    p32['bias_b'] = (rng.standard_normal(p32['bias_b'].shape) * 0.1).astype(np.float32)
    p32['dense_2_bias'] = np.asarray([-0.04], np.float32)
    p32['dense_3_bias'] = np.asarray([0.02], np.float32)
    p32['bias'] = np.float32(0.5 if small else 0.01)
    B, F, D, P = c['B'], cfg.F, cfg.D, cfg.P
    inp = {'fb': (rng.standard_normal((B, F)) * (0.03 if small else 0.3)).astype(np.float32),
           'inner_out': (rng.standard_normal(B) * (0.01 if small else 0.4)).astype(np.float32),
           'Eo': (rng.standard_normal((B, F, D)) * 0.2).astype(np.float32), 'C': []}
    for l in range(cfg.live_layers):
        S = D >> (l + 1)
        v = np.abs(rng.standard_normal((B, S, S, P))).astype(np.float32) * np.float32(0.1)
        v[rng.random(v.shape) < 1.0 / 3.0] = 0.0
        inp['C'].append(v)
    y = rng.choice([-1.0, 1.0], size=(B,)).astype(np.float32)
    if loss in ('log_loss', 'hybrid'):
        y = (y > 0).astype(np.float32)
    if small and cfg.outer_conv:         # keep the outer branch's share of out within +- 0.1
        t1 = np.concatenate([bc.s0_stage(inp['Eo'])[0]] + [bc.pool_stage(v, cfg.activation)[0] for v in inp['C']], axis=1)
        h1 = bc.dense_stage(t1.astype(np.float32), p32['dense_1_kernel'], p32['dense_1_bias'])[0]
        o = h1 @ np.asarray(p32['dense_2_kernel'], np.float64).reshape(-1)
        p32['dense_2_kernel'] = (p32['dense_2_kernel'] * (0.1 / max(np.abs(o).max(), 1e-30))).astype(np.float32)
    return cfg, p32, inp, y, loss


def pool_partials(C, kind, n_part):
    """[B, S, n_part] float32 partial sums of act(C[b, y]) over n_part consecutive chunks of the (x, channel) elements of a row: what a
    conv epilogue leaves in ws.pool[l].  The head adds the n_part partials of a row in index order, whichever elements each holds."""
    a = bc.act_model(C, kind)[0]
    B, S = a.shape[:2]
    a = a.reshape(B, S, -1)
    edges = np.linspace(0, a.shape[-1], n_part + 1).astype(int)
    return np.stack([a[..., edges[k]:edges[k + 1]].sum(-1) for k in range(n_part)], axis=-1).astype(np.float32)


def run_case(name, report):
    from cffm_amd import hip
    from cffm_amd.engine import HipEngine
    cfg, p32, inp, y, loss = make_head_case(name)
    B, F, D, P, live = y.shape[0], cfg.F, cfg.D, cfg.P, cfg.live_layers
    t1w = 2 * D - 2
    assert ((t1w + 7) // 8 > HEAD_KPP) == (D >= 128)
    assert (name == 'd512-f28-b1-relu') == ((1348 + F * D + F * F) * 4 + 16 > 64 * 1024), 'which case passes 64 KB of LDS changed'
    eng = HipEngine(cfg, params=p32)
    buf, wl = eng.workspace(B)
    Pp = eng.tl.Pp
    put = lambda m, shape, v, **kw: eng.ws_tensor(B, m, shape, **kw).copy_(torch.from_numpy(np.ascontiguousarray(v)))
    eng.ws_tensor(B, 'gpart', (int(wl.gpart_floats),)).zero_()           # the slabs no launch of this test writes read as zeros
    put('fb', (B, F), inp['fb'])
    put('inner_out', (B,), inp['inner_out'])
    put('Eo', (B, F, D), inp['Eo'])
    n_from_pool = 0
    for l in range(live):
        S = D >> (l + 1)
        Cp = np.zeros((B, S, S, Pp), np.float32)
        Cp[..., :P] = inp['C'][l]
        put('C', (B, S, S, Pp), Cp, index=l)
        npl = int(wl.pool_np[l])
        if npl > 0 and cfg.outer_conv:
            put('pool', (B, S, npl), pool_partials(inp['C'][l], cfg.activation, npl), index=l)
            n_from_pool += 1
    if name == 'd128-f20-b2-elu':
        assert n_from_pool > 0, 'no layer of this shape leaves pool partials any more: the case no longer reaches that loop'
    outs = [('t1', (B, t1w)), ('h1', (B, 32)), ('att', (B, F)), ('out', (B,)), ('sqerr', (B,)), ('dout', (B,)), ('dt1', (B, t1w)),
            ('dfb', (B, F)), ('scalars', (16,))]
    for m, shape in outs:
        eng.ws_tensor(B, m, shape).fill_(float('nan'))
    top = live - 1
    eng.ws_tensor(B, 'dC', (B, 2, 2, Pp), index=top).fill_(float('nan'))
    yt = torch.from_numpy(y).cuda()
    lib, s, th, st = eng.lib, eng._s, eng.theta.data_ptr(), eng._stream()
    hip.check(lib.cffm_head_fwd(s, th, buf.data_ptr(), yt.data_ptr(), B, st))
    hip.check(lib.cffm_head_bwd(s, th, buf.data_ptr(), yt.data_ptr(), B, B, st))
    flat = torch.full((int(eng.tl.n),), float('nan'), dtype=torch.float32, device=eng.device)
    hip.check(lib.cffm_reduce_slabs(s, buf.data_ptr(), B, flat.data_ptr(), st))
    torch.cuda.synchronize()
    g = lambda m, shape, **kw: eng.ws_tensor(B, m, shape, **kw).cpu().numpy()
    dev = {'fb': inp['fb'], 'inner_out': inp['inner_out'], 'out': g('out', (B,)), 'sqerr': g('sqerr', (B,)), 'att': g('att', (B, F)),
           'dout': g('dout', (B,)), 'dfb': g('dfb', (B, F))}
    sc = g('scalars', (16,))
    dev['sum'], dev['L'] = sc[0], sc[1]
    if cfg.outer_conv:
        dev.update(Eo=inp['Eo'], C=inp['C'], t1=g('t1', (B, t1w)), h1=g('h1', (B, 32)), dt1=g('dt1', (B, t1w)))
    grads = flat_grads(eng, flat)
    for k in HEAD_GRADS:
        dev[k] = np.asarray(grads[k], np.float32)
    stats, fails = {}, []
    try:
        bc.check_head(name, dev, p32, cfg, loss, y=y, sink=stats)
    except AssertionError as e:
        fails.append(str(e))
    if cfg.outer_conv:
        expect = {'t1 s0', 'h1', 'dt1', 'grad dense_1_kernel', 'grad dense_2_kernel'} | {'t1 pool %d' % (l + 1) for l in range(live)}
        assert expect <= set(stats), sorted(expect - set(stats))
        # dC of the top layer [B, 2, 2, Pp]: only its sum pool feeds the head, dCtop = dt1[off_top + y] * act'(Ctop), 0 where Ctop is 0
        dC = g('dC', (B, 2, 2, Pp), index=top)
        Ctop = inp['C'][top]
        assert np.isfinite(dC).all() and not dC[..., P:].any(), 'pad channels of dC[top]'
        off_top = sum(D >> i for i in range(live))
        assert off_top + 2 == t1w
        d = dev['dt1'][:, off_top:off_top + 2].astype(np.float64)[:, :, None, None]
        assert d.all(), 'a dt1 of exactly 0 would hide the zero pattern'
        np.testing.assert_array_equal(dC[..., :P] == 0, Ctop == 0, err_msg='zero pattern of dC[top] against Ctop == 0')
        _, gr, _, grs, _ = bc.act_model(Ctop, cfg.activation)
        on = Ctop > 0
        try:
            stats['dCtop'] = bc.check(name + ' dCtop', dC[..., :P], np.where(on, d * gr, 0.0), np.where(on, np.abs(d) * grs, 0.0), 1,
                                      bc.C_DCTOP)
        except AssertionError as e:
            fails.append(str(e))
    else:
        assert {'att', 'out', 'dfb', 'grad bias_W'} <= set(stats)
        for k in ('dense_1_kernel', 'dense_1_bias', 'dense_2_kernel', 'dense_2_bias'):
            assert not np.any(dev[k]), 'gradient of %s is not 0 with the outer branch disabled' % k
    for k, stt in stats.items():
        if isinstance(stt, dict) and 'hard' in stt:
            report.append('  %-28s hard %-9.3g q %-9.3g%s' % (k, stt['hard'], stt['q'], 'q_replay %.3g' % stt['q_replay'] if 'q_replay' in stt else ''))
    del eng
    torch.cuda.empty_cache()
    return fails


@pytest.mark.parametrize('name', list(CASES))
def test_head_edges(name):
    report = []
    try:
        fails = run_case(name, report)
    finally:
        print('\n'.join(report))
    assert not fails, '\n'.join(fails)
