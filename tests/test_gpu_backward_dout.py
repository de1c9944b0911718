"""cffm_backward_dout (HipEngine.backward_dout): the backward from a dL/dout the caller chose, against oracle.backward with the same
dout - oracle.parity.check_backward_stages with the loss taken out.  The float32 dout handed to the device IS the oracle's dout
(the float64 one is the float32 one widened), so there is no dout_slack and no dense_grad_slack: only the relu decisions within
rounding of 0 are adopted from the device (adopt_device_kinks, capped) and the inner branch's kinks get their two-sided slack.
dout is normal / B with about 10 % exact zeros and one example 1000 times larger: a hidden 1/B, 1/L or clip would show.

Then three exact statements: the bits of cffm_backward on the route it shares (regularised square loss: dL/dout = out - y), the
bits of twice the gradients for twice the dout, and the bits of a clean workspace on a dirty one."""
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
from oracle.parity import adopt_device_kinks, close, inner_kink_slack, pad_channels, to64  # noqa: E402

gpu = pytest.mark.gpu
assert 'cffm_backward_dout' in hip.PROTOTYPES           # the entry point this file is about

# K = D.  seed: one for which the oracle's own pre-activations stay within adopt_device_kinks' cap (checked without a GPU by
# test_the_seeds_keep_the_oracle_within_the_kink_cap below)
CASES = {
    'f3-d8-b6-relu': dict(F=3, D=8, B=6, act='relu'),
    'f6-d32-b12-elu': dict(F=6, D=32, B=12, act='elu', seed=1),             # (seed 0: 3 decisions in layer 2, the cap is 2.88)
    'f10-d32-b15-selu': dict(F=10, D=32, B=15, act='selu'),
    'f12-d32-b6-relu': dict(F=12, D=32, B=6, act='relu'),                   # Pp = 80: the wide-filter instances
    'f5-d16-b9-gelu': dict(F=5, D=16, B=9, act='gelu', outer_conv=0),
    'f5-d16-b9-prelu': dict(F=5, D=16, B=9, act='prelu', inner_conv=0),
    'f4-d8-b7-relu': dict(F=4, D=8, B=7, act='relu', linear_att=0),
}


def make_case(name, seed=None, **over):
    c = dict(CASES[name], **over)
    seed = c.get('seed', 0) if seed is None else seed
    cfg = CFFMConfig(M=40 * c['F'], F=c['F'], K=c['D'], D=c['D'], activation=c['act'], lamda_att=1.3, linear_att=c.get('linear_att', 1),
                     inner_conv=c.get('inner_conv', 1), outer_conv=c.get('outer_conv', 1), lamda_bilinear=c.get('lamda', 0.0))
    p32 = init_params(cfg, seed=seed, dtype=np.float32)
    rng = np.random.default_rng(seed + 7)
    p32['feature_bias'] = (rng.standard_normal(p32['feature_bias'].shape) * 0.3).astype(np.float32)     # exactly 0 at init
    p32['outer_embeddings'] = (p32['outer_embeddings'] * 20.0).astype(np.float32)
    p32['inner_embeddings'] = (p32['inner_embeddings'] * 4.0).astype(np.float32)
    B = c['B']
    X = rng.integers(0, cfg.M, size=(B, cfg.F)).astype(np.int32)
    X[1] = X[0]                                                             # duplicate ids in every column
    dout = rng.standard_normal(B) / B
    dout[rng.random(B) < 0.1] = 0.0
    dout[2] = 0.0                                                           # at least one exact zero at every B
    dout[B // 2] = 1000.0 * (1.0 + rng.random()) / B                        # one example 1000 times the others
    return cfg, p32, X, dout.astype(np.float32)


def engine_for(cfg, p32):
    from cffm_amd.engine import HipEngine
    return HipEngine(cfg, params=p32)


def test_the_seeds_keep_the_oracle_within_the_kink_cap():
    """No GPU is used here: the cap adopt_device_kinks asserts (at most max(2, 0.1 %) decisions per layer) holds for the oracle's
    own pre-activations at every case's seed, so a failure of that assertion on the device is the device's."""
    for name in CASES:
        cfg, p32, X, _ = make_case(name)
        _, c = orc.forward(to64(p32), X, cfg)
        for l in range(cfg.live_layers if cfg.outer_conv else 0):
            z = c['zs'][l]
            kink = np.abs(z) < 1e-5 * np.abs(z).max()
            assert kink.sum() <= max(2, 1e-3 * kink.size), (name, l, int(kink.sum()))


def _views(eng, cfg, B):
    """Every tensor cffm_backward_dout leaves, by name (views of the workspace and of eng.grad)."""
    Pp = eng.tl.Pp
    v = {'dout': eng.ws_tensor(B, 'dout', (B,)), 'dfb': eng.ws_tensor(B, 'dfb', (B, cfg.F)), 'grad': eng.grad}
    if cfg.outer_conv:
        v['dt1'] = eng.ws_tensor(B, 'dt1', (B, 2 * cfg.D - 2))
        for l in range(cfg.live_layers):
            S = cfg.D >> (l + 1)
            v['dC[%d]' % l] = eng.ws_tensor(B, 'dC', (B, S, S, Pp), index=l)
        v['dEo'] = eng.ws_tensor(B, 'dEo', (B, cfg.F, cfg.D))
    if cfg.inner_conv:
        v['dEi'] = eng.ws_tensor(B, 'dEi', (B, cfg.F, cfg.K))
    return v


def _snapshot(eng, cfg, B):
    torch.cuda.synchronize()
    return {k: t.detach().cpu().numpy().copy() for k, t in _views(eng, cfg, B).items()}


def _same_bits(got, want, what):
    for k in want:
        a, b = got[k].view(np.uint32), want[k].view(np.uint32)
        assert np.array_equal(a, b), '%s: %s differs in %d of %d elements (first at %s: %r vs %r)' % (
            what, k, int((a != b).sum()), a.size, np.unravel_index(int((a != b).argmax()), a.shape),
            got[k].reshape(-1)[int((a != b).argmax())], want[k].reshape(-1)[int((a != b).argmax())])


@gpu
@pytest.mark.parametrize('name', list(CASES))
def test_backward_dout_against_oracle(name):
    cfg, p32, X, dout32 = make_case(name)
    B = X.shape[0]
    p64 = to64(p32)
    dout = dout32.astype(np.float64)                        # the oracle's dout is the device's, exactly
    _, c = orc.forward(p64, X, cfg)
    eng = engine_for(cfg, p32)
    ids, dt = torch.from_numpy(X).cuda(), torch.from_numpy(dout32).cuda()
    eng.forward(ids, None)
    torch.cuda.synchronize()
    if cfg.outer_conv:
        print('%s: %d relu decisions adopted from the device' % (name, adopt_device_kinks(cfg, eng, B, c)))
    g = orc.backward(p64, c, dout, cfg)
    eng.backward_dout(dt, B)
    got = _snapshot(eng, cfg, B)
    assert np.array_equal(got['dout'].view(np.uint32), dout32.view(np.uint32)), 'ws.dout is not the dout handed in'
    slack = inner_kink_slack(p64, c, dout, cfg)
    Pp = eng.tl.Pp
    if cfg.outer_conv:
        close(got['dt1'], g['_dt1'], 'dt1 (given dout)')
        for l in range(cfg.live_layers - 1, -1, -1):
            close(got['dC[%d]' % l], pad_channels(g['_dC'][l], Pp), 'dC[%d] (given dout)' % l)
        close(got['dEo'], g['d_outer_rows'], 'dEo (given dout)')
    if cfg.inner_conv:
        close(got['dEi'], g['d_inner_rows'], 'dEi (given dout)', extra=slack.get('d_inner_rows'))
    close(got['dfb'], g['d_bias_rows'], 'dfb (given dout)')
    for k, v in eng.export_grad().items():
        if k in g:
            close(v, np.asarray(g[k]).reshape(v.shape), 'grad %s (given dout)' % k, extra=slack[k].reshape(v.shape) if k in slack else None)
        else:                                               # parameters of a disabled branch receive no gradient
            assert not (cfg.linear_att and cfg.inner_conv and cfg.outer_conv), k
            assert np.all(v == 0), k


@gpu
@pytest.mark.parametrize('name', ['f6-d32-b12-elu', 'f12-d32-b6-relu'])
def test_same_bits_as_backward_on_the_route_they_share(name):
    """Regularised square loss (CFFM_LOSS_SQUARE_L2): cffm_backward takes the stage launches with dL/dout = out - y.  The same dout
    formed in torch float32 and handed to cffm_backward_dout must leave the same bits everywhere."""
    cfg, p32, X, _ = make_case(name, lamda=0.02)
    B = X.shape[0]
    eng = engine_for(cfg, p32)
    assert eng.shape.loss == 4
    rng = np.random.default_rng(5)
    ids = torch.from_numpy(X).cuda()
    y = torch.from_numpy(rng.choice([-1.0, 1.0], size=B).astype(np.float32)).cuda()
    eng.forward(ids, y)
    eng.backward(y, B)
    want = _snapshot(eng, cfg, B)
    dout = eng.predictions(B) - y
    assert np.array_equal(dout.cpu().numpy().view(np.uint32), want['dout'].view(np.uint32))
    for t in _views(eng, cfg, B).values():
        t.fill_(float('nan'))
    eng.backward_dout(dout, B)
    _same_bits(_snapshot(eng, cfg, B), want, name + ' vs cffm_backward')


@gpu
@pytest.mark.parametrize('name', ['f6-d32-b12-elu', 'f10-d32-b15-selu', 'f12-d32-b6-relu'])
def test_twice_the_dout_gives_twice_the_gradients_bit_for_bit(name):
    cfg, p32, X, dout32 = make_case(name)
    B = X.shape[0]
    eng = engine_for(cfg, p32)
    eng.forward(torch.from_numpy(X).cuda(), None)
    eng.backward_dout(torch.from_numpy(dout32).cuda(), B)
    once = _snapshot(eng, cfg, B)
    tiny = min(float(np.abs(v[v != 0]).min()) for v in once.values() if (v != 0).any())
    assert tiny > 1e-35, 'the inputs reach down to denormals (%g): doubling would not be exact' % tiny
    eng.backward_dout(torch.from_numpy(2.0 * dout32).cuda(), B)
    _same_bits(_snapshot(eng, cfg, B), {k: 2.0 * v for k, v in once.items()}, name + ' doubled')


@gpu
@pytest.mark.parametrize('fill', [float('nan'), 3.39e38])
@pytest.mark.parametrize('name', ['f6-d32-b12-elu', 'f12-d32-b6-relu', 'f5-d16-b9-prelu', 'f5-d16-b9-gelu'])
def test_a_dirty_workspace_gives_the_bits_of_a_clean_one(name, fill):
    cfg, p32, X, dout32 = make_case(name)
    B = X.shape[0]
    eng = engine_for(cfg, p32)
    dt = torch.from_numpy(dout32).cuda()
    eng.forward(torch.from_numpy(X).cuda(), None)
    _, wl = eng.workspace(B)
    dirty = [eng.ws_tensor(B, 'scalars', (16,)), eng.ws_tensor(B, 'gpart', (int(wl.gpart_floats),)),
             eng.ws_tensor(B, 'dEi', (B, cfg.F, cfg.K)), eng.ws_tensor(B, 'dEo', (B, cfg.F, cfg.D)),
             eng.ws_tensor(B, 'dt1', (B, 2 * cfg.D - 2))]
    dirty += [eng.ws_tensor(B, 'dC', (B, cfg.D >> (l + 1), cfg.D >> (l + 1), eng.tl.Pp), index=l) for l in range(eng.tl.live)]
    dirty += list(_views(eng, cfg, B).values())
    for t in dirty:
        t.zero_()
    eng.backward_dout(dt, B)
    want = _snapshot(eng, cfg, B)
    for t in dirty:
        t.fill_(fill)
    eng.backward_dout(dt, B)
    _same_bits(_snapshot(eng, cfg, B), want, '%s dirty (%r)' % (name, fill))
