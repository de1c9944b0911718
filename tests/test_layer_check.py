"""oracle/layer_check.py on the CPU: the per-layer float64 references agree with the whole-model oracle's intermediates, and the
tiers separate a correct fp32 contraction from the two kinds of subtly wrong bf16x3 contraction (the evidence for the constants)."""
import numpy as np
import pytest
import torch

from cffm_amd.spec import CFFMConfig, init_params
from oracle import cffm_oracle as orc
from oracle import layer_check as lc

CONFIGS = {
    'f5-d16-selu': dict(M=200, F=5, K=8, D=16, act='selu', B=3),
    'f7-d8-gelu': dict(M=100, F=7, K=4, D=8, act='gelu', B=4),
    'f6-d32-prelu': dict(M=300, F=6, K=8, D=32, act='prelu', B=2),
}


def _case(name):
    c = CONFIGS[name]
    cfg = CFFMConfig(M=c['M'], F=c['F'], K=c['K'], D=c['D'], activation=c['act'], lamda_att=1.3)
    p32 = init_params(cfg, seed=5, dtype=np.float32)
    rng = np.random.default_rng(11)
    p32['outer_embeddings'] = (p32['outer_embeddings'] * 20.0).astype(np.float32)
    for l in range(cfg.Lc):       # biases of either sign, so that relu and the gated gradient both have work to do
        k = 'outer_layer_conv_bias_%d' % l
        p32[k] = (rng.standard_normal(p32[k].shape) * 0.05).astype(np.float32)
    X = rng.integers(0, cfg.M, size=(c['B'], cfg.F)).astype(np.int32)
    y = rng.choice([-1.0, 1.0], size=(c['B'],)).astype(np.float32)
    return cfg, p32, X, y


def _near(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(float(np.abs(ref).max()), 1e-300)
    assert float(np.abs(got - ref).max()) <= 1e-12 * scale, (what, float(np.abs(got - ref).max()), scale)


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_references_match_oracle(name):
    cfg, p32, X, y = _case(name)
    p64 = {k: np.asarray(v, dtype=np.float64) for k, v in p32.items()}
    out, c = orc.forward(p64, X, cfg)
    _, dout = orc.loss_and_grad(out, y.astype(np.float64), cfg, p64)
    g = orc.backward(p64, c, dout, cfg)
    Eo = p32['outer_embeddings'][X]
    D, live = cfg.D, cfg.live_layers
    assert live >= 2
    off = [sum(D >> i for i in range(l)) for l in range(live + 1)]
    n_relu_zero = 0
    for l in range(live):
        prev = Eo if l == 0 else c['rs'][l - 1]
        W, b = p64['outer_layer_conv_weight_%d' % l], p64['outer_layer_conv_bias_%d' % l]
        z, S = lc.ref_forward(prev, W, b, l, cfg, fp32_act=False)
        _near(z.numpy(), c['zs'][l], 'z[%d]' % l)
        assert bool((S >= z.abs() - 1e-12 * S.max()).all())
        pool, _ = lc.ref_pool(c['rs'][l], cfg, fp32_act=False)
        _near(pool.numpy(), c['pools'][l + 1], 'pool[%d]' % (l + 1))
        gw, sw, gb, sb = lc.ref_wgrad(prev, g['_dC'][l], l, cfg, fp32_act=False)
        _near(gw.numpy(), g['outer_layer_conv_weight_%d' % l], 'grad W[%d]' % l)
        _near(gb.numpy(), g['outer_layer_conv_bias_%d' % l], 'grad b[%d]' % l)
        if l >= 1:
            d, _ = lc.ref_dgrad(g['_dC'][l], W, g['_dt1'][:, off[l]:off[l] + (D >> l)], c['rs'][l - 1], l, cfg, fp32_act=False)
            _near(d.numpy(), g['_dC'][l - 1], 'dC[%d]' % (l - 1))
            n_relu_zero += int((c['rs'][l - 1] == 0).sum())
        else:
            d, _ = lc.ref_dgrad0(g['_dC'][0], W, g['_dt1'][:, :D], Eo, cfg)
            _near(d.numpy(), g['d_outer_rows'], 'dEo')
    assert n_relu_zero > 0                    # the gate [C > 0] was exercised


# ---- the tiers on emulated contractions -----------------------------------------------------------------------------
def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _bf16_trunc(x):
    return (_bits(x) & np.uint32(0xffff0000)).view(np.float32)


def _bf16_rn(x):
    u = _bits(x).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def _split(x, rn):
    f = _bf16_rn if rn else _bf16_trunc
    x = np.asarray(x, dtype=np.float32)
    x1 = f(x)
    r = (x - x1).astype(np.float32)          # exact in both forms
    x2 = f(r)
    x3 = (r - x2).astype(np.float32)
    assert np.array_equal(_bf16_trunc(x3), x3), 'the third piece must be an exact bf16'
    return [v.astype(np.float64) for v in (x1, x2, x3)]


TERMS6 = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))


def _emulate(A, W, mode):
    """Contraction A [N,K] @ W [K,J] as a kernel would compute it, in float64, rounded to fp32 at the end (except the fp32 chain,
    which rounds every step).  bf16x3 modes: the split pieces' cross terms summed exactly - what is left is the split's error."""
    if mode == 'fp32-seq4':                   # the 16x16x4 fp32 MFMA chain: four exact products per step, fp32 accumulator
        a32, w32 = A.astype(np.float32), W.astype(np.float32)
        acc = np.zeros((A.shape[0], W.shape[1]), dtype=np.float32)
        for k in range(0, A.shape[1], 4):
            step = a32[:, k:k + 4].astype(np.float64) @ w32[k:k + 4].astype(np.float64)
            acc = (acc.astype(np.float64) + step).astype(np.float32)
        return acc.astype(np.float64)
    rn = mode != 'trunc'
    terms = TERMS6 if mode != 'rn-5terms' else TERMS6[:5]      # five terms: a3 b1 dropped
    pa, pw = _split(A, rn), _split(W, rn)
    out = sum(pa[i] @ pw[j] for i, j in terms)
    return out.astype(np.float32).astype(np.float64)


@pytest.fixture(scope='module')
def replay():
    """relu inputs, mixed-sign weights, K = 1984 (the stress shape's forward depth), 256 x 256 outputs."""
    rng = np.random.default_rng(3)
    K, N, J = 1984, 256, 256
    A = np.maximum(rng.standard_normal((N, K)), 0).astype(np.float32).astype(np.float64)
    W = (rng.standard_normal((K, J)) * 0.05).astype(np.float32).astype(np.float64)
    ref = torch.from_numpy(A @ W)
    S = torch.from_numpy(np.abs(A) @ np.abs(W))
    res = {}
    for mode in ('fp32-seq4', 'trunc', 'rn', 'rn-5terms'):
        res[mode] = torch.from_numpy(_emulate(A, W, mode))
    return ref, S, res, K


def _verdict(ref, S, got, K, twin):
    out = {}
    for tier in ('hard', 'bias', 'dist'):
        try:
            if tier == 'hard':
                lc.check_tiers('replay', got, ref, S, K, bias=False)
            elif tier == 'bias':
                lc.check_tiers('replay', got, ref, S, K, bias=True, bias_mask=ref > 0)
            else:
                st = lc.stats(got, ref, S)
                lim = lc.DIST_FACTOR * twin['p999_u'] + lc.DIST_SLACK
                assert st['p999_u'] <= lim
            out[tier] = True
        except AssertionError:
            out[tier] = False
    return out


def test_tiers_separate_mutants(replay):
    ref, S, res, K = replay
    twin = lc.stats(res['fp32-seq4'], ref, S)
    v = {m: _verdict(ref, S, res[m], K, twin) for m in res}
    st = {m: lc.stats(res[m], ref, S, ref > 0) for m in res}
    msg = ' | '.join('%s: beta %.3g (sigma %.2g) p99.9 %.2f u %s' % (m, st[m]['beta'], st[m]['sigma_beta'], st[m]['p999_u'], v[m])
                     for m in res)
    assert st['trunc']['n_beta'] >= lc.BIAS_MIN_N, msg
    assert all(v[m]['hard'] for m in res), msg                       # no element-wise bound can tell them apart
    assert v['fp32-seq4'] == {'hard': True, 'bias': True, 'dist': True}, msg
    assert v['rn'] == {'hard': True, 'bias': True, 'dist': True}, msg
    assert not v['trunc']['bias'] and v['trunc']['dist'], msg       # truncation: a bias below the fp32 noise
    assert v['rn-5terms']['bias'] and not v['rn-5terms']['dist'], msg   # a dropped cross term: unbiased, but too wide
    # the separation is not marginal: truncation's slope is several bars away, the two correct forms well inside one
    # the bar the GPU tests hold bf16x3 tensors to (a twin given: BIAS_MAX_B3, 2 |beta_fp32|): truncation still fails it
    tw = lc.stats(res['fp32-seq4'], ref, S, ref > 0)
    for m, slope_ok in (('trunc', False), ('rn', True), ('rn-5terms', True)):
        try:
            lc.check_tiers('replay', res[m], ref, S, K, bias_mask=ref > 0, twin=tw)
            why = ''
        except AssertionError as e:
            why = str(e)
        assert ('slope' not in why) == slope_ok, (m, why, msg)
    bar = lambda m: max(lc.BIAS_MAX, lc.BIAS_SIGMAS * st[m]['sigma_beta'])
    assert abs(st['trunc']['beta']) > 3 * bar('trunc'), msg
    assert abs(st['rn']['beta']) < 0.5 * bar('rn') and abs(st['fp32-seq4']['beta']) < 0.5 * bar('fp32-seq4'), msg


def test_b3_coverage():
    """The GPU layer cases (tests/test_gpu_layers.py) reach every bf16x3 instance with each A-operand activation build, and the gelu arm of the wide kernels."""
    from tests.test_gpu_layers import CASES, b3_set, make_layer_case
    seen = {}
    for name, c in CASES.items():
        cfg, _, X, _ = make_layer_case(name)
        for d, _ in b3_set(cfg, X.shape[0]):
            seen.setdefault(d, set()).add(c['act'])
    assert {'relu', 'selu', 'gelu'} <= seen.get('fwd', set()) and {'relu', 'selu', 'gelu'} <= seen.get('dgrad', set()), seen
    assert 'gelu' in seen.get('wgrad', set()) and len(seen['wgrad']) >= 3, seen


@pytest.mark.parametrize('kind', ['relu', 'elu', 'prelu', 'selu', 'gelu'])
def test_fp32_activation(kind):
    """act32 is the model's fp32 activation: within a few fp32 ulps of the float64 one, and for selu exactly the fp32-rounded
    constant (a relative offset of 3.3e-8 that the references must not attribute to the contraction)."""
    x = torch.from_numpy(np.random.default_rng(1).standard_normal(20000).astype(np.float32)).double()
    a, g = lc.act32(x, kind)
    a6, g6 = lc.act64(x, kind), lc.act_grad64(x, kind)
    assert float((a - a6).abs().max()) <= 8 * lc.U * float(a6.abs().max())
    assert float((g - g6).abs().max()) <= 8 * lc.U * float(g6.abs().max())
    if kind == 'selu':
        pos = x > 0
        assert np.allclose(float((a[pos] / a6[pos]).mean()) - 1, float(np.float32(orc.SELU_SCALE)) / orc.SELU_SCALE - 1, rtol=1e-3)
