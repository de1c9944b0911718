"""CPU: the accumulation chains of the bf16x3 kernels replayed under oracle/mfma_model.py - does the fitted accumulate of one
v_mfma_f32_16x16x32_bf16 produce the residual slope the per-layer GPU check records (profiles/b3_mfma_model.md)?

gemm_tile_b3 at K = 512: 16 k-steps of six MFMAs (piece pairs TA / TB, the small terms first), a lane group's eight k being
4 kk .. 4 kk + 3 and 16 + 4 kk .. + 3 of the step.  wgrad3 at 32768 rows as the kernel runs it: split over CFFM_NSLAB = 64 slabs, each
an accumulator of its own over 16 steps of 32 rows (six MFMAs a step, a lane group's eight rows one octet), and the 64 slab results
added in fp32 in slab order (cffm_reduce_slabs).  Operands of the per-layer cases' magnitudes: relu(N(0,1)) activations, N(0, 0.05)
filters, N(0, 0.01) gradients.

Reported against the float64 sum: the slope beta of oracle/layer_check.py over all outputs and over ref > 0, and the signed offset
alpha = sum(err) / sum(S).  Asserted: under 'exact sum, round to nearest' the slope is at the noise level of the fp32 chain replay
of tests/test_layer_check.py on the same operands (the weight gradient: of its own sampling noise); the replay under the fitted
member is a pure function of the seed, and its slopes are pinned to the values first computed."""
import numpy as np
import pytest
import torch

from oracle import layer_check as lc
from oracle import mfma_model as mm
from tests.test_layer_check import _emulate, _split

TA, TB = (2, 0, 1, 1, 0, 0), (0, 2, 1, 0, 1, 0)            # conv.hip, gemm_tile_b3 and wgrad3_kernel
EXACT_RNE = mm.EXACT_RNE
K_ORDER_GEMM = np.array([4 * kk + t + 16 * h for kk in range(4) for h in range(2) for t in range(4)])     # lane group kk, its 8 k


def operands(seed, N=96, K=512, J=96, relu=True):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, K))
    A = (np.maximum(A, 0) if relu else A).astype(np.float32)
    W = (rng.standard_normal((K, J)) * 0.05).astype(np.float32)
    return A, W


def chain(A, W, member, k_order=None):
    """[N, J] fp32 result of the bf16x3 chain over K in 32-deep steps under `member`."""
    pa, pb = _split(A, True), _split(W, True)
    N, K = A.shape
    J = W.shape[1]
    acc = np.zeros(N * J)
    for k0 in range(0, K, 32):
        ks = k0 + (np.arange(32) if k_order is None else k_order)
        for ta, tb in zip(TA, TB):
            a = np.broadcast_to(pa[ta][:, None, ks], (N, J, 32)).reshape(N * J, 32)
            b = np.broadcast_to(pb[tb][ks, :].T[None, :, :], (N, J, 32)).reshape(N * J, 32)
            acc = mm.mfma_step(acc, a, b, member)
    return acc.reshape(N, J)


def figures(got, A, W):
    a64, w64 = A.astype(np.float64), W.astype(np.float64)
    ref, S = torch.from_numpy(a64 @ w64), torch.from_numpy(np.abs(a64) @ np.abs(w64))
    g = torch.from_numpy(np.asarray(got, dtype=np.float64))
    st_all, st_pos = lc.stats(g, ref, S), lc.stats(g, ref, S, ref > 0)
    return {'beta': st_all['beta'], 'beta_pos': st_pos['beta'], 'alpha': st_all['alpha'], 'alpha_pos': st_pos['alpha'],
            'sigma': st_all['sigma_beta'], 'p999_u': st_all['p999_u']}


@pytest.fixture(scope='module')
def gemm():
    out = {}
    for seed in (0, 1):
        A, W = operands(seed)
        out[seed] = {name: figures(chain(A, W, m, K_ORDER_GEMM), A, W) for name, m in (('exact-rne', EXACT_RNE), ('fitted', mm.FITTED))}
        out[seed]['fp32-seq4'] = figures(_emulate(A.astype(np.float64), W.astype(np.float64), 'fp32-seq4'), A, W)
    return out


def test_forward_chain(gemm):
    for seed, r in gemm.items():
        print('gemm_tile_b3 K=512 seed %d: ' % seed + ' | '.join(
            '%s beta %.3g beta(ref>0) %.3g alpha %.3g alpha(ref>0) %.3g p99.9 %.2fu' % (
                n, f['beta'], f['beta_pos'], f['alpha'], f['alpha_pos'], f['p999_u']) for n, f in r.items()))
        e, s4 = r['exact-rne'], r['fp32-seq4']
        # exact sum, RNE: no systematic slope - at the noise level the fp32 chain replay itself shows on these operands
        assert abs(e['beta']) <= max(abs(s4['beta']), lc.BIAS_SIGMAS * e['sigma']), (e, s4)
    # the fitted member: a pure function of the seed, pinned per seed (a change of the member or of the replay moves it)
    for seed, want in PINNED_BETA_POS.items():
        assert gemm[seed]['fitted']['beta_pos'] == pytest.approx(want, rel=PINNED_REL), (seed, gemm[seed]['fitted'])


# The slope over ref > 0 of the fitted member's replay as first computed, per seed.  The two seeds differ by 47 % (the slope's own
# standard error over 96 x 96 outputs is 5e-9), so a margin taken from their spread would pin little; each seed is held to its own
# value, with a margin for the last bits of the float64 reference product only.  (The device: -2.2e-8 on two million outputs of
# f16-d32-b512, profiles/b3_mfma_model.md.)
PINNED_BETA_POS = {0: -2.5307824711877112e-08, 1: -1.345247166494327e-08}
PINNED_REL = 1e-6
NSLAB, STEPS = 64, 16                                       # wgrad3 at 32768 rows: 1024 steps of 32 rows over 64 slabs


def wgrad_chain(A, G, member):
    """[I, Q] fp32 weight gradient of A [I, M] (act(C[l-1])^T) and G [M, Q] (dC[l]) as wgrad3 + reduce_slabs form it."""
    pa, pb = _split(A, True), _split(G, True)
    I, Q = A.shape[0], G.shape[1]
    acc = np.zeros((NSLAB, I, Q))
    for t in range(STEPS):
        rows = (np.arange(NSLAB) * STEPS + t)[:, None] * 32 + np.arange(32)[None, :]          # [slab, 32]
        for ta, tb in zip(TA, TB):
            a = np.broadcast_to(pa[ta][:, rows].transpose(1, 0, 2)[:, :, None, :], (NSLAB, I, Q, 32))
            b = np.broadcast_to(pb[tb][rows, :].transpose(0, 2, 1)[:, None, :, :], (NSLAB, I, Q, 32))
            acc = mm.mfma_step(acc, a, b, member)
    out = acc[0]
    for s in range(1, NSLAB):                                # the slab sum: fp32, slab order
        out = (out + acc[s]).astype(np.float32).astype(np.float64)
    return out


# slope and offset of the fitted member's weight-gradient replay as first computed (seed 5, 24 x 24 outputs: the slope's standard
# error is 1.9e-8, so the slope says nothing about the device's -1.3e-8; the offset has its sign, -4.1e-9 on the device)
PINNED_WGRAD = (-3.686937288462893e-08, -2.488872405393699e-09)


def test_wgrad3_chain():
    rng = np.random.default_rng(5)
    M, I, Q = NSLAB * STEPS * 32, 24, 24
    A = np.maximum(rng.standard_normal((I, M)), 0).astype(np.float32)          # act(C[l-1])^T
    G = (rng.standard_normal((M, Q)) * 0.01).astype(np.float32)                # dC[l]
    out = {n: figures(wgrad_chain(A, G, m), A, G) for n, m in (('exact-rne', EXACT_RNE), ('fitted', mm.FITTED))}
    print('wgrad3 32768 rows, 64 slabs: ' + ' | '.join('%s beta %r (sigma %.2g) alpha %r p99.9 %.2fu' % (
        n, f['beta'], f['sigma'], f['alpha'], f['p999_u']) for n, f in out.items()))
    assert abs(out['exact-rne']['beta']) <= max(lc.BIAS_MAX, lc.BIAS_SIGMAS * out['exact-rne']['sigma'])
    assert (out['fitted']['beta'], out['fitted']['alpha']) == pytest.approx(PINNED_WGRAD, rel=PINNED_REL)
