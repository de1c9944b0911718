"""Per-layer check of the outer conv stack: each layer's outputs against the float64 contraction of the inputs the device read.

TEST INFRASTRUCTURE, like everything under oracle/: only tests/ may import it; the product path (cffm_amd/) never does.

oracle/parity.py compares the whole model with one tolerance for every tensor, so an error that a layer makes is mixed with
what it inherits from upstream, and a systematic loss far below that tolerance passes.  Here every layer is re-anchored: the
reference of layer l is computed in float64 from the device's own fp32 inputs of that layer (C[l-1] or ws.Eo, dC[l], dt1,
the filter in theta), so no error propagates and no relu decision has to be adopted.  Each reference also returns, per element,
S = sum_k |a_k w_k| (+ |b|): the scale every fp32 summation order's rounding error is measured against.

Four tiers (check_tiers):
  exact         pad channels of C[l] / dC[l] are 0, C[l] >= 0, the relu mask bit of every element is C[l] > 0, dC[l-1] is 0
                wherever the device's C[l-1] is 0 (exact_* helpers)
  hard          |err| <= (n_terms + 2) u S per element: rigorous for any fp32 summation order of n_terms terms (u = 2^-24);
                catches a wrong, missing or double-counted term
  distribution  bf16x3 instances only: the 99.9th percentile of |err| / S within DIST_FACTOR x the same statistic of the fp32
                loop on the same case, plus DIST_SLACK u
  bias          |beta| <= max(BIAS_MAX, BIAS_SIGMAS sigma_beta) with beta = sum err ref / sum ref^2 over >= BIAS_MIN_N elements
                with ref != 0 (the forward: z > 0 only): a systematic relative error that no element-wise bound can separate from
                rounding noise.  sigma_beta = sqrt(sum (err ref)^2) / sum ref^2 is the slope's standard error if the errors were
                zero-mean: a correct fp32 sum over 10^4 elements can have |beta| ~ 5e-9 by chance, one over 10^6 elements cannot.
                bf16x3 tensors (a twin is given): BIAS_MAX_B3 in place of BIAS_MAX

The constants come from a CPU replay of the bf16x3 contraction (tests/test_layer_check.py keeps the evidence: a truncating
split fails the bias tier, dropping one of the six cross terms fails the distribution tier, a round-to-nearest split and a
sequential fp32 chain pass both)."""
import math
import os

import numpy as np

from . import cffm_oracle as orc
from .parity import WORST, WORST_AT

U = 2.0 ** -24
BIAS_MAX = 2.0 ** -27          # 7.5e-9
BIAS_MIN_N = 10000
BIAS_SIGMAS = 4.0              # the bar never sits inside the slope's own sampling noise (see stats())
BIAS_MAX_B3 = 2.0 ** -26       # bf16x3 tensors: their measured residual slope with the round-to-nearest split reaches 1.0e-8
                               # (DESIGN.md 3.4); a truncating split puts the same tensors at 3.4e-8 .. 5e-8
DIST_FACTOR = 1.5
DIST_SLACK = 0.5               # in units of u

SELU_SCALE = orc.SELU_SCALE
SELU_SCALE_ALPHA = orc.SELU_SCALE_ALPHA
PRELU_ALPHA = orc.PRELU_ALPHA


def _torch():
    import torch
    return torch


def t64(x, device):
    """float64 torch tensor of an fp32 array / tensor (exact)."""
    torch = _torch()
    if isinstance(x, torch.Tensor):
        return x.detach().to(device=device, dtype=torch.float64)
    return torch.as_tensor(np.asarray(x), dtype=torch.float64, device=device)


def act32(x, kind):
    """act(x) and act'(x) of fp32 values as the model defines them in fp32 (constants rounded to fp32, evaluated in fp32, as
    common.hpp does): the activation feeds the contraction but is not part of it, so the references take it from the same fp32
    function and do only the contraction in float64.  (In float64 the fp32 rounding of SELU_SCALE alone is a slope of 3.3e-8.)"""
    torch = _torch()
    x32 = x.to(torch.float32)
    if kind == 'gelu':
        a = x32 * (0.5 * (1.0 + torch.erf(x32 * 0.70710678118654752440)))
        cdf = 0.5 * (1.0 + torch.erf(x32 * 0.70710678118654752440))
        g = cdf + x32 * (torch.exp(-0.5 * x32 * x32) * 0.39894228040143267794)
    elif kind == 'selu':
        sc, sa = float(np.float32(SELU_SCALE)), float(np.float32(SELU_SCALE_ALPHA))     # python scalars: applied in float32
        a = torch.where(x32 < 0, sa * (torch.exp(torch.clamp(x32, max=0)) - 1.0), sc * x32)
        g = torch.where(x32 < 0, sa * torch.exp(torch.clamp(x32, max=0)), torch.full_like(x32, sc))
    else:
        return act64(x, kind), act_grad64(x, kind)
    return a.to(torch.float64), g.to(torch.float64)


def act64(x, kind):
    torch = _torch()
    if kind == 'relu':
        return torch.clamp(x, min=0)
    if kind == 'elu':
        return torch.where(x < 0, torch.expm1(torch.clamp(x, max=0)), x)
    if kind == 'selu':
        return torch.where(x < 0, SELU_SCALE_ALPHA * torch.expm1(torch.clamp(x, max=0)), SELU_SCALE * x)
    if kind == 'prelu':
        return torch.where(x < 0, PRELU_ALPHA * x, x)
    if kind == 'gelu':
        return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    raise ValueError(kind)


def act_grad64(x, kind):
    """d act / dx as orc.act_grad (TF-1.14 autodiff)."""
    torch = _torch()
    if kind == 'relu':
        return (x > 0).to(x.dtype)
    if kind == 'elu':
        y = act64(x, 'elu')
        return torch.where(y < 0, y + 1, torch.ones_like(x))
    if kind == 'selu':
        y = act64(x, 'selu')
        return torch.where(y < 0, y + SELU_SCALE_ALPHA, torch.full_like(x, SELU_SCALE))
    if kind == 'prelu':
        return (x > 0).to(x.dtype) + PRELU_ALPHA * (x < 0).to(x.dtype)
    if kind == 'gelu':
        cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
        pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
        return cdf + x * pdf
    raise ValueError(kind)


def _im2col(A):
    B, S, _, C = A.shape
    h = S // 2
    return A.reshape(B, h, 2, h, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, h, h, 4 * C)


def _col2im(G, C):
    B, h, _, _ = G.shape
    return G.reshape(B, h, h, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * h, 2 * h, C)


def outer_map(Eo, F):
    """ws.Eo [B,F,D] -> the outer-product map [B,D,D,P] of CFFM.py:355-367 (exact in float64)."""
    ii, jj = orc.pair_index(F)
    return (Eo[:, ii, :, None] * Eo[:, jj, None, :]).permute(0, 2, 3, 1)


def layer_input(prev, l, cfg, fp32_act=True):
    """Input map of conv layer l as the device reads it: the outer-product map of ws.Eo (l = 0) or act(C[l-1]) (fp32_act: the fp32
    activation, see act32; False: float64, as the whole-model oracle)."""
    if l == 0:
        return outer_map(prev, cfg.F)
    return act32(prev, cfg.activation)[0] if fp32_act else act64(prev, cfg.activation)


CHUNK = 1 << 22            # float64 elements of one layer-input chunk of the references (tests may raise it for big batches)


def _chunks(B, rows_per_ex, budget=None):
    budget = budget or CHUNK
    step = max(1, budget // max(1, rows_per_ex))
    return [(b, min(B, b + step)) for b in range(0, B, step)]


# ---- references: each returns (ref, S) in float64, arguments are the device's fp32 values ------------------------------
def ref_forward(prev, W, b, l, cfg, device='cpu', fp32_act=True):
    """z_l = im2col(input_l) @ W_l + b_l  [B,S,S,P] and S = |im2col(input_l)| @ |W_l| + |b_l|.  prev = ws.Eo (l = 0) or the
    device's C[l-1] without pad channels; W [2,2,P,P] (HWIO); b [P].  n_terms = 4P + 1."""
    torch = _torch()
    P = cfg.P
    W4 = t64(W, device).reshape(4 * P, P)
    bb = t64(b, device)
    prev = t64(prev, device)
    B = prev.shape[0]
    S_in = cfg.D >> l
    zs, ss = [], []
    for b0, b1 in _chunks(B, S_in * S_in * P):
        x = _im2col(layer_input(prev[b0:b1], l, cfg, fp32_act))
        zs.append(x @ W4 + bb)
        ss.append(x.abs() @ W4.abs() + bb.abs())
    return torch.cat(zs), torch.cat(ss)


def ref_dgrad(dC, W, dpool, prevC, l, cfg, device='cpu', fp32_act=True):
    """Input gradient of conv layer l >= 1: dC[l-1] = (dpool_l broadcast + col2im(dC_l @ W_l^T)) * act'(C[l-1]) * [C[l-1] > 0],
    dpool_l = dt1 columns of pool l (the sum pool of act(C[l-1])).  n_terms = P + 1, then one multiply."""
    torch = _torch()
    P = cfg.P
    W4 = t64(W, device).reshape(4 * P, P)
    dC, dpool, prevC = t64(dC, device), t64(dpool, device), t64(prevC, device)
    B = dC.shape[0]
    outs, ss = [], []
    for b0, b1 in _chunks(B, (cfg.D >> l) ** 2 * P):
        g = dC[b0:b1]
        dp = dpool[b0:b1][:, :, None, None]
        c = prevC[b0:b1]
        gate = (act32(c, cfg.activation)[1] if fp32_act else act_grad64(c, cfg.activation)) * (c > 0)
        outs.append((_col2im(g @ W4.T, P) + dp) * gate)
        ss.append((_col2im(g.abs() @ W4.abs().T, P) + dp.abs()) * gate.abs())
    return torch.cat(outs), torch.cat(ss)


def ref_dgrad0(dC0, W, dpool0, Eo, cfg, device='cpu'):
    """Input gradient of layer 0 = dEo [B,F,D]: dA = dpool_0 broadcast + col2im(dC_0 @ W_0^T) over the [B,D,D,P] map, then the
    outer product's gradient dEo[b,i_p,h] += sum_w dA[b,h,w,p] Eo[b,j_p,w] (and symmetrically).  n_terms = P + 1 + (F-1) D."""
    torch = _torch()
    P, F = cfg.P, cfg.F
    ii, jj = orc.pair_index(F)
    W4 = t64(W, device).reshape(4 * P, P)
    dC0, dpool0, Eo = t64(dC0, device), t64(dpool0, device), t64(Eo, device)
    B = Eo.shape[0]
    outs, ss = [], []
    iit, jjt = torch.as_tensor(ii, device=device), torch.as_tensor(jj, device=device)
    for b0, b1 in _chunks(B, cfg.D * cfg.D * P):
        res = []
        for sign in (1, -1):              # (values, magnitudes): the same contraction on |.|
            g = dC0[b0:b1] if sign > 0 else dC0[b0:b1].abs()
            w = W4 if sign > 0 else W4.abs()
            dp = dpool0[b0:b1] if sign > 0 else dpool0[b0:b1].abs()
            e = Eo[b0:b1] if sign > 0 else Eo[b0:b1].abs()
            dA = _col2im(g @ w.T, P) + dp[:, :, None, None]
            gi = torch.einsum('bhwp,bpw->bph', dA, e[:, jjt, :])
            gj = torch.einsum('bhwp,bph->bpw', dA, e[:, iit, :])
            d = torch.zeros_like(e)
            d.index_add_(1, iit, gi)
            d.index_add_(1, jjt, gj)
            res.append(d)
        outs.append(res[0])
        ss.append(res[1])
    return torch.cat(outs), torch.cat(ss)


def ref_wgrad(prev, dC, l, cfg, device='cpu', fp32_act=True):
    """Weight and bias gradient of layer l: im2col(input_l)^T @ dC_l -> [2,2,P,P], sum dC_l -> [P]; with their S.
    n_terms = B S_l^2 (the rows).  The inputs are converted chunk by chunk (a full-size C[0] is 4e9 elements)."""
    torch = _torch()
    P = cfg.P
    B = dC.shape[0]
    gw = torch.zeros(4 * P, P, dtype=torch.float64, device=device)
    sw = torch.zeros_like(gw)
    gb = torch.zeros(P, dtype=torch.float64, device=device)
    sb = torch.zeros_like(gb)
    for b0, b1 in _chunks(B, (cfg.D >> l) ** 2 * P):
        x = _im2col(layer_input(t64(prev[b0:b1], device), l, cfg, fp32_act)).reshape(-1, 4 * P)
        g = t64(dC[b0:b1], device).reshape(-1, P)
        gw += x.T @ g
        sw += x.abs().T @ g.abs()
        gb += g.sum(0)
        sb += g.abs().sum(0)
    return gw.reshape(2, 2, P, P), sw.reshape(2, 2, P, P), gb, sb


def ref_pool(C, cfg, device='cpu', fp32_act=True):
    """Sum pool of act(C_l) per (example, row) [B,S] (CFFM.py:390-391): the pool l+1 of t1.  n_terms = S P."""
    a = layer_input(t64(C, device), 1, cfg, fp32_act)
    return a.sum(dim=(2, 3)), a.abs().sum(dim=(2, 3))


# ---- tiers --------------------------------------------------------------------------------------------------------------
def stats(got, ref, S, bias_mask=None):
    """|err| / S percentiles (units of u), the regression slope beta and its element count, as plain floats."""
    torch = _torch()
    got, ref, S = t64(got, ref.device), ref, S
    err = got - ref
    pos = S > 0
    r = (err.abs()[pos] / S[pos]).flatten()
    m = ref != 0
    if bias_mask is not None:
        m = m & bias_mask
    n_b = int(m.sum())
    den = float((ref[m] * ref[m]).sum())
    beta = float((err[m] * ref[m]).sum()) / den if den > 0 else 0.0
    sigma = math.sqrt(float(((err[m] * ref[m]) ** 2).sum())) / den if den > 0 else 0.0
    if r.numel() > 2 ** 24:                       # torch.quantile's limit: a strided subsample
        r = r[::int(math.ceil(r.numel() / 2 ** 24))]
    p999 = float(torch.quantile(r, 0.999)) / U if r.numel() else 0.0
    # the signed offset alpha = mean(err) / mean(S) over the same elements: a report field (a constant one-sided loss per accumulate
    # shows here on a symmetric tensor, where it cannot show in the slope), no tier reads it
    alpha = float(err[m].sum()) / float(S[m].sum()) if n_b and float(S[m].sum()) > 0 else 0.0
    return {'beta': beta, 'alpha': alpha, 'sigma_beta': sigma, 'n_beta': n_b, 'p999_u': p999, 'max_u': float(r.max()) / U if r.numel() else 0.0, 'n': int(err.numel())}


def _record(name, ratio):
    if ratio > WORST.get(name, -1.0):
        WORST[name] = ratio
        WORST_AT[name] = os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0]


def check_tiers(name, got, ref, S, n_terms, bias_mask=None, twin=None, bias=True, sink=None, bias_ceiling=None):
    """Hard tier always; bias tier where >= BIAS_MIN_N elements qualify (bias=False: report only); distribution + bias against
    the fp32-loop twin's statistics when ``twin`` (a stats() dict of the same tensor under CFFM_CONV_FP32=1) is given.
    bias_ceiling: a pinned bar for a tensor with a known, measured residual slope (it replaces BIAS_MAX / BIAS_MAX_B3; the sampling
    noise term still applies).  Returns the stats() dict of this tensor; ``sink[name]`` receives it before the bias and distribution
    tiers are asserted."""
    torch = _torch()
    g = t64(got, ref.device)
    err = (g - ref).abs()
    bound = (n_terms + 2) * U * S
    over = err > bound
    worst = float((err / torch.clamp(bound, min=1e-300)).max()) if err.numel() else 0.0
    _record('layer ' + name + ' (hard)', worst)
    assert not bool(over.any()), '%s: %d/%d elements beyond (n+2) u S (n = %d), worst |err| / bound %.3g at %s' % (
        name, int(over.sum()), over.numel(), n_terms, worst, np.unravel_index(int((err / torch.clamp(bound, min=1e-300)).argmax()),
                                                                             tuple(err.shape)))
    st = stats(g, ref, S, bias_mask)
    bar = max(BIAS_MAX, BIAS_SIGMAS * st['sigma_beta'])
    if twin is not None:                          # a slope the fp32 loop itself shows on this case is the hardware's, not the split's
        bar = max(bar, BIAS_MAX_B3 if bias_ceiling is None else bias_ceiling, 2.0 * abs(twin['beta']))
    elif bias_ceiling is not None:
        bar = max(bar, bias_ceiling)
    st['bias_bar'] = bar
    if sink is not None:
        sink[name] = st
    _record('layer ' + name + ' (|beta| / bar)', abs(st['beta']) / bar)
    if bias and st['n_beta'] >= BIAS_MIN_N:
        assert abs(st['beta']) <= bar, '%s: slope beta = %.3g over %d elements, bar %.3g (fp32 twin: %s)' % (
            name, st['beta'], st['n_beta'], bar, None if twin is None else '%.3g' % twin['beta'])
    if twin is not None:
        lim = DIST_FACTOR * twin['p999_u'] + DIST_SLACK
        _record('layer ' + name + ' (p99.9 / limit)', st['p999_u'] / lim)
        assert st['p999_u'] <= lim, '%s: 99.9th percentile of |err|/S = %.3f u, fp32 twin %.3f u (limit %.3f u)' % (
            name, st['p999_u'], twin['p999_u'], lim)
    return st


def exact_pads_zero(name, a, P):
    """Pad channels (P .. Pp-1) of a [.., Pp] device tensor are exactly 0."""
    if a.shape[-1] > P:
        pad = a[..., P:]
        assert bool((pad == 0).all()), '%s: %d nonzero pad-channel elements (max |.| %.3g)' % (
            name, int((pad != 0).sum()), float(pad.abs().max()))


def exact_relu_out(name, C):
    assert bool((C >= 0).all()), '%s: %d negative elements' % (name, int((C < 0).sum()))


def unpack_mask(words, rows, Pp):
    """ws.relu0 of one layer: [rows][Pp/16] 16-bit words, bit j of word q = channel 16 q + j -> bool [rows, Pp]."""
    torch = _torch()
    w = words.reshape(rows, Pp // 16).to(torch.int32) & 0xffff
    bits = torch.arange(16, device=w.device, dtype=torch.int32)
    return ((w[..., None] >> bits) & 1).bool().reshape(rows, Pp)


def exact_mask(name, words, C):
    """Every relu mask bit equals C > 0 (C: the device's [B,S,S,Pp] fp32 tensor)."""
    Pp = C.shape[-1]
    rows = C.numel() // Pp
    m = unpack_mask(words, rows, Pp)
    want = (C.reshape(rows, Pp) > 0)
    bad = m != want
    assert not bool(bad.any()), '%s: %d/%d relu mask bits differ from C > 0' % (name, int(bad.sum()), bad.numel())


def exact_gated_zero(name, dprev, prevC):
    """The input gradient is exactly 0 wherever the device's relu output C[l-1] is 0."""
    z = prevC == 0
    bad = z & (dprev != 0)
    assert not bool(bad.any()), '%s: %d elements nonzero where C[l-1] == 0' % (name, int(bad.sum()))
