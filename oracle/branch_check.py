"""Per-branch check of the inner branch and the head: every stage against a float64 evaluation of the fp32 tensors that stage read.

TEST INFRASTRUCTURE, like everything under oracle/: only tests/ may import it; the product path (cffm_amd/) never does.

oracle/parity.py starts from the ids, so its one tolerance has to cover every upstream rounding and every relu / max-pool decision
(inner_kink_slack, dout_slack, dense_grad_slack).  Here, as in layer_check.py for the conv stack, each stage is re-anchored on the
device's own inputs: the gathered rows and theta for the inner branch, ws.C[l] / ws.t1 / ws.h1 / ws.fb / ws.att / ws.inner_out / ws.out
/ ws.dout for the stages of the head.  Every reference returns the value and, per element, the scale S of its sum: the sum of the
absolute values of the terms of the form the device evaluates (bias included).  Everything is numpy: the largest case is B = 64 at F32 K64.

Activations.  act_model() is the fp32 function the model defines (constants rounded to fp32, argument rounded to fp32, the algebraic
form of common.hpp: elu = exp(x) - 1, selu = sa (exp(x) - 1), gelu = x (0.5 (1 + erf(x c)))), evaluated in the working precision: in
float64 for the references (layer_check.act32 evaluates the same definitions in float32, which would add the host libm's own rounding to
the reference), in float32 for the replays.  It also returns the scale of the form's terms (exp(x) + 1 for the negative elu arm, where
the subtraction cancels), which is what the S of a stage is built from.

Tiers (check()):
  exact      fb, sort keys, pad columns, gradients of a disabled branch (0), slabs without an example (0): asserted by the tests with
             array equality
  hard       |err| <= (n_terms + c) u S per element, u = 2^-24.  (n_terms - 1) u S is the rigorous bound of any summation order;
             c counts the fp32 roundings inside ONE term, counted per stage below from the kernel's arithmetic (C_* constants), with
             every device exp / erf / log call taken as DEV_ULP roundings
  floor      sums of n_terms >= FLOOR_MIN_TERMS: q = max |err| / (u S) (99.9th percentile above 10^5 elements) must not exceed
             FLOOR_FACTOR * q_replay + FLOOR_SLACK, q_replay being the same statistic of a float32 numpy replay of the stage in plain
             sequential order on the same inputs (never the device's).  The hard bound at n = 31,744 terms is 31,764 u S; a dropped
             unit moves inner_out by ~10 - 1000 u S; fp32 rounding of any order stays at ~1 u S.  Only this tier separates them.
  bias       as layer_check: beta = sum(err ref) / sum(ref^2) within max(BIAS_MAX, 4 sigma_beta) over >= BIAS_MIN_N non-zero elements
  decisions  relu'(z) of the 1x2 conv and the arg-max of the max-pool.  With the reference anchored on the device's rows, z is known
             to AMBIG_Z u S_z (S_z = |x0 w| + |x1 w| + |b| of the form's terms) and x to its own activation rounding.  A unit whose
             float64 |z| is below that, or whose x0, x1 differ by less than that rounding without being equal, is ambiguous: for it
             alone both decisions are accepted (the bound grows by |ref(A) - ref(B)|).  At most AMBIG_MAX of the units of a case may be
             ambiguous (asserted).  An exact tie is not ambiguous: the first element takes the gradient.

DEV_ULP: ROCm publishes a table of the ulp error of its device math functions, but it is not part of the installation this was
written on (no copy under the ROCm documentation directory), so DEV_ULP = 4 is a stated, UNVERIFIED constant: expf, erff and logf
are each assumed within 4 ulp of the correctly rounded value.

The floor constants (chosen on the CPU, tests/test_branch_check.py keeps the evidence and asserts the gap): see FLOOR_FACTOR below."""
import math

import numpy as np

from . import cffm_oracle as orc
from .layer_check import BIAS_MAX, BIAS_MIN_N, BIAS_SIGMAS, U, _record

try:
    from scipy.special import erf as _erf
except Exception:  # pragma: no cover
    _erf = np.vectorize(math.erf)

DEV_ULP = 4                    # assumed ulp error of device expf / erff / logf (unverified, see the module docstring)
FLOOR_MIN_TERMS = 256
# Chosen on the CPU over the cases of tests/test_branch_check.py (relu F32 K64, gelu F20 K64, elu F28 K32, selu F10 K32, prelu F5 at
# B = 300, two tie cases, the six losses at B = 300), statistics in u S:
#   passing   inner_out: sequential (= q_replay) 0.05 .. 2.8, numpy pairwise 0.005 .. 0.6, reverse order 0.03 .. 3.2.  Sums of terms of
#             one sign (pools, loss sums) sit higher, sequential 0.5 .. 10.4, and two orders of one sum differ by more than a factor:
#             the largest passing statistic relative to its limit is 0.79 (L of log_loss summed in reverse: 4.35 against q_replay 0.51).
#             That case fixes the slack: with FLOOR_SLACK = 2 it failed (limit 3.5).
#   failing   one unit dropped, counted twice or with its two dense weights swapped: inner_out off by 137 .. 9150 where the limits are
#             4.2 .. 8.1; the smallest is 33x its limit (elu F28 K32, last unit of the last pair dropped: 137 against 4.17).
# Smallest failing / largest passing, both relative to the limit: 42 (tests/test_branch_check.py::test_floor_gap asserts >= 3).
FLOOR_FACTOR = 3.0
FLOOR_SLACK = 4.0
AMBIG_Z = 3.0                  # z of the 1x2 conv is known to 3 u S_z (two products and two additions, one of them fused or not)
AMBIG_MAX = 1e-4

SELU_SCALE, SELU_SCALE_ALPHA, PRELU_ALPHA = orc.SELU_SCALE, orc.SELU_SCALE_ALPHA, orc.PRELU_ALPHA
LIP1 = {'relu': 1.0, 'elu': 1.0, 'prelu': 1.0, 'selu': float(np.float32(SELU_SCALE)), 'gelu': 1.13}   # max act' on [0, inf)
LIP2 = {'relu': 0.0, 'elu': 0.0, 'prelu': 0.0, 'selu': 0.0, 'gelu': 0.8}                              # max |act''| on [0, inf)

# roundings inside one term (D = DEV_ULP), from inner_body.hpp / head_body.hpp:
#   x = act(I): the device call against the reference's: D + 2 (exp, - 1, * sa; gelu: erf, 1 +, x *)            -> relative to xs
#   z = x0 w0 + x1 w1 + b: 4 roundings + the x's                                                                 -> (D + 6) u S_z
#   c = act_pos(relu(z)): D + 3 of its own; s = c + mp: 1; s * w: 1; the reference rounds r to fp32 once: 1
C_INNER_FWD = 2 * DEV_ULP + 12
C_INNER_DW = C_INNER_FWD + 1                    # * dout
#   dz = (dout * w) * act'(r): 1 + (2 D + 6: cdf + x pdf) + the second-order term (D + 6, its scale LIP2 S_z is part of S)
#   gcw term dz * x: + (D + 2) + 1
C_INNER_CW = 4 * DEV_ULP + 16
#   dEi term (dz0 w + dz1 w + dmp) * act'(I) * e: the dz's + 2 products + 2 additions + dmp (2) + act'(I) (2 D + 6) + 2 products
C_INNER_DEI = 5 * DEV_ULP + 26
C_POOL = DEV_ULP + 3                            # act_pos of one element
C_S0 = 3                                        # Eo * R and the two nested sums' own first terms
C_DENSE = 1
C_OUT = 3                                       # fb * att * lin_w (2), beta * (.) (1)
C_SOFTMAX = 2 * DEV_ULP + 6                     # exp of the numerator and of each denominator term, the division, z / lamda
C_LOSS = DEV_ULP + 4                            # per term: s + eps (its rounding moves the log by u: the |y| + |1 - y| part of S), log, the product, the sum
C_DOUT = DEV_ULP + 10                           # worst: hybrid, two divisions
C_HEAD_BWD = 12                                 # softmax backward: da, sda, dz, / lamda, dfb terms
#   dC[top] = dt1[off_top + y] * act'(C_top) where C_top > 0 (head_bwd_example): one term; act' as in dz above (2 D + 6: cdf + x pdf),
#   the product (1)
C_DCTOP = 2 * DEV_ULP + 7


# ---- activations ----------------------------------------------------------------------------------------------------------
def act_model(x, kind, dtype=np.float64):
    """(act(x), act'(x), scale of act's terms, scale of act''s terms, e) of the fp32 values x, in dtype.  e u bounds the difference
    between the device's fp32 act(x) and the float64 one: 0 where the fp32 result is exact (relu, prelu, the identity arm of elu)."""
    x = np.asarray(x).astype(np.float32).astype(dtype)
    if kind == 'relu':
        a = np.maximum(x, 0)
        g = (x > 0).astype(dtype)
        return a, g, np.abs(a), g, np.zeros(x.shape)
    if kind == 'prelu':
        a = np.maximum(x, 0) + dtype(PRELU_ALPHA) * (-np.maximum(-x, 0))
        g = (x > 0).astype(dtype) + dtype(PRELU_ALPHA) * (x < 0).astype(dtype)
        return a, g, np.abs(a), g, np.zeros(x.shape)
    if kind in ('elu', 'selu'):
        selu = kind == 'selu'
        sc = dtype(np.float32(SELU_SCALE)) if selu else dtype(1)
        sa = dtype(np.float32(SELU_SCALE_ALPHA)) if selu else dtype(1)
        e = np.exp(np.minimum(x, 0))
        neg = x < 0
        a = np.where(neg, sa * (e - dtype(1)), sc * x)
        g = np.where(neg, sa * e, sc)
        err = np.where(neg, float(sa) * DEV_ULP * e + (2 if selu else 1) * np.abs(a), np.abs(a) if selu else 0.0)
        return a, g, np.where(neg, sa * (e + dtype(1)), np.abs(a)), np.abs(g), np.asarray(err, np.float64)
    if kind == 'gelu':
        xc = x * dtype(np.float32(0.70710678118654752440))
        er = _erf(xc).astype(dtype)
        cdf = dtype(0.5) * (dtype(1) + er)
        pdf = np.exp(dtype(-0.5) * x * x) * dtype(np.float32(0.39894228040143267794))
        a, g = x * cdf, cdf + x * pdf
        cs = dtype(0.5) * (dtype(1) + np.abs(er))
        err = np.abs(x) * 0.5 * (DEV_ULP * np.abs(er) + 1.13 * np.abs(xc) + 1.0 + np.abs(er)) + np.abs(a)
        return a, g, np.abs(x) * cs, cs + np.abs(x) * pdf, np.asarray(err, np.float64)
    raise ValueError(kind)


def _sum(t, order, axis=-1):
    """Sum of t along axis in t's dtype: 'seq' plain sequential order, 'rev' the reverse, 'pair' numpy's pairwise sum."""
    t = np.moveaxis(t, axis, -1)
    if order == 'pair' or t.dtype == np.float64:
        return t.sum(-1)
    if order == 'rev':
        t = t[..., ::-1]
    return np.cumsum(t, axis=-1, dtype=t.dtype)[..., -1]


# ---- inner branch -----------------------------------------------------------------------------------------------------------
def inner_eval(E, cw, cb, dw, db, kind, dout=None, dtype=np.float64, order='seq', fault=None, side=None, dw_fwd=None):
    """The inner branch (CFFM.py:301-343) and its gradient from the rows E [B,F,K], the conv taps cw [4] (tap*2+ch), cb [2], the dense
    kernel dw [P*K] and bias db, all fp32, in dtype (float64: the reference, with the scales; float32: a replay / a numpy 'device').
    dw_fwd: another dense kernel for the forward sum only (tests: a dropped or doubled unit).  fault: 'no_relu', 'tie_second',
    'grad_from_x' (tests).  side: (kink_on bool [B,P,K2,2], first bool [B,P,K2]) decisions to force on the ambiguous units.
    Returns {name: value} and {name: S}; 'units' in the first holds z, S_z, x0, x1 and the ambiguity masks."""
    E = np.asarray(E, np.float32).astype(dtype)
    B, F, K = E.shape
    K2, P = K // 2, F * (F - 1) // 2
    ii, jj = orc.pair_index(F)
    w = np.asarray(cw, np.float32).astype(dtype).reshape(2, 2)               # [tap, ch]
    b2 = np.asarray(cb, np.float32).astype(dtype)
    wd = np.asarray(dw, np.float32).astype(dtype).reshape(P, K2, 2)
    wdf = wd if dw_fwd is None else np.asarray(dw_fwd, np.float32).astype(dtype).reshape(P, K2, 2)
    bd = dtype(np.float32(np.asarray(db).reshape(-1)[0]))
    Ei, Ej = E[:, ii, :], E[:, jj, :]
    I = Ei * Ej                                                              # exact in float64, one rounding in float32
    x, gx, xs, gxs, xe = act_model(I, kind, dtype)
    if fault == 'grad_from_x':
        gx = act_model(x, kind, dtype)[1]
    x0, x1, xs0, xs1 = x[..., 0::2], x[..., 1::2], xs[..., 0::2], xs[..., 1::2]
    z = x0[..., None] * w[0] + x1[..., None] * w[1] + b2                     # [B,P,K2,2]
    Sz = xs0[..., None] * np.abs(w[0]) + xs1[..., None] * np.abs(w[1]) + np.abs(b2)
    r = z if fault == 'no_relu' else np.maximum(z, 0)
    c, gr, _, grs, _ = act_model(r, kind, dtype)
    if fault == 'no_relu':
        on = np.ones(z.shape, bool)
    else:
        on = r > 0
        c = np.where(on, c, 0)
    kink = np.abs(z) < AMBIG_Z * U * Sz
    tie = (x0 != x1) & (np.abs(x0 - x1) < U * (xe[..., 0::2] + xe[..., 1::2]))
    first = x0 >= x1
    if fault == 'tie_second':
        first = x0 > x1
    if side is not None:
        on = np.where(kink, side[0], on)
        first = np.where(tie, side[1], first)
    mp = np.maximum(x0, x1)
    mps = np.maximum(xs0, xs1)
    s = c + mp[..., None]
    maybe_on = (z > -AMBIG_Z * U * Sz) | (fault == 'no_relu')
    ss = np.where(maybe_on, LIP1[kind] * Sz, 0) + mps[..., None]
    out = {'units': dict(z=z, Sz=Sz, x0=x0, x1=x1, kink=kink, tie=tie, s=s, ss=ss, n_units=z.size)}
    S = {}
    out['inner_out'] = _sum((s * wdf).reshape(B, -1), order) + bd
    S['inner_out'] = (ss * np.abs(wdf)).reshape(B, -1).sum(-1) + abs(bd)
    if dout is None:
        return out, S
    d = np.asarray(dout, np.float32).astype(dtype)
    d4 = d[:, None, None, None]
    out['dense_kernel'] = _sum(s * d4, order, axis=0).reshape(-1)
    S['dense_kernel'] = (ss * np.abs(d4)).sum(0).reshape(-1)
    out['dense_bias'] = _sum(d, order)
    S['dense_bias'] = np.abs(d).sum()
    ds = d4 * wd
    dz = ds * np.where(on, gr, 0)
    dzs = np.abs(ds) * np.where(on | kink, grs + LIP2[kind] * Sz, 0)
    xt, xts = np.stack([x0, x1], -1), np.stack([xs0, xs1], -1)               # [B,P,K2,tap]
    out['inner_layer_conv_weight_0'] = _sum((xt[..., :, None] * dz[..., None, :]).reshape(-1, 4).T, order)      # [tap*2+ch]
    S['inner_layer_conv_weight_0'] = (xts[..., :, None] * dzs[..., None, :]).reshape(-1, 4).sum(0)
    out['inner_layer_conv_bias_0'] = _sum(dz.reshape(-1, 2).T, order)
    S['inner_layer_conv_bias_0'] = dzs.reshape(-1, 2).sum(0)
    dmp, dmps = ds[..., 0] + ds[..., 1], np.abs(ds[..., 0]) + np.abs(ds[..., 1])
    dx0 = dz[..., 0] * w[0, 0] + dz[..., 1] * w[0, 1] + np.where(first, dmp, 0)
    dx1 = dz[..., 0] * w[1, 0] + dz[..., 1] * w[1, 1] + np.where(first, 0, dmp)
    dxs0 = dzs[..., 0] * abs(w[0, 0]) + dzs[..., 1] * abs(w[0, 1]) + np.where(first | tie, dmps, 0)
    dxs1 = dzs[..., 0] * abs(w[1, 0]) + dzs[..., 1] * abs(w[1, 1]) + np.where(~first | tie, dmps, 0)
    dI, dIs = np.empty_like(I), np.empty_like(I)
    dI[..., 0::2], dI[..., 1::2] = dx0 * gx[..., 0::2], dx1 * gx[..., 1::2]
    dIs[..., 0::2], dIs[..., 1::2] = dxs0 * gxs[..., 0::2], dxs1 * gxs[..., 1::2]
    dEi, dEs = np.zeros_like(E), np.zeros_like(E)
    pr = range(P - 1, -1, -1) if order == 'rev' else range(P)
    for p in pr:                                                             # partners in pair order (the device: its own fixed order)
        dEi[:, ii[p]] += dI[:, p] * Ej[:, p]
        dEi[:, jj[p]] += dI[:, p] * Ei[:, p]
        dEs[:, ii[p]] += dIs[:, p] * np.abs(Ej[:, p])
        dEs[:, jj[p]] += dIs[:, p] * np.abs(Ei[:, p])
    out['dEi'], S['dEi'] = dEi, dEs
    return out, S


INNER_TERMS = {           # name -> (n_terms, c) as functions of (B, F, K)
    'inner_out': lambda B, F, K: (F * (F - 1) // 2 * K + 1, C_INNER_FWD),
    'dense_kernel': lambda B, F, K: (B, C_INNER_DW),
    'dense_bias': lambda B, F, K: (B, 0),
    'inner_layer_conv_weight_0': lambda B, F, K: (B * F * (F - 1) // 2 * (K // 2), C_INNER_CW),
    'inner_layer_conv_bias_0': lambda B, F, K: (B * F * (F - 1) // 2 * (K // 2), C_INNER_CW),
    'dEi': lambda B, F, K: (F - 1, C_INNER_DEI),
}
INNER_BIAS = ('dEi', 'dense_kernel')


def ambiguous_units(units):
    """(count of ambiguous units, units) of a float64 inner_eval: relu kinks (per channel) and max-pool near-ties."""
    n = int(units['kink'].any(-1).sum() + (units['tie'] & ~units['kink'].any(-1)).sum())
    return n, units['tie'].size


def check_inner(name, got, E, cw, cb, dw, db, kind, dout=None, sink=None, only=None, orders=('seq',)):
    """Every tensor of ``got`` (name -> device value; names of INNER_TERMS) against the float64 reference of the same inputs, all
    tiers.  Returns {tensor: stats}; raises AssertionError listing every tensor that missed a tier."""
    ref, S = inner_eval(E, cw, cb, dw, db, kind, dout)
    n_amb, n_units = ambiguous_units(ref['units'])
    assert n_amb <= AMBIG_MAX * n_units, '%s: %d of %d units ambiguous (cap %g)' % (name, n_amb, n_units, AMBIG_MAX)
    extra = {}
    if n_amb and dout is not None:           # two-sided: every ambiguous decision taken the other way
        u = ref['units']
        alt, _ = inner_eval(E, cw, cb, dw, db, kind, dout, side=(~(u['z'] > 0), ~(u['x0'] >= u['x1'])))
        extra = {k: np.abs(alt[k] - ref[k]) for k in INNER_TERMS if k in alt}
    rep, _ = inner_eval(E, cw, cb, dw, db, kind, dout, dtype=np.float32)
    B, F, K = np.asarray(E).shape
    stats, fails = {'ambiguous': n_amb, 'units': n_units}, []
    for k, v in got.items():
        if only is not None and k not in only:
            continue
        n, c = INNER_TERMS[k](B, F, K)
        if k == 'inner_out':             # a term with a zero weight is 0 in every order: a unit probe is held to the bound of ONE term
            n = max(1, int(np.count_nonzero(dw)) + int(np.any(np.asarray(db) != 0)))
        try:
            stats[k] = check('%s %s' % (name, k), v, ref[k], S[k], n, c, replay=rep[k], extra=extra.get(k), bias=k in INNER_BIAS)
        except AssertionError as e:
            stats[k] = getattr(e, 'stats', {})
            fails.append(str(e))
    if sink is not None:
        sink.update(stats)
    assert not fails, '\n'.join(fails)
    return stats


# ---- the tiers --------------------------------------------------------------------------------------------------------------
def q_stat(err, S):
    """max |err| / (u S) over the elements with S > 0 (99.9th percentile above 10^5 elements)."""
    err, S = np.abs(np.asarray(err, np.float64)).reshape(-1), np.asarray(S, np.float64).reshape(-1)
    pos = S > 0
    if not pos.any():
        return 0.0
    r = err[pos] / (U * S[pos])
    return float(np.quantile(r, 0.999)) if r.size > 100000 else float(r.max())


def check(name, got, ref, S, n_terms, c, replay=None, extra=None, bias=False):
    """hard, floor (n_terms >= FLOOR_MIN_TERMS and a replay given) and bias tiers of one tensor; returns its statistics."""
    got = np.asarray(got, np.float64).reshape(np.shape(ref))
    ref, S = np.asarray(ref, np.float64), np.asarray(S, np.float64)
    assert np.isfinite(got).all(), '%s: %d non-finite elements' % (name, int((~np.isfinite(got)).sum()))
    err = got - ref
    bound = (n_terms + c) * U * S + (0.0 if extra is None else extra)
    zero = bound == 0
    ratio = np.where(zero, np.where(err == 0, 0.0, np.inf), np.abs(err) / np.where(zero, 1.0, bound))
    worst = float(ratio.max()) if ratio.size else 0.0
    st = {'hard': worst, 'n_terms': int(n_terms), 'q': q_stat(err - 0.0, S) if extra is None else q_stat(np.maximum(np.abs(err) - extra, 0), S)}
    _record('branch ' + name + ' (hard)', worst)
    fails = []
    if worst > 1.0:
        at = np.unravel_index(int(ratio.argmax()), ratio.shape) if ratio.ndim else ()
        fails.append('%s [hard]: %d/%d elements beyond (n + c) u S (n = %d, c = %d), worst |err| / bound %.3g at %s (|err| / (u S) = %.3g)'
                     % (name, int((ratio > 1).sum()), ratio.size, n_terms, c, worst, at, st['q']))
    if replay is not None and n_terms >= FLOOR_MIN_TERMS:
        st['q_replay'] = q_stat(np.asarray(replay, np.float64).reshape(ref.shape) - ref, S)
        lim = FLOOR_FACTOR * st['q_replay'] + FLOOR_SLACK
        _record('branch ' + name + ' (q / floor limit)', st['q'] / lim)
        if st['q'] > lim:
            fails.append('%s [floor]: q = %.3g u S, sequential fp32 replay %.3g (limit %.3g)' % (name, st['q'], st['q_replay'], lim))
    m = ref != 0
    if bias and int(m.sum()) >= BIAS_MIN_N:
        den = float((ref[m] ** 2).sum())
        beta = float((err[m] * ref[m]).sum()) / den
        sigma = math.sqrt(float(((err[m] * ref[m]) ** 2).sum())) / den
        bar = max(BIAS_MAX, BIAS_SIGMAS * sigma)
        st['beta'], st['bias_bar'] = beta, bar
        _record('branch ' + name + ' (|beta| / bar)', abs(beta) / bar)
        if abs(beta) > bar:
            fails.append('%s [bias]: slope beta = %.3g over %d elements, bar %.3g' % (name, beta, int(m.sum()), bar))
    st['fails'] = [f.split('[')[1].split(']')[0] for f in fails]
    if fails:
        e = AssertionError('\n'.join(fails))
        e.stats = st
        raise e
    return st


# ---- head: one function per stage, (value, S) in dtype ---------------------------------------------------------------------
def _f(x, dtype):
    return np.asarray(x, np.float32).astype(dtype)


def pool_stage(C, kind, dtype=np.float64, order='seq'):
    """Sum pool of act(C_l) per (example, row): C [B,S,S,P] (>= 0) -> [B,S]; n_terms = S P."""
    a, _, s, _, _ = act_model(C, kind, dtype)
    B, S_ = a.shape[0], a.shape[1]
    return _sum(a.reshape(B, S_, -1), order), s.reshape(B, S_, -1).sum(-1)


def s0_stage(Eo, dtype=np.float64, order='seq'):
    """s0[h] = sum_i Eo[i][h] * sum_{j>i} rowsum(j) (head_body.hpp; the closed form of the pool of the outer-product map, CFFM.py:381);
    S from that form's terms; n_terms = 2 F + D."""
    E = _f(Eo, dtype)
    rs, rss = _sum(E, order), np.abs(E).sum(-1)                              # [B,F]
    R = np.cumsum(rs[:, ::-1], axis=1, dtype=dtype)[:, ::-1]                 # R_i' = sum_{j >= i} rs[j]
    Rs = np.cumsum(rss[:, ::-1], axis=1)[:, ::-1]
    t = E[:, :-1, :] * R[:, 1:, None]                                        # i = 0 .. F-2 with sum_{j > i}
    if order != 'rev':
        t = t[:, ::-1]                                                       # the device runs i = F-2 .. 0
    return _sum(t, order, axis=1), (np.abs(E[:, :-1, :]) * Rs[:, 1:, None]).sum(1)


def dense_stage(x, W, b, dtype=np.float64, order='seq'):
    """x @ W + b with S; n_terms = x.shape[1] + 1."""
    x, W, b = _f(x, dtype), _f(W, dtype), _f(b, dtype)
    v = _sum(x[:, :, None] * W[None], order, axis=1) + b
    return v, np.abs(x) @ np.abs(W) + np.abs(b)


def att_stage(fb, W, b, lam, dtype=np.float64, order='seq', fault=None):
    """softmax((fb @ W + b) / lamda_att) with its max subtracted (CFFM.py:432-436).  S = att (2 max_f S_z / lamda + 1): the relative
    error of exp(z - max) is the absolute error of z - max; n_terms = F + 3 (the sums of z and of the denominator)."""
    z, Sz = dense_stage(fb, W, b, dtype, order)
    lam = dtype(np.float32(lam))
    if fault != 'no_lamda':
        z = z / lam
    Sz = Sz / abs(lam)
    e = np.exp(z - z.max(1, keepdims=True))
    at = e / _sum(e, order)[:, None]
    return at, at * (2.0 * Sz.max(1, keepdims=True) + 1.0)


def out_stage(io, h1, att, fb, prm, cfg, dtype=np.float64, order='seq', fault=None):
    """out = inner_out + beta (h1 . d2_w + d2_b) + (fb att) . lin_w + lin_b (or sum fb) + bias (CFFM.py:410-453), raw (before the
    sigmoid of log_loss).  n_terms = 32 + F + 5."""
    B = np.asarray(fb).shape[0]
    out, S = np.zeros(B, dtype), np.zeros(B)
    if cfg.inner_conv:
        out = out + _f(io, dtype)
        S = S + np.abs(_f(io, np.float64))
    if cfg.outer_conv:
        o, So = dense_stage(h1, np.asarray(prm['dense_2_kernel']).reshape(-1, 1), np.asarray(prm['dense_2_bias']).reshape(1), dtype, order)
        if fault == 'd2b_twice':
            o = o + _f(prm['dense_2_bias'], dtype).reshape(1)
        beta = dtype(np.float32(cfg.beta_outer)) if fault != 'no_beta' else dtype(1)
        out = out + beta * o[:, 0]
        S = S + abs(float(np.float32(cfg.beta_outer))) * So[:, 0]
    f = _f(fb, dtype)
    if cfg.linear_att:
        g = f * _f(att, dtype)
        lin, Sl = dense_stage(g, np.asarray(prm['dense_3_kernel']).reshape(-1, 1), np.asarray(prm['dense_3_bias']).reshape(1), dtype, order)
        out, S = out + lin[:, 0], S + Sl[:, 0]
    else:
        out, S = out + _sum(f, order), S + np.abs(f).sum(1)
    b = dtype(np.float32(np.asarray(prm['bias']).reshape(-1)[0]))
    return out + b, S + abs(b)


EPS = np.float32(1e-7)


def loss_stage(out, y, loss, B_global, dtype=np.float64, order='seq', unscaled=False, fault=None, eval_in=True):
    """Per-example loss terms, their sum and L (CFFM.py:486-513) from ws.out (log_loss: the sigmoid the forward stored) and y.
    Returns {'sqerr', 'sum', 'L'} and their S.  'hybrid': sqerr is (y - out)^2 as the forward writes it; L takes its two sums."""
    o, yy = _f(out, dtype), _f(y, dtype)
    eps = dtype(EPS) if fault != 'no_eps' else dtype(0)
    one, half = dtype(1), dtype(0.5)
    invB = dtype(np.float32(1.0) / np.float32(B_global))
    d = yy - o
    if loss == 'mae':
        t, ts = np.abs(d), np.abs(yy) + np.abs(o)
    elif loss == 'square_l2':
        t, ts = half * d * d, half * (np.abs(yy) + np.abs(o)) ** 2
    elif loss == 'log_loss':
        a, b = np.log(o + eps), np.log(one - o + eps)
        t, ts = -(yy * a + (one - yy) * b), np.abs(yy * a) + np.abs((one - yy) * b) + np.abs(yy) + np.abs(one - yy)
    else:
        t, ts = d * d, (np.abs(yy) + np.abs(o)) ** 2
    v, S = {'sqerr': t}, {'sqerr': ts}
    v['sum'], S['sum'] = _sum(t, order), ts.sum()
    if loss == 'hybrid':
        sq, sqs = half * d * d, half * (np.abs(yy) + np.abs(o)) ** 2
        a, b = np.log(o + eps), np.log(one - o + eps)
        lg, lgs = -(yy * a + (one - yy) * b), np.abs(yy * a) + np.abs((one - yy) * b) + np.abs(yy) + np.abs(one - yy)
        s1, s2 = _sum(sq, order), _sum(lg, order)
        if fault == 'hybrid_norms':
            v['L'] = half * s1 * invB + half * s2
        else:
            v['L'] = half * s1 + half * s2 * invB
        S['L'] = 0.5 * sqs.sum() + 0.5 * lgs.sum() * float(invB)
    elif loss == 'square_loss':
        v['L'] = dtype(1) if unscaled else np.sqrt(v['sum'] * invB + dtype(np.float32(1e-10)))
        S['L'] = 1.0 if unscaled else 0.5 * float(S['sum'] * invB + 1e-10) / max(float(np.sqrt(float(v['sum']) * float(invB) + 1e-10)), 1e-300) + abs(float(v['L']))
    elif loss == 'square_l2':
        v['L'], S['L'] = v['sum'], S['sum']
    else:
        v['L'], S['L'] = v['sum'] * invB, S['sum'] * float(invB)
    return v, S


def dout_stage(out, y, L, loss, B_global, dtype=np.float64, unscaled=False):
    """dL/dout (common.hpp head_dout) from ws.out, y and the device's own L; S from the form's terms (no cancellation is excused:
    out - y is an exact-or-one-rounding difference of the two fp32 inputs)."""
    o, yy = _f(out, dtype), _f(y, dtype)
    invB = dtype(np.float32(1.0) / np.float32(B_global))
    Lv = dtype(np.float32(L))
    one, half, eps = dtype(1), dtype(0.5), dtype(EPS)
    d = o - yy
    if loss == 'square_loss':
        v = d * invB if unscaled else d * invB / Lv
        return v, np.abs(v)
    if loss == 'mse':
        return dtype(2) * d * invB, 2 * np.abs(d) * float(invB)
    if loss == 'mae':
        return np.sign(d) * invB, np.full(d.shape, float(invB))
    if loss == 'square_l2':
        return d, np.abs(d)
    a, b = yy / (o + eps), (one - yy) / (one - o + eps)
    if loss == 'hybrid':
        return half * d - half * invB * (a - b), 0.5 * np.abs(d) + 0.5 * float(invB) * (np.abs(a) + np.abs(b))
    v = -(a - b) * invB * o * (one - o)
    return v, (np.abs(a) + np.abs(b)) * float(invB) * np.abs(o * (one - o))


def head_bwd_stage(dout, fwd, prm, cfg, dtype=np.float64, order='seq'):
    """dt1, dfb and the nine head gradients from ws.dout and the forward tensors fwd = {t1, h1, att, fb} (head_body.hpp
    head_bwd_example / head_bwd_end).  Returns {name: value}, {name: S}, {name: (n_terms, c)}."""
    d = _f(dout, dtype)
    B = d.shape[0]
    v, S, T = {}, {}, {}
    v['bias'], S['bias'], T['bias'] = _sum(d, order), np.abs(d).sum(), (B, 0)
    F = cfg.F
    if cfg.outer_conv:
        beta = dtype(np.float32(cfg.beta_outer))
        dd = d * beta
        w2 = _f(np.asarray(prm['dense_2_kernel']).reshape(-1), dtype)
        W1 = _f(prm['dense_1_kernel'], dtype)
        t1, h1 = _f(fwd['t1'], dtype), _f(fwd['h1'], dtype)
        dh1 = dd[:, None] * w2[None]
        v['dense_2_bias'], S['dense_2_bias'], T['dense_2_bias'] = _sum(dd, order), np.abs(dd).sum(), (B, 1)
        v['dense_2_kernel'], S['dense_2_kernel'], T['dense_2_kernel'] = _sum(h1 * dd[:, None], order, 0), (np.abs(h1) * np.abs(dd)[:, None]).sum(0), (B, 2)
        v['dense_1_bias'], S['dense_1_bias'], T['dense_1_bias'] = _sum(dh1, order, 0), np.abs(dh1).sum(0), (B, 2)
        v['dense_1_kernel'] = _sum(t1[:, :, None] * dh1[:, None, :], order, 0)
        S['dense_1_kernel'], T['dense_1_kernel'] = np.einsum('bk,bq->kq', np.abs(t1), np.abs(dh1)), (B, 3)
        v['dt1'] = _sum(dh1[:, None, :] * W1[None], order)
        S['dt1'], T['dt1'] = np.abs(dh1) @ np.abs(W1).T, (32, 3)
    fb = _f(fwd['fb'], dtype)
    if cfg.linear_att:
        at = _f(fwd['att'], dtype)
        lw = _f(np.asarray(prm['dense_3_kernel']).reshape(-1), dtype)
        W = _f(prm['bias_W'], dtype)
        lam = dtype(np.float32(cfg.lamda_att))
        dg = d[:, None] * lw[None]
        da = dg * fb
        sda = _sum(da * at, order)[:, None]
        dz = at * (da - sda) / lam
        dzs = np.abs(at) * (np.abs(da) + (np.abs(da * at)).sum(1, keepdims=True)) / abs(lam)
        v['dfb'] = dg * at + _sum(dz[:, None, :] * W[None], order)
        S['dfb'], T['dfb'] = np.abs(dg * at) + dzs @ np.abs(W).T, (2 * F + 1, C_HEAD_BWD)
        v['dense_3_bias'], S['dense_3_bias'], T['dense_3_bias'] = _sum(d, order), np.abs(d).sum(), (B, 0)
        v['dense_3_kernel'], S['dense_3_kernel'], T['dense_3_kernel'] = _sum(fb * at * d[:, None], order, 0), np.abs(fb * at * d[:, None]).sum(0), (B, 2)
        v['bias_b'], S['bias_b'], T['bias_b'] = _sum(dz, order, 0), dzs.sum(0), (B + F, C_HEAD_BWD)
        v['bias_W'] = _sum(fb[:, :, None] * dz[:, None, :], order, 0)
        S['bias_W'], T['bias_W'] = np.einsum('bf,bg->fg', np.abs(fb), dzs), (B + F, C_HEAD_BWD)
    else:
        v['dfb'], S['dfb'], T['dfb'] = np.broadcast_to(d[:, None], fb.shape).copy(), np.broadcast_to(np.abs(d)[:, None], fb.shape).copy(), (1, 0)
    return v, S, T


HEAD_BIAS = ('h1', 'dt1')


def _t1_off(D, l):
    return sum(D >> i for i in range(l))


def check_head(name, dev, prm, cfg, loss, y=None, B_global=None, unscaled=False, sink=None):
    """Every stage of the head that ``dev`` holds outputs of, each against the reference of the inputs ``dev`` holds for it.
    dev: 'C' (list of [B,S,S,P] conv outputs without pads), 'Eo', 'pool' (list of partial pools or None), 't1', 'h1', 'fb', 'att',
    'inner_out', 'out', 'sqerr', 'sum', 'L', 'dout', 'dt1', 'dfb' and the head gradients by variable name; loss: a key of
    cffm_amd.hip.LOSS_IDS or 'square_l2'.  Returns {tensor: stats}; raises AssertionError listing every tensor that missed a tier."""
    D, F = cfg.D, cfg.F
    stats, fails = {}, []

    def tier(k, got, pair, n, c, rep=None, bias=False):
        try:
            stats[k] = check('%s %s' % (name, k), got, pair[0], pair[1], n, c, replay=None if rep is None else rep[0], bias=bias)
        except AssertionError as e:
            stats[k] = getattr(e, 'stats', {})
            fails.append(str(e))

    f32 = np.float32
    if cfg.outer_conv and 't1' in dev:
        t1 = np.asarray(dev['t1'])
        if 'Eo' in dev:
            tier('t1 s0', t1[:, :D], s0_stage(dev['Eo']), 2 * F + D, C_S0)
        for l, C in enumerate(dev.get('C', [])):
            So = D >> (l + 1)
            ref = pool_stage(C, cfg.activation)
            rep = pool_stage(C, cfg.activation, f32)
            n = So * C.shape[-1]
            tier('t1 pool %d' % (l + 1), t1[:, _t1_off(D, l + 1):_t1_off(D, l + 1) + So], ref, n, C_POOL, rep)
            if dev.get('pool') and dev['pool'][l] is not None:
                tier('pool partials %d' % (l + 1), np.asarray(dev['pool'][l], np.float64).sum(-1), ref, n, C_POOL, rep)
        if 'h1' in dev:
            a = (t1, prm['dense_1_kernel'], prm['dense_1_bias'])
            tier('h1', dev['h1'], dense_stage(*a), 2 * D - 1, C_DENSE, bias=True)
    if cfg.linear_att and 'att' in dev:
        tier('att', dev['att'], att_stage(dev['fb'], prm['bias_W'], prm['bias_b'], cfg.lamda_att), F + 3, C_SOFTMAX)
    if 'out' in dev:
        raw, S = out_stage(dev.get('inner_out'), dev.get('h1'), dev.get('att'), dev['fb'], prm, cfg)
        if loss == 'log_loss':
            with np.errstate(over='ignore'):
                sg = 1.0 / (1.0 + np.exp(-raw))
            raw, S = sg, S * sg * (1 - sg) + sg
        tier('out', dev['out'], (raw, S), 37 + F, C_OUT + (DEV_ULP + 3 if loss == 'log_loss' else 0))
    if 'sqerr' in dev:
        B = np.asarray(dev['out']).shape[0]
        Bg = B if B_global is None else B_global
        v, S = loss_stage(dev['out'], y, loss, Bg, unscaled=unscaled)
        rep, _ = loss_stage(dev['out'], y, loss, Bg, f32, unscaled=unscaled)
        tier('sqerr', dev['sqerr'], (v['sqerr'], S['sqerr']), 2, C_LOSS)
        if 'sum' in dev:
            tier('loss sum', dev['sum'], (v['sum'], S['sum']), B, C_LOSS, (rep['sum'],))
        if 'L' in dev:
            tier('L', dev['L'], (v['L'], S['L']), B + 2, C_LOSS + 3, (rep['L'],))
    if 'dout' in dev:
        B = np.asarray(dev['out']).shape[0]
        Bg = B if B_global is None else B_global
        tier('dout', dev['dout'], dout_stage(dev['out'], y, dev.get('L', 1.0), loss, Bg, unscaled=unscaled), 3, C_DOUT)
        v, S, T = head_bwd_stage(dev['dout'], dev, prm, cfg)
        rep, _, _ = head_bwd_stage(dev['dout'], dev, prm, cfg, f32)
        for k in v:
            if k in dev or k in ('dt1', 'dfb'):
                if k in dev:
                    tier(('grad ' + k) if k not in ('dt1', 'dfb') else k, dev[k], (v[k], S[k]), T[k][0], T[k][1], (rep[k],), bias=k in HEAD_BIAS)
    if sink is not None:
        sink.update(stats)
    assert not fails, '\n'.join(fails)
    return stats
