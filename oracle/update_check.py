"""Per-step check of the parameter update (cffm_amd/csrc/optim.hip) against a float64 replay of its own inputs.

TEST INFRASTRUCTURE, like everything under oracle/: only tests/ may import it; the product path (cffm_amd/) never does.

The end-to-end checks (oracle/parity.py) compare a whole step with the oracle, so they must widen the parameter bound by
what the gradient's own tolerance does to the update - and Adagrad's first step from an accumulator of 1e-8 is about
lr * sign(g), so that widening can reach lr and hides a wrong gradient scale, a dropped duplicate or a split segment.  Here
the update alone is replayed: in float64 from the exact fp32 inputs the kernel consumed (the dense gradient, the row
gradients and their ids, the loss-term sum of the late scale) and the device's own pre-step parameters and slots.  The rules
are element-wise, so there are no percentile tiers: every element must lie within a rigorous bound.

Error model (u = 2^-24).  hipcc contracts a*b + c to an FMA by default and the Makefile sets neither fast-math nor the
approximate division / square root, so every fp32 operation the kernels perform ('/', sqrtf included) is correctly rounded:
<= 1 u relative, an FMA counting as one operation (bounding it as two is only looser).
  duplicates   the n row gradients of one id are summed in slot order: |fl(sum) - sum| <= gamma_{n-1} * sum_k |g_k| with
               gamma_k = k u / (1 - k u), for any summation order; n = 1 is exact.  The dense gradient is an input (n = 1).
  late scale   s = 1 / sqrtf(sum * (1/Bg) + 1e-10f) of the data-parallel apply: three roundings under the root (reciprocal,
               product, sum; all terms >= 0) are <= 3 u relative, halved by the root, plus the root and the division:
               <= 3.5 u, LATE_U = 4.  Then g = fl(fl(sum) * s): dg = s gamma_{n-1} A (1 + LATE_U u) + (LATE_U + 1) u |g|.
               The loss it writes, sqrtf(x) (rmse) or sum * (1/Bg) (mse): <= 2.5 u, LOSS_U = 3.
  l2 term      g = fl(G + lamda * w): + 2 u (|G| + |lamda w|).
  after g      each rule then runs a few operations, each <= 1 u; the sum's error dg is propagated through the exact rule:
    Adagrad    a = a0 + g^2 (2 roundings): |da| <= (2|g| dg + dg^2)(1 + 4u) + 3 u a.  The move q(g) = lr g / sqrt(a0 + g^2) is
               monotone in g, so max |q(g +- dg) - q(g)| bounds what dg does to it exactly (no first-order guess); q itself
               takes 4 roundings (a, sqrt, lr*g, '/': the 2 u of a are halved by the root) and w - q one more:
               |dw| <= dq (1 + 8u) + 6 u |q| + 2 u |w|.
    SGD        |dw| <= lr dg (1 + 4u) + 2 u |lr g| + 2 u |w|        (lr * g, w - p: 2 roundings)
    Momentum   a = 0.95f a0 + g: |da| <= dg (1 + 4u) + 3 u (|0.95f a0| + |g|); |dw| <= lr |da| (1 + 4u) + 2 u |lr a| + 2 u |w|
    Adam       m = b1 m0 + (1-b1) g: |dm| <= (1-b1) dg (1 + 4u) + 4 u (|b1 m0| + |(1-b1) g|);
               v = b2 v0 + (1-b2) g g: |dv| <= (1-b2)(2|g| dg + dg^2)(1 + 4u) + 5 u (b2 v0 + (1-b2) g^2);
               q = lr_t m / (sqrtf(v) + eps): the root moves by ds <= min(sqrt(dv), dv / sqrt(v)), the denominator stays
               >= sqrt(v) + eps - ds, and q takes 4 roundings: |dw| <= dq (1 + 8u) + 6 u |q| + 2 u |w|.
The second-order terms the constants round up (products of two relative errors, each <= gamma_8191 < 5e-4 here) are below
1e-3 of the first-order ones; every constant above is at least 1 u or 1.5x over its first-order count.

Constants are the device's: (float)lr, (float)lamda, 0.95f, 0.9f / 0.999f, 1 - beta rounded once from double, 1e-8f, 1e-10f,
and Adam's lr_t = (float)((double)(float)lr * sqrt(1 - 0.999^t) / (1 - 0.9^t)), rounded once.  The values come from the
oracle's own statements of the rules (cffm_oracle.adagrad_dense / adagrad_sparse / apply_optimizer); the bounds from the model
above.  Exact checks (bit for bit): rows nobody looked up and their slots (Adagrad, SGD, Momentum), a disabled branch's table
and slots, elements whose dense gradient is exactly 0 (Adagrad: the conv channel pads)."""
import types

import numpy as np

from . import cffm_oracle as orc

U = 2.0 ** -24
LATE_U = 4
LOSS_U = 3
LATE_EPS = float(np.float32(1e-10))
WORST = {}


def f32(x):
    return float(np.float32(x))


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def adam_lr_t(lr, t):
    """lr_t as cffm_apply_opt computes it: in double from the float lr, rounded to float once."""
    return f32(np.float64(f32(lr)) * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t))


DEVICE_CONSTS = dict(b1=f32(0.9), b2=f32(0.999), omb1=f32(1.0 - 0.9), omb2=f32(1.0 - 0.999), eps=f32(1e-8), mom=f32(0.95))

TABLES = (('inner', 'inner_embeddings', 'dEi', 'd_inner_rows'), ('outer', 'outer_embeddings', 'dEo', 'd_outer_rows'),
          ('fbias', 'feature_bias', 'dfb', 'd_bias_rows'))


def seg_sums(ids, rows, M):
    """Per-row duplicate sums of the row gradients in float64: (G [M, C], A = sum |g_k| [M, C], n [M]); ids outside [0, M)
    are skipped, as every update kernel skips them."""
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    rows = np.asarray(rows, dtype=np.float64).reshape(ids.shape[0], -1)
    ok = (ids >= 0) & (ids < M)
    G = np.zeros((M, rows.shape[1]))
    A = np.zeros((M, rows.shape[1]))
    n = np.zeros(M, dtype=np.int64)
    np.add.at(G, ids[ok], rows[ok])
    np.add.at(A, ids[ok], np.abs(rows[ok]))
    np.add.at(n, ids[ok], 1)
    return G, A, n


# ---- bounds of one rule, element-wise, given the exact gradient g and the bound dg on the device's gradient --------------
def adagrad_bounds(w, a0, g, dg, lr):
    with np.errstate(divide='ignore', invalid='ignore'):
        Q = lambda x: lr * x / np.sqrt(a0 + x * x)
        q = Q(g)
        dq = np.maximum(np.abs(Q(g + dg) - q), np.abs(Q(g - dg) - q))
    ba = (2 * np.abs(g) * dg + dg * dg) * (1 + 4 * U) + 3 * U * (a0 + g * g)
    bw = dq * (1 + 8 * U) + 6 * U * np.abs(q) + 2 * U * np.abs(w)
    return bw, ba


def sgd_bounds(w, g, dg, lr):
    return lr * dg * (1 + 4 * U) + 2 * U * np.abs(lr * g) + 2 * U * np.abs(w)


def momentum_bounds(w, a, a0, g, dg, lr, mom):
    ba = dg * (1 + 4 * U) + 3 * U * (np.abs(mom * a0) + np.abs(g))
    bw = lr * ba * (1 + 4 * U) + 2 * U * np.abs(lr * a) + 2 * U * np.abs(w)
    return bw, ba


def adam_bounds(w, m, v, m0, v0, g, dg, lr_t, c):
    bm = c['omb1'] * dg * (1 + 4 * U) + 4 * U * (np.abs(c['b1'] * m0) + np.abs(c['omb1'] * g))
    bv = c['omb2'] * (2 * np.abs(g) * dg + dg * dg) * (1 + 4 * U) + 5 * U * (c['b2'] * v0 + c['omb2'] * g * g)
    sv = np.sqrt(v)
    with np.errstate(divide='ignore', invalid='ignore'):
        ds = np.minimum(np.sqrt(bv), np.where(sv > 0, bv / sv, np.inf))
    den = sv + c['eps']
    den_lo = np.maximum(den - ds, c['eps'])
    q = lr_t * m / den
    dq = lr_t * (bm / den_lo + np.abs(m) * ds / (den * den_lo))
    bw = dq * (1 + 8 * U) + 6 * U * np.abs(q) + 2 * U * np.abs(w)
    return bw, bm, bv


# ---- the replay ---------------------------------------------------------------------------------------------------------
def _f64(x):
    return None if x is None else np.asarray(x, dtype=np.float64)


def replay(opt, pre, grad, ids, rows, M, lr, lamda=0.0, lamda_att=0.0, late=None, t=None):
    """float64 replay of one update.

    pre   {'theta': [n], 'inner': [M, K], 'outer': [M, D], 'fbias': [M], 's1': {same keys}, 's2': {same keys} (Adam)}: the
          device's fp32 state before the update (s1: Adagrad / Momentum accumulator, Adam m; s2: Adam v)
    grad  the dense gradient [n] the kernel read (fp32), or None (no dense update)
    ids   [N] ids of the row gradients; rows {'dEi': [N, K] | None, 'dEo': [N, D] | None, 'dfb': [N]} (None: a disabled
          branch, its table is not updated)
    late  None, or (loss_sum, Bg, rmse): the data-parallel apply (1/L applied to every gradient when rmse)
    lamda > 0: the regularised square loss (both tables dense, g = G + lamda * w, lamda_att for the outer table)
    t     Adam's step (1-based)

    Returns {'vars': {name: {'w', 'bw', 's1', 'bs1', 's2', 'bs2', 'moved'}}, 'loss': (ref, bound) | None}: reference values,
    bounds, and 'moved' = the rows the rule may change (the others must be bit-identical to pre)."""
    lr = f32(lr)
    lam = {'inner': f32(lamda), 'outer': f32(lamda_att), 'fbias': 0.0}
    l2 = lamda > 0
    s, loss = 1.0, None
    if late is not None:
        lsum, Bg, rmse = float(late[0]), int(late[1]), bool(late[2])
        x = lsum / Bg + LATE_EPS
        if rmse:
            s = 1.0 / np.sqrt(x)
            loss = (np.sqrt(x), LOSS_U * U * np.sqrt(x))
        else:
            loss = (lsum / Bg, LOSS_U * U * abs(lsum / Bg))
    ls = late is not None and s != 1.0
    parts = {}                                  # name -> (w0, g, dg, moved rows)
    if grad is not None:
        g = _f64(grad) * s
        dg = (LATE_U + 1) * U * np.abs(g) if ls else np.zeros_like(g)
        parts['theta'] = (_f64(pre['theta']), g, dg, None)
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    for name, _, rkey, _ in TABLES:
        r = rows.get(rkey)
        w0 = _f64(pre[name]).reshape(M, -1)
        if r is None:
            parts[name] = (w0, None, None, np.zeros(M, dtype=bool))
            continue
        G, A, n = seg_sums(ids, r, M)
        g = G * s
        dg = s * gamma(np.maximum(n - 1, 0))[:, None] * A * (1 + LATE_U * U)
        if ls:
            dg = dg + (LATE_U + 1) * U * np.abs(g)
        moved = n > 0
        if lam[name] != 0.0 and l2:
            dg = dg + 2 * U * (np.abs(g) + np.abs(lam[name] * w0))
            g = g + lam[name] * w0
            moved = np.ones(M, dtype=bool)
        if opt == 'AdamOptimizer':
            moved = np.ones(M, dtype=bool)
        parts[name] = (w0, g, dg, moved)
    out = {}
    if opt == 'AdagradOptimizer':
        _replay_adagrad(parts, pre, ids, rows, M, lr, s, l2, lam, out)
    else:
        _replay_other(opt, parts, pre, ids, rows, M, lr, l2, lamda, lamda_att, t, out)
    return {'vars': out, 'loss': loss}


def _replay_adagrad(parts, pre, ids, rows, M, lr, s, l2, lam, out):
    ok = (ids >= 0) & (ids < M)
    for name, (w0, g, dg, moved) in parts.items():
        a0 = _f64(pre['s1'][name]).reshape(w0.shape)
        if g is None:
            out[name] = dict(w=w0, bw=0 * w0, s1=a0, bs1=0 * a0, moved=moved)
            continue
        w, a = w0.copy(), a0.copy()
        if name == 'theta' or (l2 and lam[name] != 0.0):
            orc.adagrad_dense(w, a, g, lr)                  # dense: g = s * grad, or G + lamda * w of the regularised loss
        else:
            rk = [k for n_, _, k, _ in TABLES if n_ == name][0]
            r = np.asarray(rows[rk], dtype=np.float64).reshape(ids.shape[0], -1)
            orc.adagrad_sparse(w, a, ids[ok], r[ok] * s, lr)     # duplicates summed first, untouched rows left alone
        bw, ba = adagrad_bounds(w, a0, g, dg, lr)
        if name == 'theta':
            moved = g != 0                                  # a zero gradient leaves w and acc bit-identical (the pads)
        out[name] = dict(w=w, bw=bw, s1=a, bs1=ba, moved=moved)


def _replay_other(opt, parts, pre, ids, rows, M, lr, l2, lamda, lamda_att, t, out):
    names = {n_: full for n_, full, _, _ in TABLES}
    names['theta'] = 'theta'
    c = dict(DEVICE_CONSTS)
    lr_t = adam_lr_t(lr, t) if opt == 'AdamOptimizer' else None
    if lr_t is not None:
        c['lr_t'] = lambda tt: lr_t
    cfg = types.SimpleNamespace(optimizer=opt, lr=lr, loss_type='square_loss', lamda_bilinear=f32(lamda) if l2 else 0.0,
                                lamda_att=f32(lamda_att))
    p = {names[k]: v[0].copy() for k, v in parts.items()}
    g = {}
    if 'theta' in parts:
        g['theta'] = parts['theta'][1]
    ok = (ids >= 0) & (ids < M)                             # ids outside [0, M) are skipped
    for name, full, rkey, gkey in TABLES:
        if rows.get(rkey) is not None:
            g[gkey] = np.asarray(rows[rkey], dtype=np.float64).reshape(ids.shape[0], -1)[ok]
    s1 = {names[k]: _f64(pre['s1'][k]).reshape(v[0].shape) for k, v in parts.items()}
    if opt == 'AdamOptimizer':
        st = {'m': {k: v.copy() for k, v in s1.items()}, 't': t - 1,
              'v': {names[k]: _f64(pre['s2'][k]).reshape(v[0].shape) for k, v in parts.items()}}
        v0 = {k: v.copy() for k, v in st['v'].items()}
    elif opt == 'MomentumOptimizer':
        st = {'acc': {k: v.copy() for k, v in s1.items()}}
    else:
        st = {}
    orc.apply_optimizer(p, st, g, ids[ok], cfg, consts=c)
    for name, (w0, gg, dg, moved) in parts.items():
        k = names[name]
        if gg is None:
            out[name] = dict(w=w0, bw=0 * w0, s1=s1[k], bs1=0 * w0, moved=moved)
            if opt == 'AdamOptimizer':
                out[name].update(s2=v0[k], bs2=0 * w0)
            continue
        w = p[k]
        if opt == 'GradientDescentOptimizer':
            out[name] = dict(w=w, bw=sgd_bounds(w, gg, dg, lr), moved=moved)
        elif opt == 'MomentumOptimizer':
            a = st['acc'][k]
            bw, ba = momentum_bounds(w, a, s1[k], gg, dg, lr, c['mom'])
            out[name] = dict(w=w, bw=bw, s1=a, bs1=ba, moved=moved)
        else:
            m, v = st['m'][k], st['v'][k]
            bw, bm, bv = adam_bounds(w, m, v, s1[k], v0[k], gg, dg, lr_t, c)
            out[name] = dict(w=w, bw=bw, s1=m, bs1=bm, s2=v, bs2=bv, moved=moved)


# ---- the check ----------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def check_close(name, got, ref, bound):
    """Every element within its bound (and finite); records the worst ratio."""
    got64 = np.asarray(got, dtype=np.float64).reshape(np.shape(ref))
    err = np.abs(got64 - ref)
    bad = ~(err <= bound)                                  # NaN fails too
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    WORST[name] = max(WORST.get(name, 0.0), float(np.nanmax(ratio)) if ratio.size else 0.0)
    if np.any(bad):
        i = np.unravel_index(int(np.argmax(np.where(bad, np.nan_to_num(ratio, nan=np.inf), -1))), np.shape(ref))
        raise AssertionError('%s: %d of %d elements outside the bound; worst at %s: got %r ref %r bound %.3g' % (
            name, int(bad.sum()), bad.size, i, float(got64[i]), float(ref[i]), float(bound[i])))


def check_exact(name, got, want):
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        diff = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        raise AssertionError('%s: %d elements changed that must be bit-identical (first at %d: %r -> %r)' % (
            name, diff.size, int(diff[0]), float(np.asarray(want).reshape(-1)[diff[0]]), float(np.asarray(got).reshape(-1)[diff[0]])))


def check_update(label, pre, post, rep, loss=None):
    """post (the device's state after the update, same structure as pre) against replay(): rows outside 'moved' bit-identical
    to pre in the parameter and every slot, the others within the bounds; the loss the apply wrote, when given."""
    for name, r in rep['vars'].items():
        slots = [('', post[name], pre[name], r['w'], r['bw'])]
        if 's1' in r:
            slots.append(('.s1', post['s1'][name], pre['s1'][name], r['s1'], r['bs1']))
        if 's2' in r:
            slots.append(('.s2', post['s2'][name], pre['s2'][name], r['s2'], r['bs2']))
        moved = r['moved']
        for suffix, got, before, ref, bnd in slots:
            tag = '%s %s%s' % (label, name, suffix)
            got = np.asarray(got, dtype=np.float32).reshape(ref.shape)
            before = np.asarray(before, dtype=np.float32).reshape(ref.shape)
            if moved is None:
                check_close(tag, got, ref, bnd)
                continue
            check_exact(tag + ' (not moved)', got[~moved], before[~moved])
            check_close(tag, got[moved], ref[moved], bnd[moved])
    if rep['loss'] is not None and loss is not None:
        ref, bnd = rep['loss']
        check_close(label + ' loss', np.array([loss]), np.array([ref]), np.array([bnd]))


def theta_pad_mask(tl):
    """Elements of theta that are channel pads of the outer conv weights [4][Pp][Pp] and biases [Pp] (P real channels)."""
    mask = np.zeros(int(tl.n), dtype=bool)
    P, Pp = int(tl.P), int(tl.Pp)
    for l in range(int(tl.live)):
        w = np.ones((4, Pp, Pp), dtype=bool)
        w[:, :P, :P] = False
        o = int(tl.conv_w[l])
        mask[o:o + w.size] = w.reshape(-1)
        o = int(tl.conv_b[l])
        mask[o + P:o + Pp] = True
    return mask
