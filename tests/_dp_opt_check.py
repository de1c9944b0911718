"""float64 replay of the multi-GPU SGD / Momentum apply (cffm_dp_apply_opt) WITH the late 1/L, for oracle/update_check.check_update.

oracle/update_check.replay(opt, ..., late=...) applies the late scale to the dense gradient of every optimizer, but hands the
table rows of SGD / Momentum / Adam to the oracle rule unscaled.  That is right when the scale is exactly 1 (the mse loss),
and replay_late() uses it as it stands there.  For the RMSE-style loss this module scales the inputs itself and widens the
bounds by what the device's own rounding of the scale adds.

Derivation of the widening (u = 2^-24, the error model of update_check's docstring).  The exact scale is
s = 1 / sqrt(sum / Bg + 1e-10f); the device holds s' = s (1 + d_s) with |d_s| <= LATE_U u, sums the n duplicates of a row in fp32,
G' = G + e with |e| <= gamma_{n-1} A (A = sum_k |g_k|), and rounds the product once more: g' = G' s' (1 + d), |d| <= u.  So

    |g' - s G| <= s |e| (1 + LATE_U u)(1 + u)  +  |s G| ((1 + LATE_U u)(1 + u) - 1)
               <= s gamma_{n-1} A (1 + LATE_U u) + (LATE_U + 1) u |g|          to first order, with g = s G.

replay(late=None) on the inputs multiplied by s IN FLOAT64 (no rounding: they are the exact g_k s) already charges the first
term: its own dg is gamma_{n-1} (s A) (1 + LATE_U u).  What it does not know of is the second term,

    extra = (LATE_U + 1) u |g|        (the dense gradient: n = 1, e = 0, the same extra),

the one extra rounding of s and of g s that the issue speaks of.  Both rules are linear in g, and update_check's bounds are linear
in dg, so extra goes through them as dg does: SGD's bound has lr dg (1 + 4u), so bw grows by lr extra (1 + 4u); Momentum's slot
bound has dg (1 + 4u), so bs1 grows by extra (1 + 4u) - unchanged but for the rounding factor - and its parameter bound has
lr |da| (1 + 4u), so bw grows by lr extra (1 + 4u)^2.  Rows nobody looked up have g = 0: nothing is added and they stay exact checks.
The loss the apply writes is sqrtf(x), x = sum / Bg + 1e-10f: within LOSS_U u of sqrt(x)."""
import numpy as np

from oracle import update_check as uc


def late_scale(lsum, Bg):
    """(x, s) of the RMSE-style loss in float64: x = sum / Bg + 1e-10f, s = 1 / sqrt(x)."""
    x = float(lsum) / int(Bg) + uc.LATE_EPS
    return x, 1.0 / np.sqrt(x)


def replay_late(opt, pre, grad, ids, rows, M, lr, lsum, Bg, rmse):
    """uc.replay for 'GradientDescentOptimizer' / 'MomentumOptimizer' with the late scale of the data-parallel apply.  Same
    arguments and result as uc.replay; (lsum, Bg, rmse) are its ``late``."""
    assert opt in ('GradientDescentOptimizer', 'MomentumOptimizer')
    if not rmse:
        return uc.replay(opt, pre, grad, ids, rows, M, lr, late=(lsum, Bg, False))          # scale exactly 1: correct as it stands
    x, s = late_scale(lsum, Bg)
    g64 = None if grad is None else np.asarray(grad, dtype=np.float64) * s
    rows64 = {k: (None if v is None else np.asarray(v, dtype=np.float64) * s) for k, v in rows.items()}
    rep = uc.replay(opt, pre, g64, ids, rows64, M, lr, late=None)
    lr32 = uc.f32(lr)
    r4 = 1 + 4 * uc.U
    exact = {'theta': g64}
    for name, _, rkey, _ in uc.TABLES:
        if rows64.get(rkey) is not None:
            exact[name] = uc.seg_sums(ids, rows64[rkey], M)[0]
    for name, g in exact.items():
        if g is None or name not in rep['vars']:
            continue
        r = rep['vars'][name]
        extra = (uc.LATE_U + 1) * uc.U * np.abs(g).reshape(np.shape(r['w']))
        if opt == 'GradientDescentOptimizer':
            r['bw'] = r['bw'] + lr32 * extra * r4
        else:
            r['bs1'] = r['bs1'] + extra * r4
            r['bw'] = r['bw'] + lr32 * extra * r4 * r4
    rep['loss'] = (np.sqrt(x), uc.LOSS_U * uc.U * np.sqrt(x))
    return rep
