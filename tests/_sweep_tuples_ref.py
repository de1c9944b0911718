"""float64 reading of the tuple sweep's identity (the header comment of cffm_amd/csrc/sweep.hip) and of nothing else.

Swept fields f_0 < f_1 < ... < f_{nf-1} (sorted), E_i the context's outer rows, e_a the candidate's outer row at field f_a.  Every
layer-0 pair (i, j), i < j, is of exactly one class:

    neither swept     Zctx[y][x][q]    = sum over those pairs of sum_dh sum_dw E_i[2y+dh] E_j[2x+dw] W[dh][dw][(i,j)][q]
    one swept, f_a    U_a[dw][y][q]    = sum_dh sum_{i<f_a, i not swept} E_i[2y+dh] W[dh][dw][(i,f_a)][q]
                      V_a[dh][x][q]    = sum_dw sum_{j>f_a, j not swept} E_j[2x+dw] W[dh][dw][(f_a,j)][q]
    both, f_a < f_b   X_ab[y][x][q]    = sum_dh sum_dw e_a[2y+dh] e_b[2x+dw] W[dh][dw][(f_a,f_b)][q]       (per candidate)

    Z     = b + Zctx + sum_a (sum_dw e_a[2x+dw] U_a[dw][y] + sum_dh e_a[2y+dh] V_a[dh][x]) + sum_{a<b} X_ab
    s0[h] = s0fix[h] + sum_a (A_a[h] rowsum(e_a) + e_a[h] R_a) + sum_{a<b} e_a[h] rowsum(e_b)
    inner = (the pairs with no swept field, per context) + (every pair with at least one, per candidate)
    first-order term: the candidates' feature_bias at every swept slot

block_ref() is the per-context block, score_from_block() a score from a block plus the tuples' table rows.  Whatever does not depend
on the number of swept fields comes from oracle/sweep_check.py and oracle/cffm_oracle.py.  fault= names one planted mutant
(tests/test_sweep_tuples_ref.py shows that the GPU tests' criterion sees each)."""
import numpy as np

from oracle import cffm_oracle as orc
from oracle import sweep_check as sc

S16, D32 = sc.S16, sc.D32
FAULTS = ('no_cross_pair', 'slots_swapped', 'swept_row_in_U', 'A_with_swept')


def block_ref(cfg, p, ctx_row, fields, fault=None, Pp=None):
    """(block, S) of one context for the sorted swept fields: float64 values and, per element of every summed tensor, the sum of
    |terms|.  block: Z [16][16][P], U / V [nf][2][16][P], s0fix [32], A [nf][32], R [nf], fixed, and the exact fp32 copies Ei [F][K]
    and fb [16] with every swept row / slot zero."""
    F, M = cfg.F, cfg.M
    fields = [int(f) for f in fields]
    assert fields == sorted(set(fields)) and 0 <= fields[0] and fields[-1] < F and cfg.D == D32
    ids = sc.clamp_ids(ctx_row, M)
    ii, jj = orc.pair_index(F)
    keep = np.ones(F, bool)
    keep[fields] = False
    Eo_all = sc._f64(p['outer_embeddings'])[ids]                              # the swept rows: the context's own ids (mutants only)
    Eo = Eo_all * keep[:, None]
    W = sc._f64(p['outer_layer_conv_weight_0'])                               # [dh][dw][p][q]
    E2 = Eo.reshape(F, S16, 2)
    blk, S = {}, {}
    blk['Z'] = np.einsum('pyh,pxw,hwpq->yxq', E2[ii], E2[jj], W)
    S['Z'] = np.einsum('pyh,pxw,hwpq->yxq', np.abs(E2[ii]), np.abs(E2[jj]), np.abs(W))
    U, V, SU, SV, A, SA, R, SR = [], [], [], [], [], [], [], []
    for f in fields:
        Eu = Eo_all.reshape(F, S16, 2) if fault == 'swept_row_in_U' else E2
        below = [i for i in range(f) if keep[i] or fault == 'swept_row_in_U']
        above = [j for j in range(f + 1, F) if keep[j]]
        pu, pv = [sc.pair_of(i, f, F) for i in below], [sc.pair_of(f, j, F) for j in above]
        U.append(np.einsum('iyh,hwiq->wyq', Eu[below], W[:, :, pu, :]))
        SU.append(np.einsum('iyh,hwiq->wyq', np.abs(Eu[below]), np.abs(W[:, :, pu, :])))
        V.append(np.einsum('jxw,hwjq->hxq', E2[above], W[:, :, pv, :]))
        SV.append(np.einsum('jxw,hwjq->hxq', np.abs(E2[above]), np.abs(W[:, :, pv, :])))
        Ea = Eo_all if fault == 'A_with_swept' else Eo
        A.append(Ea[:f].sum(0))
        SA.append(np.abs(Ea[:f]).sum(0))
        R.append(Eo[f + 1:].sum())
        SR.append(np.abs(Eo[f + 1:]).sum())
    blk.update(U=np.stack(U), V=np.stack(V), A=np.stack(A), R=np.asarray(R))
    S.update(U=np.stack(SU), V=np.stack(SV), A=np.stack(SA), R=np.asarray(SR))
    rs, rsa = Eo.sum(1), np.abs(Eo).sum(1)
    Rge, Rgea = np.cumsum(rs[::-1])[::-1], np.cumsum(rsa[::-1])[::-1]
    blk['s0fix'] = (Eo[:-1] * Rge[1:, None]).sum(0)
    S['s0fix'] = (np.abs(Eo[:-1]) * Rgea[1:, None]).sum(0)
    Ei = np.asarray(p['inner_embeddings'], np.float32)[ids]
    Ei[fields] = 0
    blk['fixed'] = float(sc.inner_pairs64(cfg, p, Ei[None])[0, keep[ii] & keep[jj]].sum())
    blk['Ei'] = Ei
    fb = np.zeros(16, np.float32)
    fb[:F] = np.asarray(p['feature_bias'], np.float32).reshape(-1)[ids]
    fb[fields] = 0
    blk['fb'] = fb
    for k in ('Z', 'U', 'V'):
        blk[k], S[k] = sc._pad(blk[k], Pp), sc._pad(S[k], Pp)
    return blk, S


def chain_lengths(cfg, fields):
    """Terms (zeros included) of the sums the context kernel runs, per tensor; U_a: 2 f_a (the swept fields below f_a add exact zeros)."""
    F = cfg.F
    return {'Z': 2 * (F - 1) + 2 * F, 'V': 2 * (F - 1), 'U': [2 * f for f in fields], 's0fix': D32 + 2 * F, 'A': F, 'R': D32 + F}


def tuple_rows(cfg, p, cand, fields, order=None):
    """The table rows of the (clamped) tuples cand [N, nf], per SORTED field: order[a] = the column of cand that holds field
    fields[a]'s id (default: column a)."""
    cand = np.asarray(cand)
    order = list(range(len(fields))) if order is None else order
    return [sc.cand_rows(cfg, p, cand[:, order[a]]) for a in range(len(fields))]


def score_from_block(cfg, p, block, rows, fields, fault=None):
    """float64 scores [N] of the tuples whose table rows are rows[a] (tuple_rows, a over the sorted fields) from one context's block."""
    F, K, P, kind = cfg.F, cfg.K, cfg.P, cfg.activation
    fields = [int(f) for f in fields]
    nf = len(fields)
    if fault == 'slots_swapped':
        rows = [rows[1], rows[0]] + list(rows[2:])
    g = lambda k: np.asarray(block[k]).astype(np.float64)
    e = [sc._f64(r['outer']) for r in rows]                                   # [nf][N, D]
    N = e[0].shape[0]
    e2 = [v.reshape(N, S16, 2) for v in e]
    W = sc._f64(p['outer_layer_conv_weight_0'])
    Z, U, V = g('Z')[..., :P], g('U')[..., :P], g('V')[..., :P]
    z = sc._f64(p['outer_layer_conv_bias_0'])[None, None, None, :] + Z[None]
    for a in range(nf):
        z = z + np.einsum('nxw,wyq->nyxq', e2[a], U[a]) + np.einsum('nyh,hxq->nyxq', e2[a], V[a])
    if fault != 'no_cross_pair':
        for a in range(nf):
            for b in range(a + 1, nf):
                z = z + np.einsum('nyh,nxw,hwq->nyxq', e2[a], e2[b], W[:, :, sc.pair_of(fields[a], fields[b], F), :])
    A = orc.act(np.maximum(z, 0), kind)
    pools = [A.sum(axis=(2, 3))]
    for l in range(1, 4):
        Wl = sc._f64(p['outer_layer_conv_weight_%d' % l]).reshape(4 * P, P)
        A = orc.act(np.maximum(orc._im2col_2x2(A) @ Wl + sc._f64(p['outer_layer_conv_bias_%d' % l]), 0), kind)
        pools.append(A.sum(axis=(2, 3)))
    s0 = np.broadcast_to(g('s0fix')[None, :], (N, D32)).copy()
    for a in range(nf):
        s0 += g('A')[a][None, :] * e[a].sum(1)[:, None] + e[a] * float(g('R')[a])
        for b in range(a + 1, nf):
            s0 += e[a] * e[b].sum(1)[:, None]
    t1 = np.concatenate([s0] + pools, axis=1)
    h1 = t1 @ sc._f64(p['dense_1_kernel']) + sc._f64(p['dense_1_bias'])
    outer = float(cfg.beta_outer) * (h1 @ sc._f64(p['dense_2_kernel'])[:, 0] + float(sc._f64(p['dense_2_bias']).reshape(-1)[0]))
    Eall = np.broadcast_to(np.asarray(block['Ei'], np.float32)[None], (N, F, K)).copy()
    fb = np.broadcast_to(g('fb')[None, :F], (N, F)).copy()
    for a, f in enumerate(fields):
        Eall[:, f] = rows[a]['inner']
        fb[:, f] = sc._f64(rows[a]['fb'])
    ii, jj = orc.pair_index(F)
    live = np.isin(ii, fields) | np.isin(jj, fields)
    inner = float(g('fixed')) + sc.inner_pairs64(cfg, p, Eall)[:, live].sum(1) + float(sc._f64(p['dense_bias']).reshape(-1)[0])
    if cfg.linear_att:
        zl = (fb @ sc._f64(p['bias_W']) + sc._f64(p['bias_b'])) / float(cfg.lamda_att)
        a_ = np.exp(zl - zl.max(1, keepdims=True))
        a_ = a_ / a_.sum(1, keepdims=True)
        lin = (fb * a_) @ sc._f64(p['dense_3_kernel'])[:, 0] + float(sc._f64(p['dense_3_bias']).reshape(-1)[0])
    else:
        lin = fb.sum(1)
    raw = inner + outer + lin + float(sc._f64(p['bias']))
    if cfg.loss_type == 'log_loss':
        with np.errstate(over='ignore'):
            return 1.0 / (1.0 + np.exp(-raw))
    return raw


def split_columns(fields):
    """(sorted fields, order) of a caller's field list: order[a] = the caller's column of sorted field a."""
    fields = [int(f) for f in fields]
    order = sorted(range(len(fields)), key=lambda a: fields[a])
    return [fields[a] for a in order], order


def sweep_scores(cfg, p, ctx, fields, cand, fault=None):
    """[C][N] float64: block_ref + score_from_block for cand [N, nf] (one list) or [C, N, nf], `fields` in the caller's order."""
    ctx, cand = np.asarray(ctx), np.asarray(cand)
    srt, order = split_columns(fields)
    out = []
    for c in range(ctx.shape[0]):
        blk, _ = block_ref(cfg, p, ctx[c], srt, fault=fault)
        lst = cand if cand.ndim == 2 else cand[c]
        out.append(score_from_block(cfg, p, blk, tuple_rows(cfg, p, lst, srt, order), srt, fault=fault))
    return np.stack(out)


def oracle_scores(cfg, p, ctx, fields, cand, piece=100):
    """cffm_oracle.forward in float64 on the numpy-expanded, clamped id rows (tests/_cand_ref.expand_tuples) -> [C][N]."""
    from tests import _cand_ref as CR
    X = sc.clamp_ids(CR.expand_tuples(ctx, list(fields), cand), cfg.M)
    p64 = {k: np.asarray(v, np.float64) for k, v in p.items()}
    out = np.concatenate([orc.forward(p64, X[s:s + piece], cfg, keep_cache=False)[0] for s in range(0, X.shape[0], piece)])
    if cfg.loss_type == 'log_loss':
        with np.errstate(over='ignore'):
            out = 1.0 / (1.0 + np.exp(-out))
    return out.reshape(np.asarray(ctx).shape[0], -1)
