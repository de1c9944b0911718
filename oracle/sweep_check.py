"""Per-stage check of the shared candidate sweep (cffm_amd/csrc/sweep.hip): the per-context block against a float64 evaluation of
the rows and the filter it was built from, and the scores against a float64 evaluation of the block itself.

TEST INFRASTRUCTURE, like everything under oracle/: only tests/ may import it; the product path (cffm_amd/) never does.  float64 numpy;
nothing here is derived from the kernels' code: the split is the algebra written in the header comment of sweep.hip,

    Z[y][x][q] = b[q] + Zctx[y][x][q] + sum_dw e[2x+dw] U[dw][y][q] + sum_dh e[2y+dh] V[dh][x][q]
    s0[h]      = s0fix[h] + A[h] rowsum(e) + e[h] R
    inner      = (terms of the pairs without f) + (terms of the pairs with f)

f the swept field, e / the inner row / the feature_bias value of the candidate in its place.

block_ref()         the block of one context in float64 from the clamped ids and the tables, with S = sum |terms| per element of
                    every summed tensor; fault= names one mutant (tests/test_sweep_check.py shows that the bounds see each)
block_f32()         a float32 numpy stand-in of the block in the kernel's factorised order (T first, then Z): a numpy 'device'
check_block()       the bounds of tests/test_gpu_sweep_stages.py: exact copies, pads exactly 0, layer_check.check_tiers on Zctx / U / V,
                    branch_check.check on s0fix / A / R, branch_check.check_inner on the fixed inner sum
score_from_block()  float64 scores of candidates from a block (the device's own, widened, or block_ref's) and the candidates' rows:
                    layer 0 from the split, layers 1..3, the pools, dense(32) / dense(1), the first-order term, add_n, the sigmoid
                    of log_loss; fault= names one mutant
make_case()         the parameters and ids of the named cases, shared by the CPU and the GPU tests
conditions()        what keeps a case from hiding a failure: every relu switches, no dead channels, an unsaturated sigmoid

Chain lengths (n of the hard tier (n + 2) u S, zeros included, valid for any fp32 order): Zctx 2 (F - 1) + 2 F (step 1 then step 2 of
the factorised layer 0), V 2 (F - 1), U 2 f; s0fix D + 2 F, A F, R D + F with c = 1 (one product per term)."""
import numpy as np

from . import branch_check as bc
from . import cffm_oracle as orc
from . import layer_check as lc

S16, D32 = 16, 32
BLOCK_FAULTS = ('no_V', 'U_taps_swapped', 'pair_transposed', 'A_with_f', 'R_with_f', 'inner_with_f', 'pad_nonzero')
SCORE_FAULTS = ('no_relu0', 'pool1_row_short', 'pool2_row_short', 'pool3_row_short', 'pool4_row_short',
                'pool1_no_last_channel', 'pool2_no_last_channel', 'pool3_no_last_channel', 'pool4_no_last_channel',
                'no_beta', 'no_lamda', 'no_dense_bias', 'no_dense_1_bias', 'no_dense_2_bias', 'no_dense_3_bias', 'no_bias',
                'd2b_outside_beta', 'no_sigmoid')


def clamp_ids(ids, M):
    return np.clip(np.asarray(ids, np.int64), 0, M - 1)


def pair_of(i, j, F):
    """Index of pair (i, j), i < j, in the row-major order of orc.pair_index."""
    return i * (2 * F - i - 1) // 2 + j - i - 1


def _f64(x):
    return np.asarray(x, np.float32).astype(np.float64)


def _pad(a, Pp):
    if Pp is None or a.shape[-1] == Pp:
        return a
    out = np.zeros(a.shape[:-1] + (Pp,), a.dtype)
    out[..., :a.shape[-1]] = a
    return out


# ---- the block ----------------------------------------------------------------------------------------------------------------
def _fixed_inner(cfg, p, Ei, f, dtype=np.float64):
    """The inner-branch terms of the pairs without f (branch_check.inner_eval with the dense weights of the pairs with f zeroed and no
    dense bias) -> (value, S, the masked dense kernel)."""
    F, K = cfg.F, cfg.K
    ii, jj = orc.pair_index(F)
    dw = np.asarray(p['dense_kernel'], np.float32).reshape(cfg.P, K).copy()
    dw[(ii == f) | (jj == f)] = 0
    out, S = bc.inner_eval(Ei[None], p['inner_layer_conv_weight_0'].reshape(-1), p['inner_layer_conv_bias_0'], dw.reshape(-1),
                           np.zeros(1, np.float32), cfg.activation, dtype=dtype)
    return out['inner_out'][0], S['inner_out'][0], dw.reshape(-1)


def inner_pairs64(cfg, p, E):
    """The inner branch of the model (cffm_oracle.forward, CFFM.py:301-339) per pair in float64: E [N][F][K] -> [N][P], the sum of
    s * dense_kernel over the K columns of each pair (no dense bias)."""
    kind = cfg.activation
    ii, jj = orc.pair_index(cfg.F)
    E = _f64(E)
    x = orc.act(E[:, ii, :] * E[:, jj, :], kind)
    w, b2 = _f64(p['inner_layer_conv_weight_0']).reshape(2, 2), _f64(p['inner_layer_conv_bias_0'])
    x0, x1 = x[:, :, 0::2], x[:, :, 1::2]
    z = x0[..., None] * w[0] + x1[..., None] * w[1] + b2
    s = orc.act(np.maximum(z, 0), kind) + np.maximum(x0, x1)[..., None]
    return (s.reshape(E.shape[0], cfg.P, cfg.K) * _f64(p['dense_kernel']).reshape(cfg.P, cfg.K)[None]).sum(-1)


def block_ref(cfg, p, ctx_row, f, fault=None, Pp=None):
    """(block, S) of one context: float64 values from the clamped ids and the tables, and the per-element sum of |terms| of each
    summed tensor ('fixed' is evaluated as the model defines it, inner_pairs64; its S and the reference the device is held to are
    branch_check.inner_eval's, see check_block).  block: Z [16][16][P], U [2][16][P] (dw, y, q), V [2][16][P] (dh, x, q), s0fix [32], A [32], R, fixed (the inner
    sum of the pairs without f), and the exact copies Ei [F][K] (row f zero) and fb [16] (slot f and slots >= F zero), both fp32.
    Pp: pad the channel axis with zeros to Pp."""
    F, K, P, M = cfg.F, cfg.K, cfg.P, cfg.M
    assert cfg.D == D32
    ids = clamp_ids(ctx_row, M)
    ii, jj = orc.pair_index(F)
    keep = np.arange(F) != f
    Eo_all = _f64(p['outer_embeddings'])[ids]                                 # [F, D], row f: the context's own id (mutants only)
    Eo = Eo_all * keep[:, None]
    W = _f64(p['outer_layer_conv_weight_0'])                                  # [dh][dw][p][q]
    Ey, Ex = Eo.reshape(F, S16, 2), Eo.reshape(F, S16, 2)                     # [i][y][dh], [j][x][dw]
    blk, S = {}, {}
    blk['Z'] = np.einsum('pyh,pxw,hwpq->yxq', Ey[ii], Ex[jj], W)
    S['Z'] = np.einsum('pyh,pxw,hwpq->yxq', np.abs(Ey[ii]), np.abs(Ex[jj]), np.abs(W))
    below, above = [i for i in range(F) if i < f], [j for j in range(F) if j > f]
    pu, pv = [pair_of(i, f, F) for i in below], [pair_of(f, j, F) for j in above]
    Wu = W.transpose(1, 0, 2, 3) if fault == 'U_taps_swapped' else W
    blk['U'] = np.einsum('iyh,hwiq->wyq', Ey[below], Wu[:, :, pu, :])
    S['U'] = np.einsum('iyh,hwiq->wyq', np.abs(Ey[below]), np.abs(Wu[:, :, pu, :]))
    blk['V'] = np.einsum('jxw,hwjq->hxq', Ex[above], W[:, :, pv, :])
    S['V'] = np.einsum('jxw,hwjq->hxq', np.abs(Ex[above]), np.abs(W[:, :, pv, :]))
    if fault == 'no_V':
        blk['V'] = np.zeros_like(blk['V'])
    if fault == 'pair_transposed':            # (i, f) taken as (f, i): the candidate as the row operand, E_i as the column operand
        blk['V'] = blk['V'] + np.einsum('jxw,hwjq->hxq', Ex[below], W[:, :, pu, :])
        blk['U'] = np.zeros_like(blk['U'])
    rs, rsa = Eo.sum(1), np.abs(Eo).sum(1)
    Rge = np.cumsum(rs[::-1])[::-1]                                           # sum_{j >= i} rs[j]
    Rgea = np.cumsum(rsa[::-1])[::-1]
    blk['s0fix'] = (Eo[:-1] * Rge[1:, None]).sum(0)
    S['s0fix'] = (np.abs(Eo[:-1]) * Rgea[1:, None]).sum(0)
    hi = f + 1 if fault == 'A_with_f' else f
    blk['A'], S['A'] = Eo_all[:hi].sum(0), np.abs(Eo_all[:hi]).sum(0)
    lo = f if fault == 'R_with_f' else f + 1
    blk['R'], S['R'] = Eo_all[lo:].sum(), np.abs(Eo_all[lo:]).sum()
    Ei = np.asarray(p['inner_embeddings'], np.float32)[ids]
    Ei[f] = 0                                                                 # +0, as the kernel writes it (x * 0 would keep a sign)
    without = (ii != f) & (jj != f)
    Ein = Ei
    if fault == 'inner_with_f':               # one pair with f, on the row of the context's own id
        without[pair_of(f, f + 1, F) if f + 1 < F else pair_of(f - 1, f, F)] = True
        Ein = np.asarray(p['inner_embeddings'], np.float32)[ids]
    blk['fixed'] = float(inner_pairs64(cfg, p, Ein[None])[0, without].sum())
    S['fixed'] = _fixed_inner(cfg, p, Ei, f)[1]
    blk['Ei'] = Ei
    fb = np.zeros(16, np.float32)
    fb[:F] = np.asarray(p['feature_bias'], np.float32).reshape(-1)[ids]
    fb[f] = 0
    blk['fb'] = fb
    for k in ('Z', 'U', 'V'):
        blk[k], S[k] = _pad(blk[k], Pp), _pad(S[k], Pp)
    if fault == 'pad_nonzero':
        assert Pp is not None and Pp > P
        blk['Z'][3, 5, Pp - 1] = 1e-3
    return blk, S


def block_f32(cfg, p, ctx_row, f, Pp=None):
    """float32 numpy stand-in of the block in the kernel's factorised order: T[dh][i][x][q] = sum_{dw, j > i} E_j[2x+dw] W[dh][dw][(i,j)][q]
    first, Zctx[y][x][q] = sum_{dh, i} E_i[2y+dh] T[dh][i][x][q] from it; every sum sequential in float32."""
    F, P, M = cfg.F, cfg.P, cfg.M
    f32 = np.float32
    ids = clamp_ids(ctx_row, M)
    Eo = np.asarray(p['outer_embeddings'], f32)[ids]
    Eo[f] = 0
    W = np.asarray(p['outer_layer_conv_weight_0'], f32)
    E2 = Eo.reshape(F, S16, 2)
    T = np.zeros((2, F, S16, P), f32)
    for dh in range(2):
        for i in range(F - 1):
            for dw in range(2):
                for j in range(i + 1, F):
                    T[dh, i] = T[dh, i] + E2[j, :, dw, None] * W[dh, dw, pair_of(i, j, F)][None, :]
    Z = np.zeros((S16, S16, P), f32)
    for dh in range(2):
        for i in range(F):
            Z = Z + E2[i, :, dh, None, None] * T[dh, i][None]
    U = np.zeros((2, S16, P), f32)
    for dw in range(2):
        for dh in range(2):
            for i in range(f):
                U[dw] = U[dw] + E2[i, :, dh, None] * W[dh, dw, pair_of(i, f, F)][None, :]
    blk = {'Z': Z, 'U': U, 'V': T[:, f].copy()}
    rs = np.zeros(F, f32)
    for w in range(D32):
        rs = rs + Eo[:, w]
    s, R = np.zeros(D32, f32), f32(0)
    for i in range(F - 2, -1, -1):
        R = f32(R + rs[i + 1])
        s = s + Eo[i] * R
    A = np.zeros(D32, f32)
    for i in range(f):
        A = A + Eo[i]
    R = f32(0)
    for j in range(f + 1, F):
        R = f32(R + rs[j])
    blk.update(s0fix=s, A=A, R=R)
    Ei = np.asarray(p['inner_embeddings'], f32)[ids]
    Ei[f] = 0
    blk['fixed'] = f32(_fixed_inner(cfg, p, Ei, f, dtype=f32)[0])
    blk['Ei'] = Ei
    fb = np.zeros(16, f32)
    fb[:F] = np.asarray(p['feature_bias'], f32).reshape(-1)[ids]
    fb[f] = 0
    blk['fb'] = fb
    for k in ('Z', 'U', 'V'):
        blk[k] = _pad(blk[k], Pp)
    return blk


def chain_lengths(cfg, f):
    F = cfg.F
    return {'Z': 2 * (F - 1) + 2 * F, 'V': 2 * (F - 1), 'U': 2 * f, 's0fix': D32 + 2 * F, 'A': F, 'R': D32 + F}


def check_block(name, dev, cfg, p, ctx_row, f, sink=None):
    """Every tensor of one context's block (dev: name -> fp32 array, Z / U / V with all Pp channels) against block_ref of the same
    ids.  Raises AssertionError listing every tensor that missed; returns {tensor: worst |err| / bound}."""
    import torch
    P = cfg.P
    ref, S = block_ref(cfg, p, ctx_row, f, Pp=np.asarray(dev['Z']).shape[-1])
    n = chain_lengths(cfg, f)
    fails, worst = [], {}
    for k in ('Ei', 'fb'):
        got, want = np.asarray(dev[k], np.float32).reshape(-1), ref[k].reshape(-1)
        if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
            fails.append('%s %s: %d elements are not the bits of the clamped rows' % (name, k, int((got.view(np.uint32) != want.view(np.uint32)).sum())))
    for k in ('Z', 'U', 'V'):
        got = np.asarray(dev[k], np.float32)
        pad = got[..., P:]
        if pad.size and not (pad == 0).all():
            fails.append('%s %s: %d non-zero pad-channel elements' % (name, k, int((pad != 0).sum())))
        try:
            lc.check_tiers('%s %s' % (name, k), torch.from_numpy(got[..., :P].copy()), torch.from_numpy(ref[k][..., :P].copy()),
                           torch.from_numpy(S[k][..., :P].copy()), n[k])
        except AssertionError as e:
            fails.append(str(e))
        bound = (n[k] + 2) * lc.U * S[k][..., :P]
        err = np.abs(got[..., :P].astype(np.float64) - ref[k][..., :P])
        worst[k] = float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf)).max()) if err.size else 0.0
    for k in ('s0fix', 'A', 'R'):
        try:
            worst[k] = bc.check('%s %s' % (name, k), np.asarray(dev[k], np.float32), ref[k], S[k], n[k], 1)['hard']
        except AssertionError as e:
            worst[k] = getattr(e, 'stats', {}).get('hard', float('inf'))
            fails.append(str(e))
    dwm = _fixed_inner(cfg, p, ref['Ei'], f)[2]
    try:
        st = bc.check_inner('%s fixed inner sum' % name, {'inner_out': np.asarray(dev['fixed'], np.float32).reshape(1)}, ref['Ei'][None],
                            p['inner_layer_conv_weight_0'].reshape(-1), p['inner_layer_conv_bias_0'], dwm, np.zeros(1, np.float32),
                            cfg.activation)
        worst['fixed'] = st['inner_out'].get('hard', 0.0)
    except AssertionError as e:
        worst['fixed'] = float('inf')
        fails.append(str(e))
    if sink is not None:
        for k, v in worst.items():
            sink[k] = max(v, sink.get(k, 0.0))
    assert not fails, '\n'.join(fails)
    return worst


# ---- the scratch -----------------------------------------------------------------------------------------------------------------
def cut_blocks(raw, bl, cfg, C):
    """The C blocks of a scratch image (raw: its floats; bl: the struct cffm_sweep_block_layout filled) -> (list of block dicts,
    written: a bool mask over raw of the floats the context kernel is specified to write)."""
    F, K = cfg.F, cfg.K
    raw = np.asarray(raw, np.float32).reshape(-1)
    H, n = int(bl.header_floats), int(bl.block_floats)
    assert raw.size == H + C * n, (raw.size, H, C, n)
    Pp = (int(bl.U) - int(bl.Z)) // (S16 * S16)
    assert Pp % 16 == 0 and Pp >= cfg.P and (int(bl.V) - int(bl.U)) == 2 * S16 * Pp
    written = np.zeros(raw.size, bool)
    out = []
    for c in range(C):
        b = raw[H + c * n:H + (c + 1) * n]
        w = written[H + c * n:H + (c + 1) * n]
        parts = {'Z': (bl.Z, (S16, S16, Pp)), 'U': (bl.U, (2, S16, Pp)), 'V': (bl.V, (2, S16, Pp)), 'Ei': (bl.Ei, (F, K)),
                 's0fix': (bl.s0fix, (D32,)), 'A': (bl.A, (D32,)), 'fb': (bl.fb, (16,)), 'fixed': (bl.scal, ()), 'R': (bl.scal + 1, ())}
        d = {}
        for k, (off, shp) in parts.items():
            cnt = int(np.prod(shp)) if shp else 1
            d[k] = b[int(off):int(off) + cnt].reshape(shp).copy()
            w[int(off):int(off) + cnt] = True
        out.append(d)
    return out, written


# ---- the scores from a block --------------------------------------------------------------------------------------------------------
def cand_rows(cfg, p, cand):
    """The table rows of the (clamped) candidate ids, fp32."""
    ids = clamp_ids(cand, cfg.M)
    return {'inner': np.asarray(p['inner_embeddings'], np.float32)[ids], 'outer': np.asarray(p['outer_embeddings'], np.float32)[ids],
            'fb': np.asarray(p['feature_bias'], np.float32).reshape(-1)[ids]}


def _pool(A, l, fault):
    """Sum pool of one layer's activated output A [N][S][S][P] per row y; the pool mutants of layer l."""
    if fault == 'pool%d_row_short' % l:
        t = A.sum(axis=(2, 3))
        t[:, 0] = A[:, 0, :-1, :].sum(axis=(1, 2))
        return t
    if fault == 'pool%d_no_last_channel' % l:
        return A[..., :-1].sum(axis=(2, 3))
    return A.sum(axis=(2, 3))


def score_from_block(cfg, p, block, rows, f, fault=None):
    """float64 scores [N] of the candidates whose table rows are ``rows`` (cand_rows) from one context's block, and a dict with
    t1 [N][62], relu (the relu output of each of the four layers, [N][S][S][P]) and raw (the scores before the sigmoid)."""
    F, K, P, kind = cfg.F, cfg.K, cfg.P, cfg.activation
    g = lambda k: np.asarray(block[k]).astype(np.float64)
    e = _f64(rows['outer'])                                                   # [N, D]
    N = e.shape[0]
    ex = e.reshape(N, S16, 2)
    Z, U, V = g('Z')[..., :P], g('U')[..., :P], g('V')[..., :P]
    z = _f64(p['outer_layer_conv_bias_0'])[None, None, None, :] + Z[None]
    z = z + np.einsum('nxw,wyq->nyxq', ex, U) + np.einsum('nyh,hxq->nyxq', ex, V)
    relus, pools = [], []
    r = z if fault == 'no_relu0' else np.maximum(z, 0)
    relus.append(r)
    A = orc.act(r, kind)
    pools.append(_pool(A, 1, fault))
    for l in range(1, 4):
        Wl = _f64(p['outer_layer_conv_weight_%d' % l]).reshape(4 * P, P)
        z = orc._im2col_2x2(A) @ Wl + _f64(p['outer_layer_conv_bias_%d' % l])
        r = np.maximum(z, 0)
        relus.append(r)
        A = orc.act(r, kind)
        pools.append(_pool(A, l + 1, fault))
    s0 = g('s0fix')[None, :] + g('A')[None, :] * e.sum(1)[:, None] + e * float(g('R'))
    t1 = np.concatenate([s0] + pools, axis=1)
    d1b = 0.0 if fault == 'no_dense_1_bias' else _f64(p['dense_1_bias'])
    h1 = t1 @ _f64(p['dense_1_kernel']) + d1b
    d2b = 0.0 if fault == 'no_dense_2_bias' else float(_f64(p['dense_2_bias']).reshape(-1)[0])
    o = h1 @ _f64(p['dense_2_kernel'])[:, 0]
    beta = 1.0 if fault == 'no_beta' else float(cfg.beta_outer)
    outer = beta * o + d2b if fault == 'd2b_outside_beta' else beta * (o + d2b)
    # inner branch: the fixed sum + the terms of the pairs with f
    Eall = np.broadcast_to(np.asarray(block['Ei'], np.float32)[None], (N, F, K)).copy()
    Eall[:, f] = rows['inner']
    ii, jj = orc.pair_index(F)
    bd = 0.0 if fault == 'no_dense_bias' else float(_f64(p['dense_bias']).reshape(-1)[0])
    inner = float(g('fixed')) + inner_pairs64(cfg, p, Eall)[:, (ii == f) | (jj == f)].sum(1) + bd
    # first-order term
    fb = np.broadcast_to(g('fb')[None, :F], (N, F)).copy()
    fb[:, f] = _f64(rows['fb'])
    if cfg.linear_att:
        zl = fb @ _f64(p['bias_W']) + _f64(p['bias_b'])
        if fault != 'no_lamda':
            zl = zl / float(cfg.lamda_att)
        zl = zl - zl.max(1, keepdims=True)
        a = np.exp(zl)
        a = a / a.sum(1, keepdims=True)
        lin = (fb * a) @ _f64(p['dense_3_kernel'])[:, 0]
        if fault != 'no_dense_3_bias':
            lin = lin + float(_f64(p['dense_3_bias']).reshape(-1)[0])
    else:
        lin = fb.sum(1)
    raw = inner + outer + lin
    if fault != 'no_bias':
        raw = raw + float(_f64(p['bias']))
    out = raw
    if cfg.loss_type == 'log_loss' and fault != 'no_sigmoid':
        with np.errstate(over='ignore'):
            out = 1.0 / (1.0 + np.exp(-raw))
    return out, {'t1': t1, 'relu': relus, 'raw': raw}


def oracle_scores(cfg, p, ctx, f, cand, piece=100):
    """cffm_oracle.forward in float64 on the expanded, clamped id rows (the sigmoid applied for log_loss) -> [C][N]."""
    ctx, cand = np.asarray(ctx), np.asarray(cand)
    C, N = ctx.shape[0], cand.size
    X = np.repeat(ctx, N, axis=0)
    X[:, f] = np.tile(cand, C)
    X = clamp_ids(X, cfg.M)
    p64 = {k: np.asarray(v, np.float64) for k, v in p.items()}
    out = np.concatenate([orc.forward(p64, X[s:s + piece], cfg, keep_cache=False)[0] for s in range(0, C * N, piece)])
    if cfg.loss_type == 'log_loss':
        with np.errstate(over='ignore'):
            out = 1.0 / (1.0 + np.exp(-out))
    return out.reshape(C, N)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# shape, seed, and for log_loss the factors on dense_kernel / dense_2_kernel that keep the raw scores off the flat ends of the sigmoid.
# A seed is changed where a shape misses a condition of conditions(); no condition is relaxed for a seed.
CASES = {
    'F2-K4-relu': dict(F=2, K=4, act='relu', M=60, seed=0),
    'F3-K8-relu': dict(F=3, K=8, act='relu', M=60, seed=0),
    'F4-K8-prelu-noatt': dict(F=4, K=8, act='prelu', M=60, linear_att=0, seed=0),
    'F5-K16-elu': dict(F=5, K=16, act='elu', M=90, seed=0),
    'F6-K8-selu': dict(F=6, K=8, act='selu', M=90, seed=0),
    'F9-K8-gelu': dict(F=9, K=8, act='gelu', M=90, seed=0),
    'F10-K32-selu': dict(F=10, K=32, act='selu', M=5382, seed=0),
    'F10-K64-relu': dict(F=10, K=64, act='relu', M=300, seed=0),
    'F3-K8-relu-log': dict(F=3, K=8, act='relu', M=60, loss='log_loss', seed=0),
    'F6-K8-selu-log': dict(F=6, K=8, act='selu', M=90, loss='log_loss', seed=0),
    'F10-K32-selu-log': dict(F=10, K=32, act='selu', M=5382, loss='log_loss', seed=0),
}
LOG_SCALE = {'F6-K8-selu-log': (1.0, 0.01), 'F10-K32-selu-log': (0.5, 0.0025)}      # (on dense_kernel, on dense_2_kernel)
CASE_C, CASE_N = 3, 70        # contexts and candidates of a case's score checks (N: one full chunk of 64 and a ragged one)


def fields_of(cfg):
    return sorted({0, cfg.F // 2, cfg.F - 1})


def make_params(cfg, seed, log_scale=None):
    """init_params, then the magnitudes at which every term and every relu has work to do (tests/test_gpu_layers.py make_layer_case,
    tests/test_gpu_branches.py make_branch_case): trained-like tables, signed conv biases, every bias non-zero and of both signs."""
    from cffm_amd.spec import init_params
    p = init_params(cfg, seed=seed, dtype=np.float32)
    rng = np.random.default_rng(seed + 7)
    f32 = np.float32
    p['feature_bias'] = (rng.standard_normal(p['feature_bias'].shape) * 0.3).astype(f32)
    p['outer_embeddings'] = (p['outer_embeddings'] * 20.0).astype(f32)
    p['inner_embeddings'] = (p['inner_embeddings'] * 4.0).astype(f32)
    for l in range(cfg.live_layers):
        k = 'outer_layer_conv_bias_%d' % l
        p[k] = (rng.standard_normal(p[k].shape) * 0.02).astype(f32)
    p['inner_layer_conv_bias_0'] = np.asarray([0.03, -0.02], f32)
    p['dense_bias'] = np.asarray([0.5], f32)
    p['dense_1_bias'] = (rng.standard_normal(p['dense_1_bias'].shape) * 0.5).astype(f32)
    p['dense_2_bias'] = np.asarray([-0.4], f32)
    p['dense_3_bias'] = np.asarray([0.3], f32)
    p['bias'] = f32(-0.2)
    p['bias_b'] = (rng.standard_normal(p['bias_b'].shape) * 0.1).astype(f32)
    if log_scale is not None:
        p['dense_kernel'] = (p['dense_kernel'] * f32(log_scale[0])).astype(f32)
        p['dense_2_kernel'] = (p['dense_2_kernel'] * f32(log_scale[1])).astype(f32)
    return p


def make_case(name, C=CASE_C, N=CASE_N):
    """(cfg, params, ctx [C][F], cand [N]) of a named case; beta_outer = 0.7, lamda_att = 1.3."""
    from cffm_amd.spec import CFFMConfig
    c = CASES[name]
    cfg = CFFMConfig(M=c['M'], F=c['F'], K=c['K'], D=32, activation=c['act'], linear_att=c.get('linear_att', 1),
                     loss_type=c.get('loss', 'square_loss'), beta_outer=0.7, lamda_att=1.3)
    p = make_params(cfg, c['seed'], LOG_SCALE.get(name))
    rng = np.random.default_rng(c['seed'] + 100)
    ctx = rng.integers(0, cfg.M, size=(C, cfg.F)).astype(np.int32)
    cand = rng.permutation(cfg.M)[:N].astype(np.int32) if N <= cfg.M else rng.integers(0, cfg.M, size=N).astype(np.int32)
    return cfg, p, ctx, cand


def probe_params(cfg, p, k):
    """Parameters under which a raw score is t1[k] of the same tables and conv stack: dense(32) passes t1[k] to unit 0, dense(1)
    takes unit 0, and every other summand of add_n is zero (the tables' rows of the inner branch meet a zero dense kernel)."""
    from dataclasses import replace
    q = dict(p)
    f32 = np.float32
    d1 = np.zeros_like(p['dense_1_kernel'])
    d1[k, 0] = 1
    d2 = np.zeros_like(p['dense_2_kernel'])
    d2[0, 0] = 1
    q.update(dense_1_kernel=d1, dense_2_kernel=d2, dense_kernel=np.zeros_like(p['dense_kernel']),
             dense_bias=np.zeros(1, f32), dense_1_bias=np.zeros(32, f32), dense_2_bias=np.zeros(1, f32), dense_3_bias=np.zeros(1, f32),
             feature_bias=np.zeros_like(p['feature_bias']), bias_b=np.zeros_like(p['bias_b']), bias=f32(0))
    return replace(cfg, beta_outer=1.0), q


PROBE_ROWS = (0, 31, 32, 47, 48, 55, 56, 59, 60, 61)      # the first and the last row of s0 and of the four pools in t1


# ---- the conditions -------------------------------------------------------------------------------------------------------------
def conditions(relus, raw=None, log_loss=False):
    """relus: per layer, the relu outputs of all the rows of a case [rows][S][S][P].  Returns the figures; asserts that at each of
    the four layers 15 - 85 % of the elements are positive, that at most a tenth of a layer's channels are constant in sign over the
    rows, and for log_loss that at least 80 % of the raw scores lie in (-4, 4)."""
    out = {}
    for l, r in enumerate(relus):
        pos = r > 0
        frac = float(pos.mean())
        flat = pos.reshape(-1, pos.shape[-1])
        const = int((flat.all(0) | (~flat).all(0)).sum())
        out['layer %d' % l] = (frac, const, pos.shape[-1])
        assert 0.15 <= frac <= 0.85, 'layer %d: %.1f %% of the elements are positive' % (l, 100 * frac)
        assert const <= pos.shape[-1] // 10, 'layer %d: %d of %d channels are constant in sign' % (l, const, pos.shape[-1])
    if log_loss:
        inside = float((np.abs(raw) < 4).mean())
        out['|raw| < 4'] = inside
        assert inside >= 0.8, 'log_loss: only %.1f %% of the raw scores lie in (-4, 4)' % (100 * inside)
    return out
