"""Loop-level numpy reading of the candidate addressing rule of cffm_expand_candidates_ex / cffm_score_sweep_lists, written from the
prose of include/cffm_hip.h and from nothing else: id a (a < nf) of candidate n of context c lies at
cand[c * cand_ctx_stride + n * nf + a]; stride 0 is one list for every context; row g of the flattened [C * N] range is context
g / N with candidate g % N, whose ids replace the context's at the columns fields[0..nf) together."""
import numpy as np


def expand_ex_ref(ctx, fields, cand_flat, stride, N, first, rows):
    """ids of global rows [first, first + rows): int32 [rows, F].  cand_flat is the flat int32 buffer the kernel is handed."""
    ctx = np.asarray(ctx, dtype=np.int32)
    cand_flat = np.asarray(cand_flat, dtype=np.int32).reshape(-1)
    nf = len(fields)
    out = np.empty((rows, ctx.shape[1]), dtype=np.int32)
    for i in range(rows):
        g = first + i
        c, n = g // N, g % N
        for f in range(ctx.shape[1]):
            out[i, f] = ctx[c, f]
        for a in range(nf):
            out[i, fields[a]] = cand_flat[c * stride + n * nf + a]
    return out


def flat_lists(cand, stride, gap_value):
    """cand [C, N, nf] -> the flat buffer with `stride` elements per context; what lies beyond N * nf of a block is gap_value."""
    cand = np.asarray(cand, dtype=np.int32)
    C, N, nf = cand.shape
    assert stride >= N * nf
    buf = np.full((C, stride), gap_value, dtype=np.int32)
    buf[:, :N * nf] = cand.reshape(C, N * nf)
    return buf.reshape(-1)


def expand_tuples(ctx, fields, cand):
    """All C * N id rows for cand [N, nf] (one list) or [C, N, nf] (a list per context): int32 [C * N, F]."""
    cand = np.asarray(cand, dtype=np.int32)
    C = np.asarray(ctx).shape[0]
    if cand.ndim == 2:
        return expand_ex_ref(ctx, fields, cand, 0, cand.shape[0], 0, C * cand.shape[0])
    return expand_ex_ref(ctx, fields, cand, cand.shape[1] * cand.shape[2], cand.shape[1], 0, C * cand.shape[1])
