"""Exact check of the kernels that move rows and build messages (cffm_amd/csrc/gather.hip) and of evaluate()'s metric sums
(cffm_amd/csrc/eval.hip) against numpy.

TEST INFRASTRUCTURE, like everything under oracle/: only tests/ may import it; the product path (cffm_amd/) never does.

cffm_gather, cffm_gather_packed, cffm_stage_packed, cffm_pack_rows and the sorted key run behind the rows of cffm_dp_local are
pure data movement; cffm_pack_rows_dedup adds the duplicates of one id in a promised order (ascending slot), one fp32 addition
at a time, which numpy can repeat bit for bit.  So every comparison here is on the raw bits (a -0.0 or a NaN payload must
survive a copy) and there is no tolerance.  The faults such kernels have - a dropped last chunk, a column past lane 63, a
segment walked in another order, an unclamped index - change a few elements, which the whole-step comparisons at
1e-5 (|ref| + rms) with a 99 % tier can pass.

Guarded buffers.  A kernel's output lies inside a larger buffer: CANARY_BYTES of CANARY_BYTE in front of it and behind it, the
payload itself pre-filled with POISON (a quiet NaN with a payload no reference value has).  After the call every canary byte
must be unchanged (split_image), every element the contract says is written must equal the reference - and is therefore not
poison - (check_exact), and every element the contract says is not written must still be poison (check_untouched).

cffm_eval_sums is the one sum whose order numpy cannot repeat cheaply (256 workgroups, a butterfly per wavefront), so it gets
a bound instead, DERIVED here and not measured (eval_sums_ref):
  p      = pred if isnan(pred) else min(max(pred, lo), hi) in float32 (lo and hi arrive in the kernel as floats), then widened
  terms  (y - p)^2, y, y^2 in float64; the reference adds them with math.fsum (exact, rounded once)
  device rounds each term at most three times (the difference, the square, and the FMA contraction of s0 += d * d counted
         as a product and a sum) and adds the n terms in some fixed order: first order (n - 1 + 3) 2^-53 sum|term|; every
         accumulating call adds one rounding of `sums += s`, at most 2^-53 of the running sum, which the absolute sum (the value
         the call started from included) bounds.  The bound used is twice that first-order count:
             |got - ref| <= (n + n_calls + 4) 2^-52 (|start| + sum|term|)
  NaN    a NaN prediction makes sums[0] NaN (the kernel must not clip it to lo); sums[1] and sums[2] do not depend on the
         predictions and keep their bounds."""
import math

import numpy as np

f32 = np.float32
POISON = 0x7FD5A5A5                 # quiet NaN, payload 0x15A5A5; fits a positive int32 for a device-side fill
CANARY_BYTE = 0xC7
CANARY_BYTES = 4096
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
EPS64 = 2.0 ** -52


def bits(x):
    """The raw 32-bit (float32 / int32) or 64-bit (float64 / int64) patterns of an array."""
    x = np.ascontiguousarray(x)
    if x.dtype.itemsize == 4:
        return x.view(np.uint32)
    if x.dtype.itemsize == 8:
        return x.view(np.uint64)
    raise TypeError('bits(): %s' % x.dtype)


def poison(shape):
    """float32 array of the poison pattern."""
    return np.full(shape, POISON, dtype=np.uint32).view(f32)


# ---- guarded buffers ------------------------------------------------------------------------------------------------------
def image_bytes(nbytes):
    """Size of the guarded buffer around a payload of nbytes (kept a multiple of 16 so that the rear canary stays aligned)."""
    return CANARY_BYTES + (int(nbytes) + 15) // 16 * 16 + CANARY_BYTES


def make_image(nbytes):
    """Host image of a guarded buffer: canary | poisoned payload | canary (the GPU tests fill theirs on the device)."""
    img = np.full(image_bytes(nbytes), CANARY_BYTE, dtype=np.uint8)
    n4 = (int(nbytes) + 15) // 16 * 4
    img[CANARY_BYTES:CANARY_BYTES + 4 * n4].view(np.uint32)[:] = POISON
    return img


def split_image(name, image, nbytes):
    """Every canary byte unchanged -> the payload (uint8 view of nbytes bytes; the padding up to 16 bytes must stay poison)."""
    image = np.ascontiguousarray(image).view(np.uint8).reshape(-1)
    assert image.size == image_bytes(nbytes), '%s: image of %d bytes for a payload of %d' % (name, image.size, nbytes)
    end = image.size - CANARY_BYTES
    for what, part, base in (('front', image[:CANARY_BYTES], 0), ('rear', image[end:], end)):
        bad = np.flatnonzero(part != CANARY_BYTE)
        if bad.size:
            raise AssertionError('%s: canary changed: %d bytes of the %s canary, first at byte %d of the buffer (payload is '
                                 'bytes %d .. %d): 0x%02x' % (name, bad.size, what, base + bad[0], CANARY_BYTES, end, part[bad[0]]))
    assert int(nbytes) % 4 == 0, '%s: payloads are whole 32-bit words' % name
    pad = image[CANARY_BYTES + int(nbytes):end].view(np.uint32)
    if np.any(pad != POISON):
        raise AssertionError('%s: the %d bytes between the payload and the rear canary must stay poison' % (name, 4 * pad.size))
    return image[CANARY_BYTES:CANARY_BYTES + int(nbytes)]


# ---- comparison helpers ---------------------------------------------------------------------------------------------------
def check_exact(name, got, ref, describe=None):
    """Bit for bit.  An element still at poison is reported as 'left at poison', any other difference as 'wrong value';
    describe(flat index) -> text appended to the first of each kind."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype.itemsize == ref.dtype.itemsize, \
        '%s: got %s %s, reference %s %s' % (name, got.shape, got.dtype, ref.shape, ref.dtype)
    gb, rb = bits(got).reshape(-1), bits(ref).reshape(-1)
    bad = gb != rb
    if not bad.any():
        return
    pz = bad & (gb == POISON) if gb.dtype == np.uint32 else np.zeros_like(bad)
    wrong = bad & ~pz
    parts = []
    for kind, mask in (('left at poison', pz), ('wrong value', wrong)):
        n = int(mask.sum())
        if not n:
            continue
        i = int(np.flatnonzero(mask)[0])
        at = tuple(int(v) for v in np.unravel_index(i, got.shape))
        txt = '%d elements %s, first at %s' % (n, kind, at)
        if kind == 'wrong value':
            txt += ': got %r (0x%x) want %r (0x%x)' % (got.reshape(-1)[i], gb[i], ref.reshape(-1)[i], rb[i])
        if describe is not None:
            txt += ' ' + describe(i, at)
        parts.append(txt)
    raise AssertionError('%s: %d of %d elements differ; %s' % (name, int(bad.sum()), gb.size, '; '.join(parts)))


def check_untouched(name, got):
    """Every element must still hold the poison pattern."""
    gb = bits(got).reshape(-1)
    bad = np.flatnonzero(gb != POISON)
    if bad.size:
        at = tuple(int(v) for v in np.unravel_index(int(bad[0]), np.shape(got)))
        raise AssertionError('%s: must stay poison (nothing may be written here): %d of %d elements changed, first at %s: 0x%x' % (
            name, bad.size, gb.size, at, gb[bad[0]]))


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def make_tables(M, K, D):
    """Tables with a distinct value per (table, row, column), so that a row or column mix-up cannot cancel: inner = row +
    column / 1024 (< M), outer = -(row + 1) - column / 1024 (negative), feature_bias = M + row + 0.5; exact in fp32 for
    M <= 2^13 and K, D <= 1024.  A few -0.0 and one NaN element (payload 1), all in rows the id mixes look up (0, 5, M - 1)."""
    assert M >= 8 and M <= 8192
    r = np.arange(M, dtype=np.float64)[:, None]
    inner = (r + np.arange(K)[None, :] / 1024.0).astype(f32)
    outer = (-(r + 1.0) - np.arange(D)[None, :] / 1024.0).astype(f32)
    fbias = (M + r[:, 0] + 0.5).astype(f32)
    inner[0, 0] = f32(-0.0)
    outer[M - 1, D - 1] = f32(-0.0)
    outer[5, 1] = f32(-0.0)
    fbias[5] = f32(-0.0)
    inner.view(np.uint32)[M - 1, K - 1] = 0x7FC00001
    return {'inner': inner, 'outer': outer, 'fbias': fbias}


def id_mix(rng, M, n, bad=False):
    """Unsorted ids with 0, M - 1, 5 and duplicates; bad: also -1, INT32_MIN, M and INT32_MAX (where n allows)."""
    ids = rng.integers(0, M, size=n).astype(np.int64)
    fixed = [0, M - 1, 5, M - 1, 0] + ([-1, INT32_MIN, M, INT32_MAX] if bad else [])
    if n >= 2 * len(fixed):
        ids[rng.integers(0, n, size=n // 4)] = ids[:n // 4]               # duplicates
        where = rng.choice(n, size=len(fixed), replace=False)
        ids[where] = fixed
    else:
        ids[:min(n, len(fixed))] = fixed[::-1][:min(n, len(fixed))] if bad else fixed[:min(n, len(fixed))]
    return ids.astype(np.int32)


def grad_mix(rng, *shape):
    """Row gradients with exact zeros, tiny (< 1e-4) and large elements (the value mix of tests/test_gpu_update.py::grads)."""
    g = rng.standard_normal(shape) * 0.03
    u = rng.random(shape)
    g[u < 0.1] = 0.0
    g[(u >= 0.1) & (u < 0.2)] *= 1e-3
    g[(u >= 0.2) & (u < 0.25)] *= 300.0
    return g.astype(f32)


# ---- references -----------------------------------------------------------------------------------------------------------
def clamp_ids(ids, M):
    return np.clip(np.asarray(ids, dtype=np.int64), 0, M - 1)


def gather_ref(tables, ids, M):
    """tf.nn.embedding_lookup x3 with the library's clamp: ids [B,F] -> inner[id'] [B,F,K], outer[id'] [B,F,D], fbias[id'] [B,F]."""
    c = clamp_ids(ids, M)
    return tables['inner'][c], tables['outer'][c], tables['fbias'][c]


def packed_ref(tables, rows, M):
    """[n, K + D + 4] = (inner row | outer row | bias, +0.0, +0.0, +0.0) with the same clamp."""
    c = clamp_ids(rows, M).reshape(-1)
    K, D = tables['inner'].shape[1], tables['outer'].shape[1]
    out = np.zeros((c.size, K + D + 4), dtype=f32)
    out[:, :K] = tables['inner'][c]
    out[:, K:K + D] = tables['outer'][c]
    out[:, K + D] = tables['fbias'][c]
    return out


def stage_ref(packed, pos, n_records, B, F, K, D):
    """Slot i takes record clip(pos[i], 0, n_records - 1), or record i when pos is None -> Ei [B,F,K], Eo [B,F,D], fb [B,F]."""
    n = B * F
    r = np.arange(n, dtype=np.int64) if pos is None else np.asarray(pos, dtype=np.int64).reshape(-1)
    r = np.clip(r, 0, n_records - 1)
    rec = np.asarray(packed).reshape(-1, K + D + 4)[r]
    return (np.ascontiguousarray(rec[:, :K]).reshape(B, F, K), np.ascontiguousarray(rec[:, K:K + D]).reshape(B, F, D),
            np.ascontiguousarray(rec[:, K + D]).reshape(B, F))


def plan_ref(ids, world, M):
    """numpy twin of cffm_shard_plan: (local_ids, order, uniq, pos, send_rows, counts) of ids in [0, M), row r on rank
    r % world at local row r // world; sorted by (owner, local row), stable."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    owner, local = ids % world, ids // world
    lb = max(1, int(local.max()).bit_length())
    key = (owner << lb) | local
    order = np.argsort(key, kind='stable')
    sk = key[order]
    head = np.ones(ids.size, dtype=bool)
    head[1:] = sk[1:] != sk[:-1]
    uniq = np.cumsum(head) - 1
    pos = np.empty(ids.size, dtype=np.int64)
    pos[order] = uniq
    send_rows = local[order][head]
    counts = np.bincount(owner[order][head], minlength=world)
    i32 = np.int32
    return local.astype(i32), order.astype(i32), uniq.astype(i32), pos.astype(i32), send_rows.astype(i32), counts.astype(np.int64)


def _columns(n, K, D, dEi, dEo, dfb):
    """[n, K + D + 1] gradient columns; a disabled branch (None) gives +0.0 columns."""
    x = np.zeros((n, K + D + 1), dtype=f32)
    if dEi is not None:
        x[:, :K] = np.asarray(dEi, dtype=f32).reshape(n, K)
    if dEo is not None:
        x[:, K:K + D] = np.asarray(dEo, dtype=f32).reshape(n, D)
    x[:, K + D] = np.asarray(dfb, dtype=f32).reshape(n)
    return x


def dedup_ref(local_ids, order, uniq, dEi, dEo, dfb, K, D, descending=False):
    """cffm_pack_rows_dedup: [#distinct, 1 + K + D + 1].  For every distinct index u its sorted positions q are walked in
    ascending q and every column is summed sequentially in fp32, g = float32(0), g = float32(g + x[order[q]]); column 0 is the
    int32 bits of local_ids[order[q_head]].  Bit-exact: the kernel only adds.  descending: the same segments walked backwards
    (what the checker must tell apart)."""
    local_ids = np.asarray(local_ids, dtype=np.int32).reshape(-1)
    order, uniq = np.asarray(order, dtype=np.int64), np.asarray(uniq, dtype=np.int64)
    n = order.size
    x = _columns(n, K, D, dEi, dEo, dfb)
    nd = int(uniq[-1]) + 1
    out = np.zeros((nd, K + D + 2), dtype=f32)
    heads = np.flatnonzero(np.r_[True, uniq[1:] != uniq[:-1]])
    ends = np.r_[heads[1:], n]
    for h, e in zip(heads, ends):
        u = int(uniq[h])
        g = np.zeros(K + D + 1, dtype=f32)
        qs = range(e - 1, h - 1, -1) if descending else range(h, e)
        for q in qs:
            g = (g + x[order[q]]).astype(f32)
        out[u, 1:] = g
        out[u, 0:1].view(np.int32)[0] = local_ids[order[h]]
    return out


def pack_rows_ref(ids, dEi, dEo, dfb, K, D):
    """cffm_pack_rows: [B*F, 1 + K + D + 1] with the RAW id bits in column 0 (a bad id stays as it is)."""
    ids = np.asarray(ids, dtype=np.int32).reshape(-1)
    out = np.empty((ids.size, K + D + 2), dtype=f32)
    out[:, 0] = ids.view(f32)
    out[:, 1:] = _columns(ids.size, K, D, dEi, dEo, dfb)
    return out


def sorted_run_ref(ids, M):
    """The B*F 64-bit words cffm_dp_local leaves behind its rows: sorted (key_id << 32 | slot), key_id = M for an id outside [0, M)."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    key = np.where((ids < 0) | (ids >= M), M, ids).astype(np.uint64)
    return np.sort((key << np.uint64(32)) | np.arange(ids.size, dtype=np.uint64))


def clip_f32(pred, lo, hi):
    pred = np.asarray(pred, dtype=f32)
    with np.errstate(invalid='ignore'):
        p = np.minimum(np.maximum(pred, f32(lo)), f32(hi))
    return np.where(np.isnan(pred), pred, p).astype(f32)


def eval_sums_ref(pred, y, lo, hi, start=(0.0, 0.0, 0.0), n_calls=1):
    """(ref [3], bound [3]) of sums after accumulating (pred, y) onto `start` in n_calls calls (module docstring).  ref[0] is NaN
    when a prediction is NaN."""
    p = clip_f32(pred, lo, hi).astype(np.float64)
    yt = np.asarray(y, dtype=f32).astype(np.float64)
    d = yt - p
    terms = (d * d, yt, yt * yt)
    n = yt.size
    ref, bound = np.empty(3), np.empty(3)
    for k in range(3):
        t = terms[k]
        ref[k] = math.fsum([float(start[k])] + t.tolist()) if not np.isnan(t).any() else np.nan
        bound[k] = (n + n_calls + 4) * EPS64 * (abs(float(start[k])) + math.fsum(np.abs(t[~np.isnan(t)]).tolist()))
    return ref, bound


# ---- per-kernel checks ----------------------------------------------------------------------------------------------------
def _which_row(table, row_bits):
    """Rows of `table` [M, C] whose bits equal row_bits [C] (for the message of a mismatch)."""
    hit = np.flatnonzero((bits(table) == row_bits[None, :]).all(axis=1))
    return hit.tolist()


def check_gather(name, got, tables, ids, M):
    """got = (Ei, Eo, fb) as read back from the guarded outputs; an entry that is None was passed as NULL and is not compared."""
    ids = np.asarray(ids)
    ref = gather_ref(tables, ids, M)
    flat = ids.reshape(-1)
    for label, g, r, tab in zip(('Ei', 'Eo', 'fb'), got, ref, (tables['inner'], tables['outer'], tables['fbias'].reshape(-1, 1))):
        if g is None:
            continue
        C = tab.shape[1]
        g2 = np.ascontiguousarray(g).reshape(flat.size, C)

        def describe(i, at, g2=g2, tab=tab, C=C):
            slot = i // C
            return '(slot %d, id %d -> row %d; the slot holds row %s of the table)' % (
                slot, flat[slot], clamp_ids(flat[slot], M), _which_row(tab, bits(g2[slot])) or '<none>')
        check_exact('%s %s' % (name, label), g2, np.ascontiguousarray(r).reshape(flat.size, C), describe)


def check_packed(name, got, tables, rows, M):
    """got [n, K + D + 4].  The pad floats are looked at first: they must be exactly +0.0."""
    K, D = tables['inner'].shape[1], tables['outer'].shape[1]
    got = np.ascontiguousarray(got).reshape(-1, K + D + 4)
    pad = bits(got[:, K + D + 1:])
    bad = np.argwhere((pad != 0) & (pad != POISON))
    if bad.size:
        raise AssertionError('%s: pad float of a packed record is not +0.0: %d elements, first record %d pad %d: 0x%x' % (
            name, len(bad), bad[0][0], bad[0][1], pad[bad[0][0], bad[0][1]]))
    rows = np.asarray(rows).reshape(-1)
    full = np.concatenate([tables['inner'], tables['outer'], tables['fbias'].reshape(-1, 1)], axis=1)

    def describe(i, at):
        rec = at[0]
        return '(record %d, row %d -> %d; the record holds row %s of the tables)' % (
            rec, rows[rec], clamp_ids(rows[rec], M), _which_row(full, bits(got[rec, :K + D + 1])) or '<none>')
    check_exact(name, got, packed_ref(tables, rows, M), describe)


def check_stage(name, got, packed, pos, n_records, B, F, K, D):
    """got = (Ei, Eo, fb); an entry that is None (disabled branch) is not compared - the caller checks that it kept its poison."""
    ref = stage_ref(packed, pos, n_records, B, F, K, D)
    rec = np.asarray(packed).reshape(-1, K + D + 4)
    want = np.clip(np.arange(B * F) if pos is None else np.asarray(pos, dtype=np.int64).reshape(-1), 0, n_records - 1)
    for label, g, r, c0 in zip(('Ei', 'Eo', 'fb'), got, ref, (0, K, K + D)):
        if g is None:
            continue
        C = r.size // (B * F)
        g2 = np.ascontiguousarray(g).reshape(B * F, C)

        def describe(i, at, g2=g2, C=C, c0=c0):
            slot = i // C
            return '(slot %d; the slot holds record %s, want record %d)' % (
                slot, _which_row(rec[:, c0:c0 + C], bits(g2[slot])) or '<none>', want[slot])
        check_exact('%s %s' % (name, label), g2, np.ascontiguousarray(r).reshape(B * F, C), describe)


def check_dedup(name, got, local_ids, order, uniq, dEi, dEo, dfb, K, D):
    """got [B*F, 1 + K + D + 1] as read back: the first #distinct records equal dedup_ref, the others keep their poison."""
    W = K + D + 2
    got = np.ascontiguousarray(got).reshape(-1, W)
    ref = dedup_ref(local_ids, order, uniq, dEi, dEo, dfb, K, D)
    nd = ref.shape[0]
    check_untouched('%s records [%d, %d) beyond the distinct ids' % (name, nd, got.shape[0]), got[nd:])
    check_exact(name + ' column 0 (local row bits)', got[:nd, 0].view(np.int32), ref[:, 0].view(np.int32))
    if (bits(got[:nd]) != bits(ref)).any():
        other = dedup_ref(local_ids, order, uniq, dEi, dEo, dfb, K, D, descending=True)
        rows_bad = np.flatnonzero((bits(got[:nd]) != bits(ref)).any(axis=1))
        if all((bits(got[r]) == bits(other[r])).all() for r in rows_bad):
            raise AssertionError('%s: summation order: %d records equal the sum of their segment in DESCENDING slot order, not '
                                 'ascending (first record %d)' % (name, rows_bad.size, rows_bad[0]))
    check_exact(name, got[:nd], ref, lambda i, at: '(record %d, column %d of %d)' % (at[0], at[1], W))


def check_pack_rows(name, got, ids, dEi, dEo, dfb, K, D):
    W = K + D + 2
    ref = pack_rows_ref(ids, dEi, dEo, dfb, K, D)
    check_exact(name, np.ascontiguousarray(got).reshape(-1, W), ref, lambda i, at: '(slot %d, column %d of %d)' % (at[0], at[1], W))


def check_sorted_run(name, got, ids, M):
    check_exact(name, np.ascontiguousarray(got).view(np.uint64).reshape(-1), sorted_run_ref(ids, M),
                lambda i, at: '(sorted position %d)' % at[0])


def check_eval(name, got, pred, y, lo, hi, start=(0.0, 0.0, 0.0), n_calls=1):
    """got [3] float64 against eval_sums_ref.  Returns the |err| / bound ratios (nan for a NaN sum)."""
    got = np.asarray(got, dtype=np.float64).reshape(3)
    ref, bound = eval_sums_ref(pred, y, lo, hi, start, n_calls)
    ratio = np.full(3, np.nan)
    for k, what in enumerate(('sum (y - p)^2', 'sum y', 'sum y^2')):
        if np.isnan(ref[k]):
            if not np.isnan(got[k]):
                raise AssertionError('%s: sums[%d] (%s) must be NaN with a NaN prediction, got %r' % (name, k, what, got[k]))
            continue
        if not np.isfinite(got[k]):
            raise AssertionError('%s: sums[%d] (%s) is %r, reference %r' % (name, k, what, float(got[k]), float(ref[k])))
        err = abs(got[k] - ref[k])
        ratio[k] = err / bound[k] if bound[k] > 0 else (0.0 if err == 0 else np.inf)
        if err > bound[k]:
            raise AssertionError('%s: sums[%d] (%s) outside the bound: got %r ref %r |err| %.3g bound %.3g' % (
                name, k, what, float(got[k]), float(ref[k]), err, bound[k]))
    return ratio


# ---- the dedup cases (shared by tests/test_rows_check.py and tests/test_gpu_rows.py) ----------------------------------------
DEDUP_CASES = {   # name: F, K, D, B, inner_conv, outer_conv, ids
    'w10-21-slots': (3, 4, 4, 7, 1, 1, 'mix'),              # 21 slots, not a multiple of the 4 wavefronts of a workgroup
    'w46': (10, 12, 32, 64, 1, 1, 'mix'),
    'w66': (10, 32, 32, 64, 1, 1, 'mix'),                   # columns 64 and 65 sit in the second 64-lane pass
    'w130': (8, 64, 64, 32, 1, 1, 'mix'),                   # three passes
    'w66-one-id': (8, 32, 32, 256, 1, 1, 'one'),            # one segment of 2048 terms
    'w66-distinct': (10, 32, 32, 16, 1, 1, 'distinct'),
    'w66-no-inner': (10, 32, 32, 64, 0, 1, 'mix'),
    'w66-no-outer': (10, 32, 32, 64, 1, 0, 'mix'),
    'w66-hand-plan': (10, 32, 32, 16, 1, 1, 'hand'),        # hand-built order / uniq, local_ids the kernel must not validate
}
DEDUP_M = 3000


def dedup_case(name):
    """Inputs of one cffm_pack_rows_dedup case.  'mix' draws the ids from 40 values (heavy duplication) plus 0 and M - 1; the
    plan (world 1) is plan_ref's, which the GPU test holds cffm_shard_plan's output against before it uses that.  'hand' builds
    order / uniq by hand from keys that are NOT the local_ids, which hold a value >= 2^24 and the bits of a NaN."""
    F, K, D, B, ic, oc, kind = DEDUP_CASES[name]
    seed = sorted(DEDUP_CASES).index(name) + 100
    rng = np.random.default_rng(seed)
    n = B * F
    M = DEDUP_M
    if kind == 'one':
        ids = np.full(n, 7, dtype=np.int32)
    elif kind == 'distinct':
        ids = rng.permutation(M)[:n].astype(np.int32)
    else:
        ids = (rng.integers(0, 40, size=n) * 71).astype(np.int32)
        ids[rng.choice(n, size=2, replace=False)] = [0, M - 1]
    local_ids, order, uniq, pos, send_rows, counts = plan_ref(ids, 1, M)
    if kind == 'hand':
        local_ids = local_ids.copy()
        local_ids[order[0]] = (1 << 24) + 1               # not exact as a float
        local_ids[order[-1]] = 0x7FC00001                 # the bits of a NaN
    c = {'name': name, 'F': F, 'K': K, 'D': D, 'B': B, 'M': M, 'inner_conv': ic, 'outer_conv': oc, 'kind': kind, 'ids': ids.reshape(B, F),
         'local_ids': local_ids, 'order': order, 'uniq': uniq,
         'dEi': grad_mix(rng, n, K), 'dEo': grad_mix(rng, n, D), 'dfb': grad_mix(rng, n)}
    c['has_duplicates'] = int(uniq[-1]) + 1 < n
    return c


def dedup_inputs(c):
    """(dEi, dEo, dfb) as the kernel sees them: a disabled branch is None."""
    return (c['dEi'] if c['inner_conv'] else None, c['dEo'] if c['outer_conv'] else None, c['dfb'])
