"""What oracle/rows_check.py can catch, on the CPU.  For one case per reference the correct output is built by an independent
formulation - a plain Python loop over slots and columns, not the vectorised code of the reference - and passes the check;
then each fault of the kind the whole-step comparisons let through is planted into that output and the check must name it."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import rows_check as rc  # noqa: E402

f = np.float32
M, F, K, D, B = 50, 4, 8, 12, 3
N = B * F
IDS = np.array([[7, 0, 49, 7], [-1, 50, rc.INT32_MIN, rc.INT32_MAX], [5, 33, 5, 12]], dtype=np.int32)
TABLES = rc.make_tables(M, K, D)


def clamp(i):
    return 0 if i < 0 else (M - 1 if i >= M else int(i))


def loop_gather(row_of=clamp):
    Ei, Eo, fb = rc.poison((B, F, K)), rc.poison((B, F, D)), rc.poison((B, F))
    for b in range(B):
        for s in range(F):
            r = row_of(int(IDS[b, s]))
            for c in range(K):
                Ei[b, s, c] = TABLES['inner'][r, c]
            for c in range(D):
                Eo[b, s, c] = TABLES['outer'][r, c]
            fb[b, s] = TABLES['fbias'][r]
    return Ei, Eo, fb


def loop_packed(rows):
    out = rc.poison((len(rows), K + D + 4))
    for i, r in enumerate(rows):
        r = clamp(r)
        for c in range(K):
            out[i, c] = TABLES['inner'][r, c]
        for c in range(D):
            out[i, K + c] = TABLES['outer'][r, c]
        out[i, K + D] = TABLES['fbias'][r]
        for c in range(1, 4):
            out[i, K + D + c] = f(0.0)
    return out


def test_tables_hold_the_special_values():
    assert np.signbit(TABLES['inner'][0, 0]) and TABLES['inner'][0, 0] == 0
    assert np.isnan(TABLES['inner'][M - 1, K - 1]) and rc.bits(TABLES['inner'])[M - 1, K - 1] != rc.POISON
    flat = np.concatenate([TABLES['inner'].reshape(-1), TABLES['outer'].reshape(-1), TABLES['fbias']])
    assert np.unique(rc.bits(flat)).size == flat.size - 3        # distinct apart from the four -0.0 (one pattern)
    assert not (rc.bits(flat) == rc.POISON).any()


# ---- cffm_gather ----------------------------------------------------------------------------------------------------------
def test_gather_check_passes_on_the_loop_formulation():
    rc.check_gather('gather', loop_gather(), TABLES, IDS, M)
    Ei, Eo, fb = loop_gather()
    rc.check_gather('gather NULL Eo', (Ei, None, fb), TABLES, IDS, M)
    # -0.0 and the NaN payload survive: +0.0 / another NaN in their place is a difference
    assert rc.bits(Ei)[0, 1, 0] == 0x80000000 and rc.bits(Ei)[0, 2, K - 1] == 0x7FC00001
    Ei[0, 1, 0] = f(0.0)
    with pytest.raises(AssertionError, match='wrong value'):
        rc.check_gather('gather', (Ei, Eo, fb), TABLES, IDS, M)


def test_gather_last_chunk_missing():
    Ei, Eo, fb = loop_gather()
    Eo[2, 3, D - 4:] = rc.poison(4)
    with pytest.raises(AssertionError, match=r'Eo: 4 of .*4 elements left at poison, first at \(11, 8\)'):
        rc.check_gather('gather', (Ei, Eo, fb), TABLES, IDS, M)


def test_gather_chunk_written_to_the_next_slot():
    Ei, Eo, fb = loop_gather()
    Ei[1, 2, 4:8] = Ei[1, 1, 4:8]                # the chunk of slot 5 lands in slot 6
    Ei[1, 1, 4:8] = rc.poison(4)
    with pytest.raises(AssertionError, match=r'left at poison, first at \(5, 4\).*wrong value, first at \(6, 4\)'):
        rc.check_gather('gather', (Ei, Eo, fb), TABLES, IDS, M)


def test_gather_id_not_clamped():
    got = loop_gather(row_of=lambda i: i % M)    # -1 -> row 49 instead of 0, 50 -> row 0 instead of 49
    with pytest.raises(AssertionError, match=r'slot 4, id -1 -> row 0; the slot holds row \[49\]'):
        rc.check_gather('gather', got, TABLES, IDS, M)


# ---- cffm_gather_packed ---------------------------------------------------------------------------------------------------
ROWS = [3, 49, 0, -1, 50, 3, rc.INT32_MAX]


def test_packed_check_passes_and_names_faults():
    good = loop_packed(ROWS)
    rc.check_packed('packed', good, TABLES, ROWS, M)
    bad = good.copy()
    bad[2, K + D + 2] = f(1e-30)
    with pytest.raises(AssertionError, match=r'pad float of a packed record is not \+0.0: 1 elements, first record 2 pad 1'):
        rc.check_packed('packed', bad, TABLES, ROWS, M)
    bad = good.copy()
    bad[5, K + D + 1] = f(-0.0)                  # -0.0 is not +0.0
    with pytest.raises(AssertionError, match='pad float'):
        rc.check_packed('packed', bad, TABLES, ROWS, M)
    bad = good.copy()
    bad[6, K + D:] = rc.poison(4)                # the last 16-byte chunk of the last record
    with pytest.raises(AssertionError, match=r'4 elements left at poison, first at \(6, 20\)'):
        rc.check_packed('packed', bad, TABLES, ROWS, M)
    bad = loop_packed([r % M for r in ROWS])     # not clamped
    with pytest.raises(AssertionError, match=r'record 3, row -1 -> 0; the record holds row \[49\]'):
        rc.check_packed('packed', bad, TABLES, ROWS, M)


# ---- cffm_stage_packed ----------------------------------------------------------------------------------------------------
POS = [2, 0, 1, 1, 4, -3, 2, 9, 0, 3, 3, 1]      # one negative, one >= n_records (5)
NREC = 5


def loop_stage(packed, pos, nrec=NREC):
    Ei, Eo, fb = rc.poison((B, F, K)), rc.poison((B, F, D)), rc.poison((B, F))
    for i in range(N):
        r = i if pos is None else pos[i]
        r = 0 if r < 0 else min(r, nrec - 1)
        for c in range(K):
            Ei[i // F, i % F, c] = packed[r, c]
        for c in range(D):
            Eo[i // F, i % F, c] = packed[r, K + c]
        fb[i // F, i % F] = packed[r, K + D]
    return Ei, Eo, fb


def test_stage_check_passes_and_names_faults():
    packed = loop_packed([3, 49, 0, 7, 21])
    rc.check_stage('stage', loop_stage(packed, POS), packed, POS, NREC, B, F, K, D)
    Ei, Eo, fb = loop_stage(packed, POS)
    rc.check_stage('stage no inner', (None, Eo, fb), packed, POS, NREC, B, F, K, D)
    ignored = loop_stage(packed, None)           # pos ignored: slot i takes record min(i, n_records - 1)
    with pytest.raises(AssertionError, match=r'slot 0; the slot holds record \[0\], want record 2'):
        rc.check_stage('stage', ignored, packed, POS, NREC, B, F, K, D)
    fb2 = fb.copy()
    fb2[2, 3] = rc.poison(1)[0]
    with pytest.raises(AssertionError, match=r'fb: 1 of 12 elements differ; 1 elements left at poison'):
        rc.check_stage('stage', (Ei, Eo, fb2), packed, POS, NREC, B, F, K, D)
    full = loop_packed(list(range(N)))
    rc.check_stage('stage pos None', loop_stage(full, None, N), full, None, N, B, F, K, D)


# ---- cffm_pack_rows_dedup -------------------------------------------------------------------------------------------------
def loop_dedup(c, descending=False, split_first_duplicate=False):
    """[B*F, W] by a loop over records, positions and columns; records beyond the distinct ids stay poison."""
    Kc, Dc = c['K'], c['D']
    W = Kc + Dc + 2
    n = c['B'] * c['F']
    dEi, dEo, dfb = rc.dedup_inputs(c)
    out = rc.poison((n, W))
    segs = {}
    for q in range(n):
        segs.setdefault(int(c['uniq'][q]), []).append(int(c['order'][q]))
    extra = len(segs)
    for u, slots in segs.items():
        if split_first_duplicate and len(slots) > 1:
            out[extra, 0:1].view(np.int32)[0] = c['local_ids'][slots[-1]]
            slots, last = slots[:-1], slots[-1]
        else:
            last = None
        out[u, 0:1].view(np.int32)[0] = c['local_ids'][slots[0]]
        for col in range(1, W):
            def x(sl):
                if col <= Kc:
                    return dEi[sl, col - 1] if dEi is not None else f(0.0)
                if col <= Kc + Dc:
                    return dEo[sl, col - 1 - Kc] if dEo is not None else f(0.0)
                return dfb[sl]
            g = f(0.0)
            for sl in (slots[::-1] if descending else slots):
                g = f(g + x(sl))
            out[u, col] = g
            if last is not None:
                out[extra, col] = f(f(0.0) + x(last))
        if last is not None:
            split_first_duplicate = False
    return out


@pytest.mark.parametrize('name', list(rc.DEDUP_CASES))
def test_dedup_inputs_are_order_sensitive(name):
    """A condition on the INPUTS of every dedup GPU case with duplicates: summing a segment in ascending and in descending slot
    order differs in at least one element (otherwise the GPU case could not tell the two orders apart)."""
    c = rc.dedup_case(name)
    assert c['has_duplicates'] == (c['kind'] != 'distinct')
    up = rc.dedup_ref(c['local_ids'], c['order'], c['uniq'], *rc.dedup_inputs(c), c['K'], c['D'])
    down = rc.dedup_ref(c['local_ids'], c['order'], c['uniq'], *rc.dedup_inputs(c), c['K'], c['D'], descending=True)
    assert up.shape == (int(c['uniq'][-1]) + 1, c['K'] + c['D'] + 2)
    if c['has_duplicates']:
        assert (rc.bits(up) != rc.bits(down)).any(), name + ': ascending and descending sums are identical'
    else:
        assert (rc.bits(up) == rc.bits(down)).all()
    if not c['inner_conv']:
        assert (rc.bits(up[:, 1:1 + c['K']]) == 0).all()             # exactly +0.0
    if not c['outer_conv']:
        assert (rc.bits(up[:, 1 + c['K']:1 + c['K'] + c['D']]) == 0).all()
    # slots ascend inside every segment (the stable order the header promises)
    o, u = c['order'].astype(np.int64), c['uniq']
    same = u[1:] == u[:-1]
    assert (o[1:][same] > o[:-1][same]).all()


def dedup_check(c, got):
    rc.check_dedup(c['name'], got, c['local_ids'], c['order'], c['uniq'], *rc.dedup_inputs(c), c['K'], c['D'])


def test_dedup_check_passes_and_names_faults():
    c = rc.dedup_case('w66')
    good = loop_dedup(c)
    dedup_check(c, good)
    bad = good.copy()
    bad[:3, 64] = rc.poison(3)                    # the second 64-lane pass never ran
    with pytest.raises(AssertionError, match=r'3 elements left at poison, first at \(0, 64\) \(record 0, column 64 of 66\)'):
        dedup_check(c, bad)
    with pytest.raises(AssertionError, match='summation order: .* DESCENDING slot order'):
        dedup_check(c, loop_dedup(c, descending=True))
    with pytest.raises(AssertionError, match=r'beyond the distinct ids: must stay poison'):
        dedup_check(c, loop_dedup(c, split_first_duplicate=True))
    bad = good.copy()
    bad[0, 0:1].view(np.int32)[0] += 1
    with pytest.raises(AssertionError, match='column 0'):
        dedup_check(c, bad)


@pytest.mark.parametrize('name', ['w10-21-slots', 'w66-no-inner', 'w66-no-outer', 'w66-hand-plan'])
def test_dedup_reference_equals_the_loop(name):
    c = rc.dedup_case(name)
    dedup_check(c, loop_dedup(c))
    if name == 'w66-hand-plan':
        got = loop_dedup(c)
        col0 = got[:int(c['uniq'][-1]) + 1, 0].view(np.int32)
        assert (1 << 24) + 1 in col0 and 0x7FC00001 in col0


def test_plan_ref_is_a_stable_sort_by_owner_then_local_row():
    ids = np.array([9, 4, 9, 2, 7, 4, 0, 9], dtype=np.int32)
    local, order, uniq, pos, send, counts = rc.plan_ref(ids, 2, 10)
    assert local.tolist() == [4, 2, 4, 1, 3, 2, 0, 4]
    assert order.tolist() == [6, 3, 1, 5, 4, 0, 2, 7]              # owner 0: rows 0, 2, 4, 4; owner 1: 7, 9, 9, 9
    assert uniq.tolist() == [0, 1, 2, 2, 3, 4, 4, 4]
    assert pos.tolist() == [4, 2, 4, 1, 3, 2, 0, 4]
    assert send.tolist() == [0, 1, 2, 3, 4] and counts.tolist() == [3, 2]


# ---- cffm_pack_rows and the sorted run of cffm_dp_local --------------------------------------------------------------------
def test_pack_rows_and_sorted_run():
    rng = np.random.default_rng(5)
    dEi, dEo, dfb = rc.grad_mix(rng, N, K), rc.grad_mix(rng, N, D), rc.grad_mix(rng, N)
    ids = IDS.reshape(-1)
    got = rc.poison((N, K + D + 2))
    for s in range(N):
        got[s, 0:1].view(np.int32)[0] = ids[s]
        for c in range(K):
            got[s, 1 + c] = dEi[s, c]
        for c in range(D):
            got[s, 1 + K + c] = dEo[s, c]
        got[s, 1 + K + D] = dfb[s]
    rc.check_pack_rows('rows', got, ids, dEi, dEo, dfb, K, D)
    noin = got.copy()
    noin[:, 1:1 + K] = f(0.0)
    rc.check_pack_rows('rows', noin, ids, None, dEo, dfb, K, D)
    bad = got.copy()
    bad[4, 0:1].view(np.int32)[0] = 0            # the bad id -1 clamped: column 0 must keep the RAW bits
    with pytest.raises(AssertionError, match=r'wrong value, first at \(4, 0\)'):
        rc.check_pack_rows('rows', bad, ids, dEi, dEo, dfb, K, D)
    keys = sorted(((M if (i < 0 or i >= M) else int(i)) << 32) | s for s, i in enumerate(ids.tolist()))
    rc.check_sorted_run('run', np.array(keys, dtype=np.uint64), ids, M)
    raw = sorted(((int(i) & 0xffffffff) << 32) | s for s, i in enumerate(ids.tolist()))       # bad ids keyed by their raw bits
    with pytest.raises(AssertionError, match='wrong value'):
        rc.check_sorted_run('run', np.array(raw, dtype=np.uint64), ids, M)


# ---- guarded buffers ------------------------------------------------------------------------------------------------------
def test_canaries():
    img = rc.make_image(40)
    assert img.size == 4096 + 48 + 4096
    pay = rc.split_image('buf', img, 40)
    rc.check_untouched('buf', pay.view(f))
    for byte in (0, 4095, 4096 + 48, img.size - 1):
        bad = img.copy()
        bad[byte] ^= 1
        with pytest.raises(AssertionError, match='canary changed: 1 bytes .* first at byte %d ' % byte):
            rc.split_image('buf', bad, 40)
    bad = img.copy()
    bad[4096 + 44] = 0                            # the padding between a 40-byte payload and the rear canary
    with pytest.raises(AssertionError, match='must stay poison'):
        rc.split_image('buf', bad, 40)
    pay2 = pay.copy().view(f)
    pay2[3] = f(1.0)
    with pytest.raises(AssertionError, match=r'must stay poison .* first at \(3,\)'):
        rc.check_untouched('buf', pay2)


# ---- cffm_eval_sums -------------------------------------------------------------------------------------------------------
LO, HI = -0.9, 0.1                                # 0.1 and -0.9 are not floats: the kernel clips to float32(lo), float32(hi)


def eval_case(n, seed=3):
    rng = np.random.default_rng(seed)
    pred = (rng.standard_normal(n) * 0.8).astype(f)
    pred[:6] = [np.inf, -np.inf, f(LO), f(HI), 5.0, -5.0]
    y = rng.choice([-1.0, 1.0, 0.25], size=n).astype(f)
    return pred, y


def device_like_sums(pred, y, lo, hi, start, stale=None, nan_to_lo=False, clip64=False):
    """The kernel's two stages with Python floats: element i belongs to workgroup (i // 256) % 256, every workgroup leaves one
    partial, the partials are added in workgroup order onto the running sums.  stale = (workgroup, values): that partial is
    not written and keeps what the scratch held."""
    part = [[0.0, 0.0, 0.0] for _ in range(256)]
    for i in range(len(pred)):
        raw = pred[i]
        if clip64:
            p = float(raw) if math.isnan(raw) else min(max(float(raw), lo), hi)
        elif math.isnan(raw) and not nan_to_lo:
            p = float(raw)
        else:
            p = f(lo) if math.isnan(raw) else min(max(raw, f(lo)), f(hi))
            p = float(p)
        yt = float(y[i])
        w = part[(i // 256) % 256]
        w[0] += (yt - p) * (yt - p)
        w[1] += yt
        w[2] += yt * yt
    if stale is not None:
        part[stale[0]] = list(stale[1])
    out = list(start)
    for k in range(3):
        s = 0.0
        for b in range(256):
            s += part[b][k]
        out[k] += s
    return np.array(out)


def test_eval_check_passes_and_names_faults():
    n = 1000
    pred, y = eval_case(n)
    start = (3.5, -2.25, 7.0)
    good = device_like_sums(pred, y, LO, HI, start)
    ratio = rc.check_eval('eval', good, pred, y, LO, HI, start)
    assert (ratio <= 1).all()
    # one partial taken from stale scratch: workgroup 200 has no element at n = 1000 and must still leave a 0
    with pytest.raises(AssertionError, match=r'sums\[0\] .* outside the bound'):
        rc.check_eval('eval', device_like_sums(pred, y, LO, HI, start, stale=(200, (1e-9, 0.0, 0.0))), pred, y, LO, HI, start)
    with pytest.raises(AssertionError, match=r'sums\[1\] \(sum y\) is nan'):
        rc.check_eval('eval', device_like_sums(pred, y, LO, HI, start, stale=(200, (0.0, np.nan, 0.0))), pred, y, LO, HI, start)
    # the clip in float64 against the unrounded bounds moves every clipped p
    assert float(f(HI)) != HI and rc.clip_f32([5.0], LO, HI).astype(np.float64)[0] != min(max(5.0, LO), HI)
    with pytest.raises(AssertionError, match=r'sums\[0\] .* outside the bound'):
        rc.check_eval('eval', device_like_sums(pred, y, LO, HI, start, clip64=True), pred, y, LO, HI, start)
    # NaN prediction
    pn = pred.copy()
    pn[n - 1] = np.nan
    good = device_like_sums(pn, y, LO, HI, start)
    assert np.isnan(good[0]) and np.isfinite(good[1:]).all()
    rc.check_eval('eval nan', good, pn, y, LO, HI, start)
    with pytest.raises(AssertionError, match=r'sums\[0\] .* must be NaN with a NaN prediction'):
        rc.check_eval('eval nan', device_like_sums(pn, y, LO, HI, start, nan_to_lo=True), pn, y, LO, HI, start)


def test_eval_bound_is_the_derived_one():
    pred, y = eval_case(64)
    ref, bound = rc.eval_sums_ref(pred, y, LO, HI, start=(1.0, 2.0, 3.0), n_calls=3)
    p = rc.clip_f32(pred, LO, HI).astype(np.float64)
    yt = y.astype(np.float64)
    A = [1.0 + float(np.sum((yt - p) ** 2)), 2.0 + float(np.sum(np.abs(yt))), 3.0 + float(np.sum(yt * yt))]
    np.testing.assert_allclose(bound, [(64 + 3 + 4) * 2.0 ** -52 * a for a in A], rtol=1e-12)
    assert p.max() == float(f(HI)) and p.min() == float(f(LO))        # +inf / -inf clip to the bounds
