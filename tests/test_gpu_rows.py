"""GPU: the kernels that move rows and build messages (gather.hip) and evaluate()'s metric sums (eval.hip) through the C ABI
against the numpy references of oracle/rows_check.py - bit for bit, except the float64 eval sums, which are held to the bound
derived there.

Every output pointer comes from a test-owned guarded buffer (Guard): 4 KiB of canary bytes in front of the payload and behind
it, the payload pre-filled with a NaN poison pattern.  After the call every canary byte is unchanged, every element the
contract says is written equals the reference (and so is not poison), every element it says is not written is still poison.
The shapes are the smallest at which each kernel can still go wrong: ragged unroll tails, chunk counts that are no power of
two, records wider than one 64-lane pass, and for each grid-stride loop one case beyond the cap of its grid."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cffm_amd.spec import CFFMConfig, init_params  # noqa: E402
from oracle import rows_check as rc  # noqa: E402

pytestmark = pytest.mark.gpu

M_TAB = 4999


def stream():
    return int(torch.cuda.current_stream().cuda_stream)


def dev_of(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guard(object):
    """canary | poisoned payload of nbytes | canary on the device; ptr is the payload's address (16-byte aligned)."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.buf = torch.empty(rc.image_bytes(nbytes), dtype=torch.uint8, device='cuda')
        self.poison()

    def poison(self):
        self.buf.fill_(rc.CANARY_BYTE)
        self.buf[rc.CANARY_BYTES:self.buf.numel() - rc.CANARY_BYTES].view(torch.int32).fill_(rc.POISON)

    @property
    def ptr(self):
        return self.buf.data_ptr() + rc.CANARY_BYTES

    def view(self, dtype=torch.float32):
        """The payload as a device tensor (to place inputs inside it)."""
        return self.buf[rc.CANARY_BYTES:rc.CANARY_BYTES + self.nbytes].view(dtype)

    def read(self, name, dtype=np.float32):
        """Canaries checked; the payload on the host."""
        torch.cuda.synchronize()
        return rc.split_image(name, self.buf.cpu().numpy(), self.nbytes).view(dtype)


class Dev(object):
    """Shape + the tables of rc.make_tables on the device, without an engine (no dense parameters: F = 64 would cost 260 MB)."""

    def __init__(self, M, F, K, D, inner_conv=1, outer_conv=1):
        from cffm_amd import hip
        hip.load()
        self.hip = hip
        self.lib = hip.fast()
        self.cfg = CFFMConfig(M=M, F=F, K=K, D=D, inner_conv=inner_conv, outer_conv=outer_conv)
        self.shape = hip.make_shape(self.cfg)
        self.tables = tables(M, K, D)
        self.d = {k: dev_of(v) for k, v in self.tables.items()}
        self.tab = hip.Tables(self.d['inner'].data_ptr(), self.d['outer'].data_ptr(), self.d['fbias'].data_ptr())
        self._s, self._t = C.addressof(self.shape), C.addressof(self.tab)

    def ws_layout(self, B):
        return self.hip.ws_layout(self.shape, B)


@functools.lru_cache(maxsize=None)
def tables(M, K, D):
    return rc.make_tables(M, K, D)


@functools.lru_cache(maxsize=8)
def dev(M, F, K, D, inner_conv=1, outer_conv=1):
    return Dev(M, F, K, D, inner_conv, outer_conv)


def engine(cfg, seed=1):
    """HipEngine whose three tables are rc.make_tables."""
    from cffm_amd.engine import HipEngine
    p = init_params(cfg, seed=seed)
    t = tables(cfg.M, cfg.K, cfg.D)
    p['inner_embeddings'], p['outer_embeddings'], p['feature_bias'] = t['inner'], t['outer'], t['fbias'].reshape(-1, 1)
    return HipEngine(cfg, params=p)


# ---- cffm_gather ----------------------------------------------------------------------------------------------------------
GATHER = {   # name: F, K, D, B, bad ids, every subset of NULL outputs
    'f3-k4-d4-b1': (3, 4, 4, 1, False, True),                    # smallest case
    'f10-k12-d32-b257': (10, 12, 32, 257, False, True),          # 11 chunks per slot, ragged unroll tail
    'f7-k32-d8-b63': (7, 32, 8, 63, False, True),                # K > D
    'f64-k32-d32-b5': (64, 32, 32, 5, False, True),              # the maximum number of fields
    'f10-k12-d32-b257-bad-ids': (10, 12, 32, 257, True, False),  # -1, INT32_MIN, M, INT32_MAX clamp to rows 0 and M - 1
    # 8,389,632 chunks > 8192 * 1024: second trip of the grid-stride loop (outputs of 67 MB each)
    'f32-k64-d64-b8193': (32, 64, 64, 8193, False, False),
}


def run_gather(d, ids, B, want, name):
    F, K, D = d.cfg.F, d.cfg.K, d.cfg.D
    n = max(B, 1) * F
    guards = [Guard(n * K * 4), Guard(n * D * 4), Guard(n * 4)]
    ptrs = [g.ptr if w else 0 for g, w in zip(guards, want)]
    rcode = d.lib.cffm_gather(d._s, d._t, ids.data_ptr(), B, ptrs[0], ptrs[1], ptrs[2], stream())
    assert rcode == 0, '%s: cffm_gather returned %d' % (name, rcode)
    return [g.read('%s %s' % (name, lab)) for g, lab in zip(guards, ('Ei', 'Eo', 'fb'))]


@pytest.mark.parametrize('name', list(GATHER))
def test_gather(name):
    F, K, D, B, bad, subsets = GATHER[name]
    d = dev(M_TAB, F, K, D)
    ids = rc.id_mix(np.random.default_rng(B + F), M_TAB, B * F, bad=bad).reshape(B, F)
    flat = ids.reshape(-1)
    assert 0 in flat and M_TAB - 1 in flat
    if bad:
        assert all(v in flat for v in (-1, rc.INT32_MIN, M_TAB, rc.INT32_MAX))
    if B * F >= 64:
        assert np.unique(flat).size < flat.size and (np.diff(flat) < 0).any()      # duplicates, unsorted
    dids = dev_of(ids)
    wants = [(bool(m & 1), bool(m & 2), bool(m & 4)) for m in range(7, -1, -1)] if subsets else [(True, True, True)]
    for want in wants:
        label = '%s want=%s' % (name, ''.join('EOB'[i] if w else '-' for i, w in enumerate(want)))
        got = run_gather(d, dids, B, want, label)
        rc.check_gather(label, [g if w else None for g, w in zip(got, want)], d.tables, ids, M_TAB)
        for g, w, lab in zip(got, want, ('Ei', 'Eo', 'fb')):
            if not w:
                rc.check_untouched('%s %s (passed as NULL)' % (label, lab), g)


def test_gather_empty_batch_writes_nothing():
    d = dev(M_TAB, 10, 12, 32)
    ids = dev_of(np.zeros((1, 10), dtype=np.int32))
    for g, lab in zip(run_gather(d, ids, 0, (True, True, True), 'gather B=0'), ('Ei', 'Eo', 'fb')):
        rc.check_untouched('gather B=0 ' + lab, g)


# ---- cffm_gather_packed ---------------------------------------------------------------------------------------------------
PACKED = {   # name: K, D, n, bad rows
    'k4-d4-n1': (4, 4, 1, False),
    'k12-d32-n1000': (12, 32, 1000, False),
    'k32-d32-n4099': (32, 32, 4099, False),
    'k12-d32-n1000-bad-rows': (12, 32, 1000, True),
    # 33 chunks per record, 8,650,785 chunks > 8192 * 1024: second trip of the grid-stride loop (output of 138 MB)
    'k64-d64-n262145': (64, 64, 262145, False),
}


@pytest.mark.parametrize('name', list(PACKED))
def test_gather_packed(name):
    K, D, n, bad = PACKED[name]
    d = dev(M_TAB, 3, K, D)
    rows = rc.id_mix(np.random.default_rng(n + K), M_TAB, n, bad=bad)
    out = Guard(n * (K + D + 4) * 4)
    assert d.lib.cffm_packed_row_floats(d._s) == K + D + 4
    rcode = d.lib.cffm_gather_packed(d._s, d._t, dev_of(rows).data_ptr(), n, out.ptr, stream())
    assert rcode == 0, '%s: cffm_gather_packed returned %d' % (name, rcode)
    rc.check_packed(name, out.read(name), d.tables, rows, M_TAB)


def test_gather_packed_no_rows_writes_nothing():
    d = dev(M_TAB, 3, 12, 32)
    out = Guard(48 * 4)
    assert d.lib.cffm_gather_packed(d._s, d._t, dev_of(np.zeros(4, dtype=np.int32)).data_ptr(), 0, out.ptr, stream()) == 0
    rc.check_untouched('gather_packed n=0', out.read('gather_packed n=0'))


# ---- cffm_stage_packed ----------------------------------------------------------------------------------------------------
STAGE = {   # name: F, K, D, B, n_records (None: B * F with pos = NULL), bad pos, inner_conv, outer_conv
    'f3-k4-d4-b1-nopos': (3, 4, 4, 1, None, False, 1, 1),
    'f10-k12-d32-b37-nopos': (10, 12, 32, 37, None, False, 1, 1),
    'f6-k32-d32-b64-nopos': (6, 32, 32, 64, None, False, 1, 1),
    'f10-k32-d32-b100-dups': (10, 32, 32, 100, 40, False, 1, 1),
    'f10-k32-d32-b100-bad-pos': (10, 32, 32, 100, 40, True, 1, 1),          # one negative, one >= n_records: clamped
    'f10-k12-d32-b37-no-inner': (10, 12, 32, 37, 50, False, 0, 1),          # ws.Ei keeps its poison
    'f10-k12-d32-b37-no-outer': (10, 12, 32, 37, 50, False, 1, 0),          # ws.Eo keeps its poison
    # 32768 slots x 66 chunks = 2,162,688 > 8192 * 256: second trip of the grid-stride loop.  F = 4 keeps the workspace at 89 MB
    # (cffm_ws_layout on the CPU; the slab plan of F = 64, K = 256, D = 4, B = 512 - the same slot and chunk counts - asks for 5.3 GB)
    'f4-k256-d4-b8192-cap': (4, 256, 4, 8192, 1000, False, 1, 1),
}


@pytest.mark.parametrize('name', list(STAGE))
def test_stage_packed(name):
    F, K, D, B, n_rec, bad, ic, oc = STAGE[name]
    d = dev(M_TAB, F, K, D, ic, oc)
    rng = np.random.default_rng(B + F + K)
    n = B * F
    wl = d.ws_layout(B)
    assert wl.bytes < (1 << 30)
    if name.endswith('cap'):
        assert n * (K // 4 + D // 4 + 1) > 8192 * 256
    pos = None
    if n_rec is not None:
        pos = rng.integers(0, n_rec, size=n).astype(np.int32)
        pos[:2] = [n_rec - 1, 0]
        if bad:
            pos[7], pos[n - 3] = -5, n_rec + 2
    packed = rc.packed_ref(d.tables, rc.id_mix(rng, M_TAB, n_rec or n), M_TAB)
    ws = Guard(wl.bytes)
    dpacked, dpos = dev_of(packed), (dev_of(pos) if pos is not None else None)
    rcode = d.lib.cffm_stage_packed(d._s, dpacked.data_ptr(), dpos.data_ptr() if dpos is not None else 0, n_rec or n, B, ws.ptr,
                                    stream())
    assert rcode == 0, '%s: cffm_stage_packed returned %d' % (name, rcode)
    img = ws.read(name + ' workspace')

    def member(off, count):
        return img[off // 4:off // 4 + count]
    got = (member(wl.Ei, n * K) if ic else None, member(wl.Eo, n * D) if oc else None, member(wl.fb, n))
    rc.check_stage(name, got, packed, pos, n_rec or n, B, F, K, D)
    # the whole workspace: the three members and nothing else - a disabled branch's member, the alignment gaps, ws.scalars in
    # front of Ei and ws.inner_out behind fb keep their poison
    assert wl.scalars < wl.Ei < wl.Eo < wl.fb < wl.inner_out
    want = rc.poison(wl.bytes // 4)
    for g, off in zip(got, (wl.Ei, wl.Eo, wl.fb)):
        if g is not None:
            want[off // 4:off // 4 + g.size] = g
    rc.check_exact(name + ' workspace outside Ei / Eo / fb', img, want)
    if not ic:
        rc.check_untouched(name + ' ws.Ei (inner_conv = 0)', member(wl.Ei, n * K))
    if not oc:
        rc.check_untouched(name + ' ws.Eo (outer_conv = 0)', member(wl.Eo, n * D))


# ---- round trip of a row-sharded lookup at world size 1 ---------------------------------------------------------------------
@pytest.mark.parametrize('F,K,D,B,id_range', [(10, 32, 32, 256, 150), (32, 64, 64, 9, None)])
def test_round_trip_equals_gather(F, K, D, B, id_range):
    """shard_plan -> gather_packed(send_rows[:u]) -> stage_packed(pos) leaves in the workspace what cffm_gather(ids) returns."""
    cfg = CFFMConfig(M=M_TAB, F=F, K=K, D=D)
    eng = engine(cfg)
    rng = np.random.default_rng(B)
    ids = rng.integers(0, id_range or M_TAB, size=(B, F)).astype(np.int32) * ((M_TAB // id_range) if id_range else 1)
    ids[0, :3] = [0, M_TAB - 1, 5]
    dids = dev_of(ids)
    plan = eng.shard_plan(dids, 1, M_TAB)
    ref = rc.plan_ref(ids, 1, M_TAB)
    u = int(ref[5][0])
    for lab, g, r in zip(('local_ids', 'order', 'uniq', 'pos', 'send_rows', 'counts'), plan, ref):
        g = g.cpu().numpy().reshape(-1)
        rc.check_exact('shard_plan ' + lab, g[:u] if lab == 'send_rows' else g, r)
    got = eng.gather_packed(plan[4][:u])
    eng.ws_tensor(B, 'Ei', (B, F, K)).view(torch.int32).fill_(rc.POISON)
    eng.ws_tensor(B, 'Eo', (B, F, D)).view(torch.int32).fill_(rc.POISON)
    eng.ws_tensor(B, 'fb', (B, F)).view(torch.int32).fill_(rc.POISON)
    eng.stage_packed(got, plan[3], B)
    Ei, Eo, fb = eng.gather(dids)
    for lab, a, b in (('Ei', eng.ws_tensor(B, 'Ei', (B, F, K)), Ei), ('Eo', eng.ws_tensor(B, 'Eo', (B, F, D)), Eo),
                      ('fb', eng.ws_tensor(B, 'fb', (B, F)), fb)):
        rc.check_exact('round trip ' + lab, a.cpu().numpy(), b.cpu().numpy())
    rc.check_gather('round trip', (Ei.cpu().numpy(), Eo.cpu().numpy(), fb.cpu().numpy()), tables(M_TAB, K, D), ids, M_TAB)


# ---- cffm_pack_rows_dedup -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(rc.DEDUP_CASES))
def test_pack_rows_dedup(name):
    c = rc.dedup_case(name)
    F, K, D, B = c['F'], c['K'], c['D'], c['B']
    n, W = B * F, K + D + 2
    cfg = CFFMConfig(M=c['M'], F=F, K=K, D=D, inner_conv=c['inner_conv'], outer_conv=c['outer_conv'])
    eng = engine(cfg)
    buf, wl = eng.workspace(B)
    # the row gradients go where the backward leaves them; a disabled branch's member holds poison, which must not reach the message
    for member, cols, on in (('dEi', K, c['inner_conv']), ('dEo', D, c['outer_conv']), ('dfb', 1, 1)):
        t = eng.ws_tensor(B, member, (n, cols))
        if on:
            t.copy_(dev_of(c[member].reshape(n, cols)))
        else:
            t.view(torch.int32).fill_(rc.POISON)
    if c['kind'] == 'hand':
        local_ids, order, uniq = dev_of(c['local_ids']), dev_of(c['order']), dev_of(c['uniq'])
    else:
        local_ids, order, uniq = eng.shard_plan(dev_of(c['ids']), 1, c['M'])[:3]
        for lab, g in (('local_ids', local_ids), ('order', order), ('uniq', uniq)):
            rc.check_exact('%s shard_plan %s' % (name, lab), g.cpu().numpy().reshape(-1), c[lab])
    runs = []
    for rep in range(2):
        out = Guard(n * W * 4)
        rcode = eng.lib.cffm_pack_rows_dedup(eng._s, local_ids.data_ptr(), order.data_ptr(), uniq.data_ptr(), B, buf.data_ptr(),
                                             out.ptr, stream())
        assert rcode == 0, '%s: cffm_pack_rows_dedup returned %d' % (name, rcode)
        runs.append(out.read('%s run %d' % (name, rep)))
    rc.check_dedup(name, runs[0], c['local_ids'], c['order'], c['uniq'], *rc.dedup_inputs(c), K, D)
    rc.check_exact(name + ' second run', runs[1], runs[0])


# ---- cffm_pack_rows (the rows output of cffm_backward_unscaled) -----------------------------------------------------------
PACK = {   # name: M, F, K, D, B, inner_conv, bad id
    'frappe-b7': (5382, 10, 32, 32, 7, 1, False),
    'f20-b5-wide': (3000, 20, 32, 32, 5, 1, False),
    'frappe-b7-no-inner': (5382, 10, 32, 32, 7, 0, False),
    'frappe-b7-bad-id': (5382, 10, 32, 32, 7, 1, True),
}


def row_grads_host(eng, B):
    dEi, dEo, dfb = eng.row_grads(B)
    n = B * eng.cfg.F
    return tuple(None if t is None else t.cpu().numpy().reshape(n, -1) for t in (dEi, dEo)) + (dfb.cpu().numpy().reshape(n),)


def step_inputs(M, F, B, seed, bad=False, id_range=None):
    rng = np.random.default_rng(seed)
    ids = (rng.integers(0, id_range or M, size=(B, F)) * ((M // id_range) if id_range else 1)).astype(np.int32)
    ids[0, :2] = [0, M - 1]
    if bad:
        ids[0, 3], ids[B - 1, F - 1] = M, -1
    y = rng.choice([-1.0, 1.0], size=B).astype(np.float32)
    return ids, y


@pytest.mark.parametrize('name', list(PACK))
def test_pack_rows(name):
    M, F, K, D, B, ic, bad = PACK[name]
    cfg = CFFMConfig(M=M, F=F, K=K, D=D, activation='selu', inner_conv=ic)
    eng = engine(cfg)
    ids, y = step_inputs(M, F, B, 3, bad)
    dids, dy = dev_of(ids), dev_of(y)
    n, W = B * F, K + D + 2
    buf, wl = eng.workspace(B)
    rows = Guard(n * W * 4)
    eng.forward(dids, dy)
    rcode = eng.lib.cffm_backward_unscaled(eng._s, eng.theta.data_ptr(), dids.data_ptr(), dy.data_ptr(), B, B, buf.data_ptr(),
                                           eng._grad_full.data_ptr(), rows.ptr, stream())
    assert rcode == 0, '%s: cffm_backward_unscaled returned %d' % (name, rcode)
    got = rows.read(name + ' rows')
    dEi, dEo, dfb = row_grads_host(eng, B)
    assert (dEi is None) == (not ic)
    assert np.isfinite(dEo).all() and np.any(dEo != 0) and np.any(dfb != 0), name + ': the backward left no row gradients'
    rc.check_pack_rows(name, got, ids, dEi, dEo, dfb, K, D)
    if bad:
        col0 = got.reshape(n, W)[:, 0].view(np.int32)
        assert col0[3] == M and col0[n - 1] == -1                   # the raw bits of a bad id stay
    nth = int(eng.tl.n)
    rc.check_exact(name + ' grad[theta.n] = ws.scalars[0]', eng._grad_full[nth:nth + 1].cpu().numpy(),
                   eng.ws_tensor(B, 'scalars', (16,))[0:1].cpu().numpy())


# ---- the block of cffm_dp_local: rows | sorted key run ---------------------------------------------------------------------
DP_LOCAL = {   # name: B, bad id, id range
    'frappe-b256-bad-id': (256, True, None),
    'frappe-b256-dups': (256, False, 40),
    'frappe-b1': (1, False, None),
}


@pytest.mark.parametrize('name', list(DP_LOCAL))
def test_dp_local_block(name):
    B, bad, id_range = DP_LOCAL[name]
    M, F, K, D = 5382, 10, 32, 32
    cfg = CFFMConfig(M=M, F=F, K=K, D=D, activation='selu')
    eng = engine(cfg)
    assert eng.lib.cffm_dp_runs_ok(eng._s, B) == 1
    ids, y = step_inputs(M, F, B, 5, bad, id_range)
    dids, dy = dev_of(ids), dev_of(y)
    n, W = B * F, K + D + 2
    buf, wl = eng.workspace(B)
    block = Guard(n * (W + 2) * 4)
    rcode = eng.lib.cffm_dp_local(eng._s, eng._t, eng.theta.data_ptr(), dids.data_ptr(), dy.data_ptr(), B, B, buf.data_ptr(),
                                  eng._grad_full.data_ptr(), block.ptr, stream())
    assert rcode == 0, '%s: cffm_dp_local returned %d' % (name, rcode)
    got = block.read(name + ' block')
    rows, run = got[:n * W].reshape(n, W), got[n * W:].view(np.uint64)
    rc.check_exact(name + ' column 0 (id bits)', rows[:, 0].view(np.int32), ids.reshape(-1))
    rc.check_sorted_run(name + ' sorted run', run, ids, M)
    rc.check_pack_rows(name + ' rows', rows, ids, *row_grads_host(eng, B), K, D)


# ---- cffm_eval_sums -------------------------------------------------------------------------------------------------------
LO, HI = -0.9, 0.1           # not floats: the kernel clips to float32(lo), float32(hi)
START = (3.5, -2.25, 7.0)
EVAL_N = [1, 63, 255, 256, 257, 65535, 65536, 65537, 200001]


@functools.lru_cache(maxsize=None)
def eval_case(n):
    rng = np.random.default_rng(n)
    pred = (rng.standard_normal(n) * 0.8).astype(np.float32)
    special = [np.inf, -np.inf, np.float32(LO), np.float32(HI), 5.0, -5.0]
    where = rng.choice(n, size=min(n, len(special)), replace=False)
    pred[where] = special[:where.size]
    y = rng.choice([-1.0, 1.0, 0.25], size=n).astype(np.float32)
    return pred, y


class EvalBuffers(object):
    def __init__(self, lib):
        self.lib = lib
        nb = int(lib.cffm_eval_scratch_bytes())
        assert nb == 256 * 3 * 8
        self.scratch, self.sums = Guard(nb), Guard(24)
        self.sums.view(torch.float64).copy_(dev_of(np.array(START)))

    def add(self, name, pred, y):
        """One call on scratch that holds NaN on entry; afterwards every partial is a number and a workgroup without elements left 0."""
        self.scratch.poison()
        n = int(pred.numel())
        rcode = self.lib.cffm_eval_sums(pred.data_ptr(), y.data_ptr(), n, LO, HI, self.scratch.ptr, self.sums.ptr, stream())
        assert rcode == 0, '%s: cffm_eval_sums returned %d' % (name, rcode)
        part = self.scratch.read(name + ' scratch', np.float64).reshape(256, 3)
        if n > 0:
            assert not np.isnan(part[:, 1:]).any(), name + ': a partial was left at the NaN the scratch held'
            idle = part[min(256, -(-n // 256)):]
            assert (rc.bits(idle) == 0).all(), name + ': a workgroup without elements did not leave a +0.0 partial'
        return part

    def result(self, name):
        return self.sums.read(name + ' sums', np.float64).copy()


def eval_lib():
    return dev(M_TAB, 3, 4, 4).lib


@pytest.mark.parametrize('n', EVAL_N)
def test_eval_sums(n):
    pred, y = eval_case(n)
    eb = EvalBuffers(eval_lib())
    eb.add('eval n=%d' % n, dev_of(pred), dev_of(y))
    ratio = rc.check_eval('eval n=%d' % n, eb.result('eval n=%d' % n), pred, y, LO, HI, START)
    print('eval n=%d |err|/bound: %s' % (n, ratio))


def test_eval_sums_split_in_three_calls():
    n = 200001
    pred, y = eval_case(n)
    cuts = [0, 65537, 165537, n]
    runs = []
    for rep in range(2):
        eb = EvalBuffers(eval_lib())
        for a, b in zip(cuts[:-1], cuts[1:]):
            eb.add('eval split [%d, %d)' % (a, b), dev_of(pred[a:b]), dev_of(y[a:b]))
        runs.append(eb.result('eval split'))
    rc.check_eval('eval split', runs[0], pred, y, LO, HI, START, n_calls=3)
    rc.check_exact('eval split, second run', runs[1], runs[0])


def test_eval_sums_empty_split_leaves_sums():
    eb = EvalBuffers(eval_lib())
    z = torch.zeros(4, dtype=torch.float32, device='cuda')
    part = eb.add('eval n=0', z[:0], z[:0])
    rc.check_untouched('eval n=0 scratch', part.view(np.float32))
    rc.check_exact('eval n=0 sums', eb.result('eval n=0'), np.array(START))


@pytest.mark.parametrize('where', ['first', 'last', 'beyond-65536'])
def test_eval_sums_nan_prediction(where):
    n = 70000
    pred, y = eval_case(n)
    pred = pred.copy()
    pred[{'first': 0, 'last': n - 1, 'beyond-65536': 65536 + 123}[where]] = np.nan
    eb = EvalBuffers(eval_lib())
    eb.add('eval nan ' + where, dev_of(pred), dev_of(y))
    got = eb.result('eval nan ' + where)
    assert np.isnan(got[0]) and np.isfinite(got[1:]).all(), got
    rc.check_eval('eval nan ' + where, got, pred, y, LO, HI, START)
