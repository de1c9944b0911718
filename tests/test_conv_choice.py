"""cffm_conv_choice on the CPU: which kernel instance runs conv layer l of a shape at batch B (include/cffm_hip.h; conv_fwd_choice /
conv_bwd_choice in csrc/conv.hip, the value cffm_conv_fwd_impl / cffm_conv_bwd_impl switch on).

tests/golden/conv_choice.json was recorded from the commit BEFORE the choice functions existed, by tracing which instances its
dispatch ladders launched (the library's imports of the HIP runtime replaced by a recorder, the stage entry points driven over the
grid with dummy pointers), never from cffm_conv_choice itself: {"tuples": the distinct [fwd x5, wgrad x5, dgrad x5, paired] records,
each role (family, NT, RM, HALVES, b3), "cases": [F, D, B, act, index into tuples for layer 0 .. live-1]}.  The grid: 15 F x 6 D x
14 B, plus per layer the B that reaches each row-count threshold of the choice and the B just below it (tap-split row groups at 1024
and 2048 tiles of 16 rows, the direct kernels' 128 x 256 rows, 128 rows per slab at 64 and 256 slabs, the 64 -> 256 slab switch of
the plan), selu; relu and gelu on a sub-grid."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from cffm_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conv_choice.json')
BAD_SHAPE = 10001
ROLES = ('fwd', 'wgrad', 'dgrad')
FWD_TILE, FWD_TILE_PACKED, WGRAD_WGRAD2, WGRAD_WGRAD3, DGRAD_TILE_PACKED = 4, 5, 6, 7, 2     # include/cffm_hip.h


def _shape(F, D, act):
    return hip.Shape(M=5000, F=F, K=D, D=D, act=act, linear_att=1, inner_conv=1, outer_conv=1, loss=0, lamda_att=1.3,
                     beta_outer=1.0, lr=0.05, lamda=0.0, optimizer=0)


def _record(ch):
    return [getattr(getattr(ch, r), f) for r in ROLES for f in ('family', 'NT', 'RM', 'HALVES', 'b3')] + [ch.paired]


def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def choices(cases):
    """[[record of layer 0, .. live-1] per case] and the raw ConvChoice structs, from this process's library."""
    recs, raw = [], []
    for F, D, B, act, *_ in cases:
        sh = _shape(F, D, act)
        live = D.bit_length() - 2
        chs = [hip.conv_choice(sh, B, l) for l in range(live)]
        raw.append(chs)
        recs.append([_record(ch) for ch in chs])
    return recs, raw


@pytest.fixture(scope='module')
def golden():
    g = _golden()
    recs, raw = choices(g['cases'])
    return g, recs, raw


def _check_grid(g):
    cases = g['cases']
    assert {c[0] for c in cases} == {2, 3, 6, 7, 10, 11, 12, 16, 20, 23, 28, 32, 33, 34, 64}
    assert {c[1] for c in cases} == {4, 8, 16, 32, 64, 128}
    base = {1, 5, 33, 63, 64, 128, 255, 256, 257, 512, 1024, 2048, 4096, 8192}
    by_shape = {}
    for F, D, B, act, *idx in cases:
        assert len(idx) == D.bit_length() - 2 and all(0 <= i < len(g['tuples']) for i in idx)
        by_shape.setdefault((F, D, act), set()).add(B)
    for (F, D, act), bs in by_shape.items():
        if act != 3:
            continue
        assert base <= bs, (F, D)
        for l in range(D.bit_length() - 2):       # the B at each threshold and the one below it, where 1 <= B <= 16384
            S2 = (D >> (l + 1)) ** 2
            for rows in (16 * 1023 + 1, 16 * 2047 + 1, 128 * 256, 127 * 64 + 1, 127 * 256 + 1, 256 * 64):
                b = -(-rows // S2)
                assert {x for x in (b, b - 1) if 1 <= x <= 16384} <= bs, (F, D, l, rows)
    assert {c[3] for c in cases} == {0, 3, 4}     # relu, selu, gelu


def test_choice_equals_the_recorded_dispatch(golden):
    g, recs, _ = golden
    _check_grid(g)
    bad = [(c[:4], l, r, g['tuples'][i]) for c, rs in zip(g['cases'], recs) for l, (r, i) in enumerate(zip(rs, c[4:])) if r != g['tuples'][i]]
    assert not bad, '%d of %d differ, first: %s' % (len(bad), sum(len(r) for r in recs), bad[:3])
    # the activation does not enter the choice
    by = {}
    for c, rs in zip(g['cases'], recs):
        by.setdefault(tuple(c[:3]), {})[c[3]] = rs
    multi = [v for v in by.values() if len(v) > 1]
    assert len(multi) >= 50 and all(v[0] == v[3] == v[4] for v in multi)      # the sub-grid: 5 F x 2 D x 5 B


def test_fp32_latch_clears_b3_and_nothing_else(golden):
    g = golden[0]
    code = ('import json, sys; sys.path.insert(0, %r); from tests.test_conv_choice import choices, _golden; '
            'print("CHOICES " + json.dumps(choices(_golden()["cases"])[0]))' % ROOT)
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=dict(os.environ, CFFM_CONV_FP32='1'), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('CHOICES ')][-1][8:])

    def fp32(t):
        t = list(t)
        if t[5] == WGRAD_WGRAD3:
            t[5] = WGRAD_WGRAD2
        t[4] = t[9] = t[14] = 0
        return t
    want = [[fp32(g['tuples'][i]) for i in c[4:]] for c in g['cases']]
    assert any(t[4] or t[9] or t[14] for t in g['tuples'])          # the default latch has b3 choices to clear
    assert got == want


def test_layout_and_slab_plan_agree_with_the_choice(golden):
    g, _, raw = golden
    n_deferred = n_packed = 0
    for (F, D, B, act, *_), chs in zip(g['cases'], raw):
        sh = _shape(F, D, act)
        wl = hip.ws_layout(sh, B)
        Pp = (F * (F - 1) // 2 + 15) // 16 * 16
        live = len(chs)
        packed = chs[0].fwd.family == FWD_TILE_PACKED or chs[0].dgrad.family == DGRAD_TILE_PACKED
        assert (wl.w0pack_floats > 0) == packed, (F, D, B)
        n_packed += packed
        if any(ch.fwd.b3 or ch.dgrad.b3 for ch in chs):
            assert wl.wb3_bytes > 0, (F, D, B)
        tiles = (D // 2 // 16) * (Pp // 16)
        tiled = chs[0].fwd.family in (FWD_TILE, FWD_TILE_PACKED)
        assert (tiles > 0 and wl.pool_np[0] == tiles) == tiled, (F, D, B, wl.pool_np[0], tiles)
        # the fused top of the backward leaves its weight gradients to the launch of the layer below it: that launch is the pair kernel
        assert len({ch.top_wgrad_deferred for ch in chs}) == 1
        if chs[0].top_wgrad_deferred:
            first = max(live - 2, 1)
            assert first >= 2 and chs[first - 1].paired == 1, (F, D, B)
            n_deferred += 1
    assert n_deferred > 0 and n_packed > 0


def test_bad_arguments_are_refused():
    lib = hip.load()
    ch = hip.ConvChoice()
    ok = _shape(10, 32, 3)
    assert lib.cffm_conv_choice(C.byref(ok), 64, 0, C.byref(ch)) == 0
    assert lib.cffm_conv_choice(C.byref(ok), 64, 3, C.byref(ch)) == 0                 # live = 4
    assert lib.cffm_conv_choice(C.byref(ok), 0, 0, C.byref(ch)) == BAD_SHAPE
    assert lib.cffm_conv_choice(C.byref(ok), 64, -1, C.byref(ch)) == BAD_SHAPE
    assert lib.cffm_conv_choice(C.byref(ok), 64, 4, C.byref(ch)) == BAD_SHAPE
    assert lib.cffm_conv_choice(C.byref(_shape(1, 32, 3)), 64, 0, C.byref(ch)) == BAD_SHAPE
    assert lib.cffm_conv_choice(C.byref(_shape(10, 24, 3)), 64, 0, C.byref(ch)) == BAD_SHAPE
    assert lib.cffm_conv_choice(None, 64, 0, C.byref(ch)) == BAD_SHAPE
    assert lib.cffm_conv_choice(C.byref(ok), 64, 0, None) == BAD_SHAPE
