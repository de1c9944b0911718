"""The arithmetic of the accepted shape domain, on the CPU ("Shape domain").

check_shape() (csrc/common.hpp) accepts F = 2 .. 64, D = a power of two in 4 .. 512 and K = any multiple of 4 from 4 up.  Three things
in the library are sized by those numbers and checked here without a GPU:

  fast_div   the float reciprocal division of the kernels' index arithmetic: a float32 numpy emulation over every divisor a call site
             can be given, with the reciprocal and its two float32 neighbours; the call sites are listed, so a new one is noticed
  LDS        the dynamic-LDS claims of the head forward and the inner-branch kernels: which accepted shapes pass 64 KB (the launch
             has to ask for them: set_lds) and which pass a CU's LDS (refused on the host with CFFM_ERR_UNSUPPORTED by cffm_ws_layout
             and the stage entry points, before anything is launched)
  ledger     which kernel instances of the recorded dispatch grid (tests/golden/conv_choice.json) the (F, D, B) of no GPU case reaches:
             compared with the committed list tests/golden/conv_unreached.json, one reason per entry; the test fails when the list is
             stale in either direction"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cffm_amd import hip  # noqa: E402

CSRC = os.path.join(ROOT, 'cffm_amd', 'csrc')
UNSUPPORTED = 10002
MAX_FIELDS, HEAD_UNITS = 64, 32
LDS_DEFAULT = 64 * 1024                      # what a launch gets without hipFuncSetAttribute
LDS_WHOLE_CU = 160 * 1024 - 512              # CFFM_LDS_WHOLE_CU
LDS_SHARED_CU = 150 * 1024                   # CFFM_LDS_SHARED_CU
F_ALL = range(2, MAX_FIELDS + 1)
D_ALL = [1 << i for i in range(2, 10)]


def _lib():
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return hip.load()


def _shape(F, K, D, **kw):
    base = dict(M=100, F=F, K=K, D=D, act=0, linear_att=1, inner_conv=1, outer_conv=1, loss=0, lamda_att=1.0, beta_outer=1.0, lr=0.05,
                lamda=0.0, optimizer=0)
    base.update(kw)
    return hip.Shape(**base)


def Pp_of(F):
    return (F * (F - 1) // 2 + 15) // 16 * 16


# the three formulas of csrc/common.hpp, in bytes
def head_fwd_lds(F, D):
    return (1024 + 8 * HEAD_UNITS + MAX_FIELDS + 4 + F * D + F * F) * 4 + 16


def inner_fwd_lds(F, K):
    return (F * K + Pp_of(F) + 16) * 4


def inner_bwd_lds(F, K):
    return (5 * F * K + Pp_of(F) + 8) * 4


def k_max(F):
    """The largest K of F fields whose inner-branch backward fits a CU."""
    K = ((LDS_WHOLE_CU // 4 - Pp_of(F) - 8) // (5 * F)) // 4 * 4
    assert inner_bwd_lds(F, K) <= LDS_WHOLE_CU < inner_bwd_lds(F, K + 4)
    return K


# ---- fast_div -----------------------------------------------------------------------------------------------------------------------
def fast_div(n, inv):
    """common.hpp fast_div in float32: (int)(((float)n + 0.5f) * inv_d)."""
    n = np.asarray(n)
    assert n.max() < 1 << 23                                      # (float)n + 0.5f is exact below 2^23
    return ((n.astype(np.float32) + np.float32(0.5)) * np.float32(inv)).astype(np.int64)


def reciprocals(d):
    """1.f / (float)d and its two float32 neighbours."""
    inv = np.float32(1.0) / np.float32(d)
    return inv, np.nextafter(inv, np.float32(0)), np.nextafter(inv, np.float32(np.inf))


def boundaries(d, n_end):
    """The n in [0, n_end) at which n // d steps (q d - 1 and q d), with 0 and n_end - 1.  fast_div is non-decreasing in n (the
    conversion, the addition and the product with a positive constant are monotone under round-to-nearest), so it equals n // d
    on [0, n_end) if and only if it does at these points."""
    q = np.arange(1, (n_end - 1) // d + 1, dtype=np.int64) * d
    n = np.concatenate([[0, n_end - 1], q - 1, q])
    return n[(n >= 0) & (n < n_end)]


N_DOC = 1 << 19          # the documented domain of fast_div: 0 <= n < 2^19, 1 <= d <= 4096
D_DOC = 4096

# (file, divisor as written at the call) of every fast_div call, plus the loops that spell the expression out ('(inline)').  Per divisor: the values it can take and a bound of n, both from the code at the site:
#   invD     D = 4 .. 512.  n < n_ex F D where the n_ex examples' rows [n_ex][F][D + 1] share one workgroup's LDS with more: < 40,832
#   invF     F = 2 .. 64.   n < n_ex F, the rows of the same tile
#   invPp    Pp = 16 .. 2016.  n is a column of the [4 taps][Pp] filter image, rounded up to a block of at most 8 tiles: < 4 Pp + 128
#   invK2    K / 2, n < P K / 2 (the units of one example) with F K within k_max(F): K2 <= 2040, n < 130,000
#   invK4    K / 4, n < F K / 4 (the 16-byte pieces of one example's rows): K4 <= 1020, n < 2048
#   a.inv_run_len   m = rows of one rank's sorted run, m = B F <= 4096 (cffm_fwd_all_ok); n < n_rows <= CFFM_LDS_SHARED_CU / 4 = 38,400
CALL_SITES = {
    'common.hpp': ['invD(inline)', 'invD(inline)'],              # the two branches of stage_example_rows
    'inner_body.hpp': ['invK2', 'invK4', 'invK2'],
    'conv.hip': ['invD', 'invPp', 'invPp', 'invPp', 'invPp', 'invD', 'invF', 'invPp', 'invPp', 'invPp', 'invD', 'invD', 'invD', 'invF',
                 'invD(inline)'],                                # conv0_fact_tile_fwd2_kernel stages its rows the same way
    'optim.hip': ['a.inv_run_len'],
}


def divisor_domain():
    """name -> (divisors, exclusive bound of n), as listed above; every one inside the documented domain."""
    kk = sorted({K for F in F_ALL for K in range(4, k_max(F) + 1, 4)})
    units = max(F * (F - 1) // 2 * (k_max(F) // 2) for F in F_ALL)
    dom = {
        'invD': (D_ALL, LDS_WHOLE_CU // 4),
        'invD(inline)': (D_ALL, MAX_FIELDS * 512),
        'invF': (list(F_ALL), LDS_WHOLE_CU // 4),
        'invPp': (sorted({Pp_of(F) for F in F_ALL}), 4 * Pp_of(MAX_FIELDS) + 128),
        'invK2': ([K // 2 for K in kk], units),
        'invK4': ([K // 4 for K in kk], MAX_FIELDS * max(kk) // 4),
        'a.inv_run_len': (list(range(2, 4097)), LDS_SHARED_CU // 4),
    }
    return dom


def test_fast_div_call_sites_are_the_listed_ones():
    """A plain count per file: a new call (or a new spelled-out '+ 0.5f) * inv') fails here until its divisor is listed."""
    found = {}
    for fn in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, fn)) as fh:
            src = fh.read()
        n = src.count('fast_div(') - src.count('int fast_div(')                  # calls, without the definition
        inline = src.count('+ 0.5f) * inv') - src.count('+ 0.5f) * inv_d')      # the expression spelled out
        if n or inline:
            found[fn] = (n, inline)
    want = {fn: (sum('inline' not in d for d in v), sum('inline' in d for d in v)) for fn, v in CALL_SITES.items()}
    assert found == want, 'fast_div call sites changed: list the new divisor in CALL_SITES and its range in divisor_domain()\n%s' % found
    dom = divisor_domain()
    assert {d for v in CALL_SITES.values() for d in v} == set(dom)
    for name, (ds, n_end) in dom.items():
        assert 1 <= min(ds) and max(ds) <= D_DOC and n_end <= N_DOC, name


def test_fast_div_is_exact_with_the_reciprocal_and_both_neighbours():
    """Every divisor 1 .. 4096 over the whole documented domain n < 2^19 (a superset of every call site's, see divisor_domain), with
    1/d rounded to float32 and moved one ulp either way."""
    bad = []
    for d in range(1, D_DOC + 1):
        n = boundaries(d, N_DOC)
        for inv in reciprocals(d):
            got = fast_div(n, inv)
            if not np.array_equal(got, n // d):
                bad.append((d, float(inv), int(n[np.argmax(got != n // d)])))
    assert not bad, '%d (divisor, reciprocal) pairs wrong, first (d, 1/d, n): %s' % (len(bad), bad[:5])


def test_fast_div_full_sweep_of_the_odd_inner_widths():
    """The boundary argument above, checked by brute force where a GPU case runs it: every n of the unit split (K / 2) and the piece
    split (K / 4) at the K that are no power of two, very small or large, and at the largest K of F = 64."""
    for F, K in ((3, 4), (7, 12), (10, 20), (6, 36), (5, 100), (10, 128), (64, 8), (64, k_max(64)), (2, k_max(2))):
        for d, n_end in ((K // 2, F * (F - 1) // 2 * (K // 2)), (K // 4, F * K // 4)):
            n = np.arange(n_end)
            for inv in reciprocals(d):
                np.testing.assert_array_equal(fast_div(n, inv), n // d, err_msg='F %d K %d d %d' % (F, K, d))
    for Pp in sorted({Pp_of(F) for F in F_ALL}):
        n = np.arange(4 * Pp + 128)
        for inv in reciprocals(Pp):
            np.testing.assert_array_equal(fast_div(n, inv), n // Pp, err_msg='Pp %d' % Pp)


# ---- LDS claims -------------------------------------------------------------------------------------------------------------------
def test_lds_claims_over_the_accepted_domain():
    """Which accepted shapes pass 64 KB and a CU, from the formulas alone (the numbers DESIGN.md states)."""
    head = {(F, D): head_fwd_lds(F, D) for F in F_ALL for D in D_ALL}
    assert max(head.values()) == head[(64, 512)] == 152864 <= LDS_WHOLE_CU          # the head always fits a CU ...
    over = sorted(k for k, v in head.items() if v > LDS_DEFAULT)                     # ... but not the default 64 KB
    assert over == sorted([(F, 512) for F in range(28, 65)] + [(F, 256) for F in range(50, 65)])
    assert all((F * D + F * F > 15032) == (v > LDS_DEFAULT) for (F, D), v in head.items())
    # inner branch: K is unbounded, so every F has a K beyond the CU; the backward (5 F K floats) gets there first, at F K = 7560 ..
    # 8160 (the pair table of Pp words shifts it with F)
    for F in F_ALL:
        K = k_max(F)
        assert inner_fwd_lds(F, K) < inner_bwd_lds(F, K) <= LDS_WHOLE_CU < inner_bwd_lds(F, K + 4)
        assert 7560 <= F * K <= 8160
    assert (k_max(2), k_max(10), k_max(32), k_max(34), k_max(40), k_max(64)) == (4080, 812, 252, 236, 200, 120)
    # within k_max the forward stays below 64 KB (38,848 bytes at the most), the backward passes it from F K ~ 3000 on (F = 64: K = 48)
    assert max(inner_fwd_lds(F, k_max(F)) for F in F_ALL) == 38848 <= LDS_DEFAULT
    assert inner_bwd_lds(64, 48) > LDS_DEFAULT >= inner_bwd_lds(64, 44)


# the layer-0 conv launchers of csrc/conv.hip that go through set_lds with an embedding tile [n_ex][F][D + 1] (bytes; the fp32 loops)
KSTEP, WG_KM, WGT_SUB = 32, 64, 256
FWD_ROWS, FWD_TAPS, FWD_TILE, FWD_DIRECT, WGRAD_TAPS, WGRAD_DIRECT0, DGRAD_TAPS, DGRAD_DIRECT = 2, 3, 4, 6, 2, 5, 1, 3


def _emb(Pp, n_ex, F, D):
    return Pp + n_ex * F * (D + 1)


def _fwd_ex(BM, S2):
    return BM // S2 if BM > S2 else 1


def conv0_lds(F, D, ch):
    """{role: bytes} of the layer-0 instances cffm_conv_choice reports in ch, by the formulas of their launchers."""
    Pp, S2, So = Pp_of(F), (D // 2) ** 2, D // 2
    lg = So.bit_length() - 1
    out = {}
    f, w, d = ch.fwd, ch.wgrad, ch.dgrad
    if f.family == FWD_TAPS:
        PP = f.NT * 16
        out['fwd'] = max(4 * PP * (PP + 4) * 4, 4 * f.RM * f.NT * 64 * 16) + _emb(PP, _fwd_ex(16 * f.RM, S2), F, D) * 4 + 16
    elif f.family == FWD_ROWS:
        PP = f.NT * 16
        out['fwd'] = 4 * PP * PP * 4 + _emb(PP, _fwd_ex(64, S2), F, D) * 4 + 16
    elif f.family == FWD_TILE:
        out['fwd'] = (2 * F * 272 + F * (D + 1) + 8 * So) * 4 + 16
    elif f.family == FWD_DIRECT:
        out['fwd'] = (2 * KSTEP * (f.NT * 16 + 4) + _emb(Pp, _fwd_ex(64 * f.RM, S2), F, D) + 4) * 4
    if w.family == WGRAD_TAPS:
        n_ex = WGT_SUB // S2 + 2
        out['wgrad'] = (WGT_SUB * w.NT * 16 + w.NT * 16 + (n_ex * F * (D + 1) + 7) // 4 * 4) * 4 + 16 + \
            ((4 * w.NT * w.NT * 64 * 16 + w.NT * 64 * 4) if w.HALVES == 2 else 0)
    elif w.family == WGRAD_DIRECT0:
        out['wgrad'] = (WG_KM * (w.NT * 16 + (0 if w.NT & 1 else 16)) + _emb(Pp, _fwd_ex(WG_KM, S2), F, D) + 4) * 4
    if d.family == DGRAD_TAPS:
        PP, n_ex = d.NT * 16, max(S2, 64) // S2
        scratch = (4 + 4 * d.HALVES) * PP * So if 4 <= lg <= 6 else 4 * d.HALVES * n_ex * F * (D + 1)
        out['dgrad'] = (PP + n_ex * F * (D + 1) + 2 * n_ex * F + scratch) * 4 + 16
    elif d.family == DGRAD_DIRECT:
        n_ex = max(S2, 64 * d.RM) // S2
        out['dgrad'] = (2 * KSTEP * 132 + Pp + 5 * n_ex * F * (D + 1) + 2 * n_ex * F + 4) * 4
    return out


def conv_refused(B):
    """{(F, D): role with the largest claim} of the accepted shapes whose layer-0 instance at batch B asks for more than a CU."""
    _lib()
    out = {}
    for D in D_ALL:
        for F in F_ALL:
            need = conv0_lds(F, D, hip.conv_choice(_shape(F, 8, D), B, 0))
            if need and max(need.values()) > LDS_WHOLE_CU:
                out[(F, D)] = max(need, key=need.get)
    return out


def _ranges(fs):
    out = []
    for f in sorted(fs):
        if out and out[-1][1] == f - 1:
            out[-1][1] = f
        else:
            out.append([f, f])
    return [tuple(r) for r in out]


# D -> ranges of F whose layer-0 input gradient cannot fit a CU, at every B.  Wide filters: the direct kernel keeps
# five copies of the embedding tile, 5 F (D + 1) floats (F >= 49 at D = 128, F >= 25 at D = 256, F >= 13 at D = 512).  Narrow filters:
# F = 11 at D = 128 is the fast path's T planes, 12 x 64 x 64 floats; F = 9 .. 11 at D = 512 the eight private copies of [F][D + 1].
CONV_REFUSED = {128: [(11, 11), (49, 64)], 256: [(25, 64)], 512: [(9, 11), (13, 64)]}
# ... and from 32768 rows of the outer-product map on (128-row tiles: 32 examples of D = 4 per workgroup)
CONV_REFUSED_MANY_ROWS = {4: [(37, 64)], **CONV_REFUSED}


def test_conv_lds_claims_over_the_accepted_domain():
    """The (F, D) the conv stack cannot run, from the launchers' formulas and the library's own choice of instance."""
    for B, want in ((1, CONV_REFUSED), (8, CONV_REFUSED), (8192, CONV_REFUSED_MANY_ROWS)):
        bad = conv_refused(B)
        assert {D: _ranges(F for F, d in bad if d == D) for D in sorted({d for _, d in bad})} == want, B
        assert set(bad.values()) == {'dgrad'}


def test_shapes_beyond_a_cu_are_refused_before_any_launch():
    """The stage entry points return CFFM_ERR_UNSUPPORTED on the host: these calls run without a GPU (theta, ws and y below are never
    dereferenced on the host and no call here gets as far as a launch).  cffm_ws_layout stays a pure layout query and serves every
    shape the shape check accepts (tests/test_conv_choice.py asks it for the whole recorded grid)."""
    lib = _lib()
    wl = hip.WsLayout()
    th, ws, y = 0x10000, 0x20000, 0x30000
    for F in (2, 3, 10, 31, 32, 33, 63, 64):
        K = k_max(F)
        for Kbad in (K + 4, 2 * K, 1 << 20, (1 << 31) - 4):
            s = _shape(F, Kbad, 8)
            assert lib.cffm_inner_fwd(C.byref(s), th, ws, 3, None) == UNSUPPORTED
            assert lib.cffm_inner_bwd(C.byref(s), th, ws, 3, None) == UNSUPPORTED
            assert lib.cffm_head_fwd(C.byref(s), th, ws, y, 3, None) == UNSUPPORTED
            assert lib.cffm_head_bwd(C.byref(s), th, ws, y, 3, 3, None) == UNSUPPORTED
            assert lib.cffm_ws_layout(C.byref(s), 3, C.byref(wl)) == 0
    # the conv stack: every conv stage and the two composites, at both ends of every refused range
    for F, D, B in [(f, d, 1) for d, rs in CONV_REFUSED.items() for r in rs for f in r] + [(34, 256, 1), (37, 4, 8192), (64, 4, 8192)]:
        s = _shape(F, 8, D)
        live = D.bit_length() - 2
        assert lib.cffm_outer_conv0_fwd(C.byref(s), th, ws, B, None) == UNSUPPORTED, (F, D)
        assert lib.cffm_outer_conv0_bwd(C.byref(s), th, ws, B, None) == UNSUPPORTED, (F, D)
        if live > 1:
            assert lib.cffm_conv_fwd(C.byref(s), th, ws, B, live - 1, None) == UNSUPPORTED
            assert lib.cffm_conv_bwd(C.byref(s), th, ws, B, 1, None) == UNSUPPORTED
        assert lib.cffm_forward(C.byref(s), None, th, None, None, B, ws, None) == UNSUPPORTED        # a composite: before its gather
        assert lib.cffm_backward(C.byref(s), th, y, B, B, ws, None, None) == UNSUPPORTED
        assert lib.cffm_ws_layout(C.byref(s), B, C.byref(wl)) == 0
        # without the outer branch the shape has no conv stack and is served: only the refusal is checked here, nothing may launch
    assert b'unsupported' in lib.cffm_error_string(UNSUPPORTED)


# ---- coverage ledger ----------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conv_choice.json')
UNREACHED = os.path.join(ROOT, 'tests', 'golden', 'conv_unreached.json')
ROLES = ('fwd', 'wgrad', 'dgrad')
WGRAD_WGRAD2, WGRAD_WGRAD3 = 6, 7


def _records(layer, t):
    """The (role, 'l0' | 'l1+', family, NT, RM, HALVES, b3, paired) records of one recorded tuple (tests/test_conv_choice.py)."""
    return {(r, 'l0' if layer == 0 else 'l1+') + tuple(t[5 * i:5 * i + 5]) + (t[15],) for i, r in enumerate(ROLES)}


def golden_records(with_case=False):
    with open(GOLDEN) as fh:
        g = json.load(fh)
    out, first = set(), {}
    for F, D, B, act, *idx in g['cases']:
        for l, i in enumerate(idx):
            for rec in _records(l, g['tuples'][i]):
                out.add(rec)
                if rec not in first or (B, F, D) < first[rec]:
                    first[rec] = (B, F, D)
    return (out, first) if with_case else out


def first_golden_case(recs):
    first = golden_records(True)[1]
    return {r: first[r] for r in recs}


def gpu_cases():
    """(file, case, F, D, B, fp32 twin) of every case of the three GPU files that runs the conv stack."""
    from tests import test_gpu_branches, test_gpu_layers, test_gpu_parity
    out = []
    for mod in (test_gpu_layers, test_gpu_branches, test_gpu_parity):
        for name, c in mod.CASES.items():
            if c.get('outer_conv', 1):
                out.append((mod.__name__.split('.')[-1], name, c['F'], c['D'], c['B'], mod is test_gpu_layers))
    return out


def reached_records():
    _lib()
    out = set()
    for _, _, F, D, B, twin in gpu_cases():
        sh = _shape(F, D, D, M=5000, act=3, lamda_att=1.3)
        for l in range(D.bit_length() - 2):
            ch = hip.conv_choice(sh, B, l)
            t = [getattr(getattr(ch, r), f) for r in ROLES for f in ('family', 'NT', 'RM', 'HALVES', 'b3')] + [ch.paired]
            out |= _records(l, t)
            if twin and (t[4] or t[9] or t[14]):          # the CFFM_CONV_FP32=1 child of test_gpu_layers: the fp32 loops of the same tile
                t = list(t)
                t[5] = WGRAD_WGRAD2 if t[5] == WGRAD_WGRAD3 else t[5]
                t[4] = t[9] = t[14] = 0
                out |= _records(l, t)
    return out


def test_coverage_ledger_is_current():
    """tests/golden/conv_unreached.json lists exactly the records of the golden grid that no GPU case's (F, D, B) reaches."""
    with open(UNREACHED) as fh:
        listed = json.load(fh)
    assert all(isinstance(e.get('reason'), str) and len(e['reason']) > 10 and '\n' not in e['reason'] for e in listed)
    want = {tuple(e['record']) for e in listed}
    assert len(want) == len(listed), 'duplicate entries'
    gold = golden_records()
    unreached = gold - reached_records()
    assert want <= gold, 'entries that are not records of the golden grid: %s' % sorted(want - gold)
    stale = sorted(want - unreached)
    missing = sorted(unreached - want)
    assert not stale, 'listed as unreached but a GPU case reaches them now - remove them from the list: %s' % stale
    assert not missing, 'no GPU case reaches these any more and they are not listed: %s' % missing
