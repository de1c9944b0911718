"""CPU: the host side of the tuple sweep's C ABI (include/cffm_hip.h: cffm_sweep_tuples_ok, cffm_sweep_tuples_scratch_bytes,
cffm_score_sweep_tuples, cffm_sweep_tuples_block_layout) through both bindings - every refusal with NULL device pointers, so that a
call that got as far as a launch would read through one; the served / unserved table; the scratch size; the block layout."""
import ctypes as C
import itertools

import pytest

from cffm_amd import hip
from cffm_amd.spec import CFFMConfig

BAD, UNSUPPORTED = 10001, 10002


@pytest.fixture(scope='module')
def libs():
    lib = hip.load()
    fast = hip.fast()
    assert hip.binding_name() == 'pybind11'
    return lib, fast


def shape(F=10, K=32, D=32, **kw):
    return hip.make_shape(CFFMConfig(M=100, F=F, K=K, D=D, **kw))


def both(libs, name, sh, *rest):
    """The same call through ctypes and through pybind11 (pointers as integers); the two must agree."""
    lib, fast = libs
    a = getattr(lib, name)(C.byref(sh), *rest)
    b = getattr(fast, name)(C.addressof(sh), *[0 if r is None else (C.addressof(r) if isinstance(r, C.Array) else r) for r in rest])
    assert a == b, (name, a, b)
    return a


def score(libs, sh, fields, nf, N=5, Cn=2, stride=0, row_stride=None, ptr=None):
    """cffm_score_sweep_tuples with every device pointer NULL (or `ptr`)."""
    fl = None if fields is None else (C.c_int32 * max(1, len(fields)))(*fields)
    tab = hip.Tables(ptr, ptr, ptr)
    lib, fast = libs
    rs = N if row_stride is None else row_stride
    a = lib.cffm_score_sweep_tuples(C.byref(sh), C.byref(tab), ptr, ptr, Cn, fl, nf, ptr, stride, N, ptr, rs, ptr, None)
    b = fast.cffm_score_sweep_tuples(C.addressof(sh), C.addressof(tab), ptr or 0, ptr or 0, Cn, 0 if fl is None else C.addressof(fl), nf,
                                     ptr or 0, stride, N, ptr or 0, rs, ptr or 0, 0)
    assert a == b, (a, b)
    return a


def test_served_table(libs):
    ok = lambda sh, nf: both(libs, 'cffm_sweep_tuples_ok', sh, nf)
    frappe = shape(10, 32)
    assert ok(frappe, 1) == 1 and ok(frappe, 2) == 1                       # nf = 2 at the frappe shape
    assert ok(frappe, 4) == 0                                              # 4 fields of Pp = 48 do not fit a CU
    for F, K in ((2, 8), (3, 8), (6, 8), (6, 32), (8, 16), (8, 32)):       # Pp <= 32: every nf <= min(F, 4)
        for nf in range(1, 7):
            assert ok(shape(F, K), nf) == (1 if nf <= min(F, hip.SWEEP_MAX_NF) else 0), (F, K, nf)
    for F in range(2, 11):                                                 # nf = 2 wherever the single-field sweep is served at K = 32
        assert ok(shape(F, 32), 2) == 1, F
    for sh in (frappe, shape(6, 8)):
        assert ok(sh, 5) == 0 and ok(sh, 0) == 0 and ok(sh, -1) == 0       # nf = 5 and less than one field
    assert ok(shape(3, 8), 4) == 0                                         # nf > F
    assert ok(shape(6, 8, D=64), 2) == 0 and ok(shape(11, 8), 2) == 0      # where the single-field sweep is not served either
    for sh in (frappe, shape(6, 8), shape(6, 8, D=64), shape(11, 8), shape(10, 64), shape(4, 8, D=8)):
        assert ok(sh, 1) == both(libs, 'cffm_sweep_ok', sh)                # nf = 1 is the single-field domain
    # whatever the answer at nf = 3, Pp = 48: the scratch query, the layout and the call agree with it
    three = ok(frappe, 3)
    bl = hip.SweepTuplesBlock()
    assert (both(libs, 'cffm_sweep_tuples_scratch_bytes', frappe, 3, 2) > 0) == bool(three)
    assert (libs[0].cffm_sweep_tuples_block_layout(C.byref(frappe), 3, C.byref(bl)) == 0) == bool(three)
    assert score(libs, frappe, (1, 6, 8), 3) == (BAD if three else UNSUPPORTED)


def test_served_boundaries_in_K(libs):
    """The last K served per (F, nf) that DESIGN.md 3.6.2 states, each with its first unserved neighbour: the candidate role's one
    LDS formula decides them, to the byte (one field at F = 10, K = 408 has 96 bytes to spare)."""
    ok = lambda F, K, nf: both(libs, 'cffm_sweep_tuples_ok', shape(F, K), nf)
    for F, nf, last in ((10, 1, 408), (10, 2, 160), (10, 3, 24), (9, 3, 28), (8, 4, 448)):
        assert ok(F, last, nf) == 1 and ok(F, last + 4, nf) == 0, (F, nf, last)
        assert both(libs, 'cffm_sweep_tuples_scratch_bytes', shape(F, last), nf, 1) > 0
        assert both(libs, 'cffm_sweep_tuples_scratch_bytes', shape(F, last + 4), nf, 1) < 0
    assert both(libs, 'cffm_sweep_ok', shape(10, 408)) == 1 and both(libs, 'cffm_sweep_ok', shape(10, 412)) == 0


def test_refusals_come_before_any_launch(libs):
    sh = shape(6, 8)
    bad_shape = hip.Shape(M=10, F=1, K=8, D=8, act=0, linear_att=1, inner_conv=1, outer_conv=1, loss=0, lamda_att=1.0, beta_outer=1.0, lr=0.05)
    cases = [
        (bad_shape, (0,), 1, {}, BAD),                                     # the shape check is first
        (shape(6, 8, D=64), (9, 9), 2, {}, UNSUPPORTED),                   # then the single-field domain, before the fields are read
        (shape(11, 8), (0, 1), 2, {}, UNSUPPORTED),
        (sh, (0, 1), 0, {}, BAD), (sh, (0, 1), -1, {}, BAD), (sh, tuple(range(6)) + (0,), 7, {}, BAD),      # nf < 1, nf > F
        (sh, None, 2, {}, BAD),                                            # fields == NULL
        (sh, (0, 6), 2, {}, BAD), (sh, (-1, 2), 2, {}, BAD), (sh, (3, 3), 2, {}, BAD),   # outside [0, F), the same field twice
        (sh, (0, 1, 2, 3, 3), 5, {}, BAD),                                 # ... seen before nf = 5 is found unserved
        (sh, (0, 1, 2, 3, 4), 5, {}, UNSUPPORTED),                         # nf > CFFM_SWEEP_MAX_NF
        (shape(10, 32), (0, 1, 2, 3), 4, {}, UNSUPPORTED),                 # the candidate role's LDS
        (sh, (0, 1), 2, dict(N=0), BAD), (sh, (0, 1), 2, dict(Cn=-1), BAD), (sh, (0, 1), 2, dict(row_stride=4), BAD),
        (sh, (0, 1), 2, dict(stride=-1), BAD), (sh, (0, 1), 2, dict(stride=9), BAD),     # a non-zero stride below N * nf = 10
        (sh, (0,), 1, dict(stride=4), BAD),
        (sh, (0, 1), 2, dict(Cn=0), 0), (sh, (0, 1), 2, dict(Cn=0, stride=10), 0),       # C == 0: nothing to do, no launch
        (sh, (0, 1), 2, {}, BAD), (sh, (1, 0), 2, dict(stride=10), BAD), (sh, (2,), 1, {}, BAD),    # NULL pointers of a real call
    ]
    for i, (s, fields, nf, kw, want) in enumerate(cases):
        assert score(libs, s, fields, nf, **kw) == want, (i, fields, nf, kw)
    bl = hip.SweepTuplesBlock()
    lib, fast = libs
    assert lib.cffm_sweep_tuples_block_layout(C.byref(sh), 2, None) == BAD == fast.cffm_sweep_tuples_block_layout(C.addressof(sh), 2, 0)
    assert lib.cffm_sweep_tuples_block_layout(C.byref(bad_shape), 2, C.byref(bl)) == BAD
    assert lib.cffm_sweep_tuples_block_layout(C.byref(sh), 5, C.byref(bl)) == UNSUPPORTED
    assert bytes(bl) == bytes(hip.SweepTuplesBlock())                      # *out untouched by a refusal
    with pytest.raises(RuntimeError):
        hip.sweep_tuples_block_layout(sh, 7)


def test_scratch_bytes_are_linear_in_C_and_grow_with_nf(libs):
    nbytes = lambda sh, nf, Cn: both(libs, 'cffm_sweep_tuples_scratch_bytes', sh, nf, Cn)
    for sh, top in ((shape(10, 32), 2), (shape(8, 16), 4), (shape(3, 8), 3)):
        prev = 0
        for nf in range(1, top + 1):
            b0, b1, b7 = nbytes(sh, nf, 0), nbytes(sh, nf, 1), nbytes(sh, nf, 7)
            bl = hip.sweep_tuples_block_layout(sh, nf)
            assert b0 == 4 * bl.header_floats and b1 - b0 == 4 * bl.block_floats and b7 == b0 + 7 * (b1 - b0)
            assert b1 > prev                                               # a larger nf needs a larger block
            prev = b1
        assert nbytes(sh, 1, 3) == both(libs, 'cffm_sweep_scratch_bytes', sh, 3)
        assert nbytes(sh, top, -1) < 0 and nbytes(sh, 5, 1) < 0 and nbytes(sh, 0, 1) < 0
    assert nbytes(shape(6, 8, D=64), 2, 1) < 0 and nbytes(shape(3, 8), 4, 1) < 0


def test_block_layout_members_are_disjoint_and_inside_the_block(libs):
    for (F, K), nf in itertools.product(((10, 32), (8, 16), (6, 8), (3, 8), (2, 8)), (1, 2, 3, 4)):
        sh = shape(F, K)
        if not libs[0].cffm_sweep_tuples_ok(C.byref(sh), nf):
            continue
        bl = hip.sweep_tuples_block_layout(sh, nf)
        fast_bl = hip.SweepTuplesBlock()
        assert libs[1].cffm_sweep_tuples_block_layout(C.addressof(sh), nf, C.addressof(fast_bl)) == 0 and bytes(fast_bl) == bytes(bl)
        Pp = (F * (F - 1) // 2 + 15) // 16 * 16
        assert bl.UV_stride == 2 * 16 * Pp and bl.A_stride == 32
        spans = [(bl.Z, 256 * Pp), (bl.U, nf * bl.UV_stride), (bl.V, nf * bl.UV_stride), (bl.Ei, F * K), (bl.s0fix, 32),
                 (bl.A, nf * bl.A_stride), (bl.fb, 16), (bl.scal, 16)]
        spans.sort()
        assert spans[0][0] == 0
        for (o0, n0), (o1, _) in zip(spans, spans[1:]):
            assert o0 + n0 <= o1 and o0 % 4 == 0 and o1 % 4 == 0           # disjoint, 16-byte aligned
        assert spans[-1][0] + spans[-1][1] <= bl.block_floats
        if nf == 1:                                                        # one field: the layout of cffm_sweep_block_layout
            one = hip.sweep_block_layout(sh)
            assert all(getattr(one, k) == getattr(bl, k) for k, _ in hip.SweepBlock._fields_)
