"""The shared candidate sweep's entry points (cffm_sweep_ok, cffm_sweep_scratch_bytes, cffm_sweep_block_layout, cffm_score_sweep): what they return before any
device work, through both bindings.  Every refusal include/cffm_hip.h lists comes back ahead of the first launch or HIP call, so
the pointers here are dummies that are never read - a case that got any further would fault on them - and no GPU is needed."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cffm_amd import hip  # noqa: E402

BASE = dict(M=100, F=3, K=8, D=32, act=0, linear_att=1, inner_conv=1, outer_conv=1, loss=0, lamda_att=1.0, beta_outer=1.0, lr=0.05)
BAD, UNSUPPORTED, P = 10001, 10002, 0x1000            # P: a non-NULL address nobody may read


@pytest.fixture(scope='module', params=['ctypes', 'pybind11'])
def lib(request):
    hip.load()
    if request.param == 'ctypes':
        return hip.load()
    assert hip.binding_name() == 'pybind11', 'cffm_amd/lib/_cffm_pybind*.so is not built (make)'
    return hip.fast()


def shape(**kw):
    return hip.Shape(optimizer=0, **dict(BASE, **kw))


def test_the_entry_points_are_declared_in_both_bindings():
    for name in ('cffm_sweep_ok', 'cffm_sweep_scratch_bytes', 'cffm_score_sweep', 'cffm_sweep_block_layout'):
        assert name in hip.PROTOTYPES and hasattr(hip.load(), name) and hasattr(hip.fast(), name), name
    assert hip.load().cffm_abi_version() == 9                              # additive: the version stays
    header = open(os.path.join(ROOT, 'include', 'cffm_hip.h')).read()
    assert '#define CFFM_SWEEP_CHUNK %d' % hip.SWEEP_CHUNK in header


def test_sweep_ok_over_shapes(lib):
    def ok(**kw):
        s = shape(**kw)                                                      # kept alive across the call
        return lib.cffm_sweep_ok(C.addressof(s))
    # the required domain: both branches, D = 32, 2 <= F <= 10, K up to 64, every activation, linear_att 0 and 1
    for F in range(2, 11):
        for K in (4, 8, 16, 32, 64):
            assert ok(F=F, K=K) == 1, (F, K)
    for act in range(5):
        for att in (0, 1):
            assert ok(F=10, K=32, act=act, linear_att=att) == 1, (act, att)
    assert ok(F=10, K=64, M=1) == 1 and ok(F=2, K=4, M=1 << 30) == 1
    # refused whatever else holds: a branch off, D outside {32, 64}, Pp > 64
    for kw in (dict(inner_conv=0), dict(outer_conv=0), dict(inner_conv=0, outer_conv=0), dict(D=8), dict(D=16), dict(D=128),
               dict(D=4), dict(F=12), dict(F=16), dict(F=33), dict(F=64)):
        assert ok(**kw) == 0, kw
    # D = 64 and F = 11 (Pp = 64) are not served by this build
    assert ok(D=64) == 0 and ok(F=11) == 0
    # a shape the shape check refuses, and no shape at all
    assert ok(F=1) == 0 and ok(K=6) == 0 and ok(D=24) == 0 and lib.cffm_sweep_ok(0) == 0
    # K beyond what the kernels' LDS holds next to their tiles
    assert ok(F=10, K=4096) == 0


def test_scratch_bytes(lib):
    f = lib.cffm_sweep_scratch_bytes
    good = shape(F=10, K=32)
    assert f(0, 4) < 0 and f(C.addressof(good), -1) < 0
    for kw in (dict(inner_conv=0), dict(D=64), dict(F=11), dict(F=1), dict(D=8)):
        s = shape(**kw)
        assert f(C.addressof(s), 4) < 0, kw
    for kw in (dict(F=2, K=4), dict(F=3), dict(F=10, K=32), dict(F=10, K=64)):
        s = shape(**kw)
        last = 0
        for C_ in (0, 1, 2, 3, 64, 4096, 1 << 20, (1 << 31) - 1):
            b = f(C.addressof(s), C_)
            assert b > 0 and b >= last, (kw, C_, b, last)
            last = b
    # a context's block holds at least Zctx [16][16][Pp], U [2][16][Pp] and V [2][16][Pp]
    assert f(C.addressof(good), 3) - f(C.addressof(good), 2) >= (256 + 64) * 48 * 4


MEMBERS = ('Z', 'U', 'V', 'Ei', 's0fix', 'A', 'fb', 'scal')


def test_block_layout(lib):
    f, nbytes = lib.cffm_sweep_block_layout, lib.cffm_sweep_scratch_bytes
    good = shape(F=10, K=32)
    untouched = hip.SweepBlock(*([-7] * 10))
    # refused where the scratch-bytes call refuses: no shape, a shape the shape check refuses, a shape that is not served, no result
    assert f(0, C.addressof(untouched)) == BAD and f(C.addressof(good), 0) == BAD
    for kw, want in ((dict(F=1), BAD), (dict(K=6), BAD), (dict(inner_conv=0), UNSUPPORTED), (dict(D=64), UNSUPPORTED), (dict(F=11), UNSUPPORTED),
                     (dict(D=8), UNSUPPORTED), (dict(F=10, K=4096), UNSUPPORTED)):
        s = shape(**kw)
        assert nbytes(C.addressof(s), 4) < 0, kw
        assert f(C.addressof(s), C.addressof(untouched)) == want, kw
    assert all(getattr(untouched, n) == -7 for n, _ in hip.SweepBlock._fields_)          # a refusal writes nothing
    for F in range(2, 11):
        for K in (4, 8, 16, 32, 64):
            s, bl = shape(F=F, K=K), hip.SweepBlock()
            assert f(C.addressof(s), C.addressof(bl)) == 0, (F, K)
            offs = [getattr(bl, n) for n in MEMBERS]
            assert offs[0] == 0 and all(a < b for a, b in zip(offs, offs[1:])) and all(o % 4 == 0 for o in offs), (F, K, offs)
            assert bl.header_floats * 4 == 256 and bl.block_floats % 4 == 0 and bl.block_floats >= bl.scal + 16, (F, K)
            Pp = (F * (F - 1) // 2 + 15) // 16 * 16
            # every tensor has room in front of the next one
            sizes = dict(Z=256 * Pp, U=32 * Pp, V=32 * Pp, Ei=F * K, s0fix=32, A=32, fb=16)
            for a, b in zip(MEMBERS, MEMBERS[1:]):
                assert getattr(bl, b) - getattr(bl, a) >= sizes[a], (F, K, a)
            for C_ in (0, 1, 3, 260, 1 << 20):
                assert (bl.header_floats + C_ * bl.block_floats) * 4 == nbytes(C.addressof(s), C_), (F, K, C_)
    bl = hip.sweep_block_layout(good)                                            # the helper the tests read the scratch through
    assert (bl.header_floats + 2 * bl.block_floats) * 4 == nbytes(C.addressof(good), 2)


def sweep(lib, s, tab=None, theta=P, ctx=P, C_=2, field=1, cand=P, N=5, scores=P, row_stride=5, scratch=P):
    if tab is None:
        tab = hip.Tables(P, P, P)
    return lib.cffm_score_sweep(C.addressof(s) if s is not None else 0, C.addressof(tab) if tab else 0, theta, ctx, C_, field, cand, N,
                                scores, row_stride, scratch, 0)


def test_score_sweep_refusals(lib):
    s = shape()
    assert sweep(lib, None) == BAD and sweep(lib, shape(F=1)) == BAD
    # a shape that is not served: CFFM_ERR_UNSUPPORTED after the shape check, before any pointer is read (all NULL here) and
    # before the other arguments are looked at
    for kw in (dict(inner_conv=0), dict(outer_conv=0), dict(D=64), dict(D=8), dict(F=11), dict(F=16)):
        assert sweep(lib, shape(**kw), tab=0, theta=0, ctx=0, cand=0, scores=0, scratch=0) == UNSUPPORTED, kw
        assert sweep(lib, shape(**kw), field=-1, N=0) == UNSUPPORTED, kw
    for kw in (dict(tab=0), dict(tab=hip.Tables(0, P, P)), dict(tab=hip.Tables(P, 0, P)), dict(tab=hip.Tables(P, P, 0)),
               dict(theta=0), dict(ctx=0), dict(cand=0), dict(scores=0), dict(scratch=0),     # a NULL pointer that would be read or written
               dict(field=-1), dict(field=3),                                                  # field outside [0, F)
               dict(N=0), dict(N=-5), dict(C_=-1),
               dict(row_stride=4), dict(row_stride=0), dict(row_stride=-1)):
        assert sweep(lib, s, **kw) == BAD, kw
    # nothing to do: 0 without a launch (the pointers may then be anything, NULL included)
    assert sweep(lib, s, C_=0) == 0
    assert sweep(lib, s, C_=0, tab=0, theta=0, ctx=0, cand=0, scores=0, scratch=0) == 0
    assert sweep(lib, s, C_=0, N=0) == BAD and sweep(lib, s, C_=0, row_stride=4) == BAD      # the arguments are checked first
