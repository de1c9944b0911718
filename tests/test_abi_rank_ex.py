"""cffm_expand_candidates_ex and cffm_score_sweep_lists: what they return before any device work, through both bindings, and the
hand-written answers of the addressing rule's numpy reading (tests/_cand_ref.py).  Every refusal include/cffm_hip.h lists comes back
ahead of the first launch or HIP call, so the device pointers here are NULL or a poison address that is never read - a case that
got any further would fault on them - and no GPU is needed.  `fields` is a HOST list: it is real memory."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cffm_amd import hip  # noqa: E402
from tests import _cand_ref as CR  # noqa: E402

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
    for name in ('cffm_expand_candidates_ex', 'cffm_score_sweep_lists'):
        assert name in hip.PROTOTYPES and hasattr(hip.load(), name) and hasattr(hip.fast(), name), name
    assert hip.load().cffm_abi_version() == 9                              # additive: the version stays


def expand_ex(lib, s, ctx=P, C_=4, fields=(1,), nf=None, cand=P, stride=0, N=5, first=0, rows=20, out=P):
    host = (C.c_int32 * max(1, len(fields)))(*fields) if fields is not None else None
    return lib.cffm_expand_candidates_ex(C.addressof(s) if s is not None else 0, ctx, C_, C.addressof(host) if host is not None else 0,
                                         len(fields) if nf is None else nf, cand, stride, N, first, rows, out, 0)


@pytest.mark.parametrize('null', [False, True])
def test_expand_ex_refusals(lib, null):
    s = shape()                                                            # F = 3
    ptrs = dict(ctx=0, cand=0, out=0) if null else {}                      # every device pointer NULL, or the poison address
    assert expand_ex(lib, None, **ptrs) == BAD and expand_ex(lib, shape(F=1), **ptrs) == BAD
    for kw in (dict(fields=(), nf=0), dict(fields=(1,), nf=-1),            # nf < 1
               dict(fields=(0, 1, 2, 0), nf=4),                            # nf = F + 1
               dict(fields=None, nf=1),                                    # fields == NULL
               dict(fields=(-1,)), dict(fields=(3,)), dict(fields=(0, 3)),  # a field outside [0, F)
               dict(fields=(1, 1)), dict(fields=(2, 0, 2)),                # the same field twice
               dict(N=0), dict(N=-5), dict(C_=-1),
               dict(first=-1), dict(rows=-1), dict(first=1, rows=20), dict(first=20, rows=1), dict(first=2 ** 40, rows=1),
               dict(stride=4), dict(stride=-1),                            # N * nf - 1 and a negative stride
               dict(fields=(0, 2), stride=9), dict(fields=(0, 2), stride=-1)):
        assert expand_ex(lib, s, **dict(ptrs, **kw)) == BAD, kw
    if not null:
        for kw in (dict(ctx=0), dict(cand=0), dict(out=0)):                # a NULL pointer that would be read or written
            assert expand_ex(lib, s, **kw) == BAD, kw
    # nothing to do: 0 without a launch (the pointers may then be anything, NULL included)
    assert expand_ex(lib, s, rows=0, **ptrs) == 0 and expand_ex(lib, s, rows=0, first=20, stride=5, **ptrs) == 0
    assert expand_ex(lib, s, C_=0, rows=0, ctx=0, cand=0, out=0) == 0
    assert expand_ex(lib, s, C_=0, rows=0, fields=(0, 1, 2), stride=15, **ptrs) == 0
    assert expand_ex(lib, s, C_=0, rows=1, **ptrs) == BAD                  # first + rows > C * N = 0
    assert expand_ex(lib, s, C_=0, rows=0, fields=(1, 1), **ptrs) == BAD   # the arguments are checked before the empty batch


def sweep_lists(lib, s, tab=None, theta=P, ctx=P, C_=2, field=1, cand=P, stride=5, N=5, scores=P, row_stride=5, scratch=P):
    if tab is None:
        tab = hip.Tables(P, P, P)
    return lib.cffm_score_sweep_lists(C.addressof(s) if s is not None else 0, C.addressof(tab) if tab else 0, theta, ctx, C_, field, cand,
                                      stride, N, scores, row_stride, scratch, 0)


def test_score_sweep_lists_refusals(lib):
    s = shape()
    null = dict(tab=0, theta=0, ctx=0, cand=0, scores=0, scratch=0)
    assert sweep_lists(lib, None) == BAD and sweep_lists(lib, shape(F=1)) == BAD
    # a shape that is not served (cffm_sweep_ok == 0): CFFM_ERR_UNSUPPORTED after the shape check, before any pointer is read
    # and before the other arguments are looked at
    for kw in (dict(inner_conv=0), dict(outer_conv=0), dict(D=64), dict(D=8), dict(F=11), dict(F=16)):
        bad = shape(**kw)                                                    # kept alive across the calls
        assert lib.cffm_sweep_ok(C.addressof(bad)) == 0
        assert sweep_lists(lib, bad, **null) == UNSUPPORTED, kw
        assert sweep_lists(lib, bad, field=-1, N=0, stride=-1) == UNSUPPORTED, kw
    for kw in (dict(field=-1), dict(field=3), dict(N=0), dict(N=-5), dict(C_=-1),
               dict(row_stride=4), dict(row_stride=0), dict(row_stride=-1),
               dict(stride=4), dict(stride=-1), dict(stride=1)):           # the stride rule: N - 1, negative, below N
        assert sweep_lists(lib, s, **kw) == BAD, kw
        assert sweep_lists(lib, s, **dict(null, **kw)) == BAD, kw           # with every pointer NULL: nothing was read
    for kw in (dict(tab=0), dict(tab=hip.Tables(0, P, P)), dict(tab=hip.Tables(P, 0, P)), dict(tab=hip.Tables(P, P, 0)),
               dict(theta=0), dict(ctx=0), dict(cand=0), dict(scores=0), dict(scratch=0)):
        assert sweep_lists(lib, s, **kw) == BAD, kw
        assert sweep_lists(lib, s, stride=0, **kw) == BAD, kw
    # nothing to do: 0 without a launch
    assert sweep_lists(lib, s, C_=0) == 0 and sweep_lists(lib, s, C_=0, stride=0, **null) == 0 and sweep_lists(lib, s, C_=0, stride=7, **null) == 0
    assert sweep_lists(lib, s, C_=0, stride=4) == BAD and sweep_lists(lib, s, C_=0, N=0) == BAD      # the arguments are checked first


# ---- the numpy reading of the addressing rule, against answers written by hand ----------------------------------------------------
CTX = np.array([[10, 11, 12, 13], [20, 21, 22, 23], [30, 31, 32, 33]], dtype=np.int32)        # C = 3, F = 4


def test_ref_one_field_shared_list():
    got = CR.expand_ex_ref(CTX, [2], np.array([7, 8], dtype=np.int32), 0, 2, 0, 6)
    assert got.tolist() == [[10, 11, 7, 13], [10, 11, 8, 13], [20, 21, 7, 23], [20, 21, 8, 23], [30, 31, 7, 33], [30, 31, 8, 33]]


def test_ref_two_fields_shared_list_in_the_order_of_fields():
    cand = np.array([[1, 2], [3, 4]], dtype=np.int32)                      # tuple n = (id for field 3, id for field 0)
    got = CR.expand_ex_ref(CTX[:2], [3, 0], cand.reshape(-1), 0, 2, 0, 4)
    assert got.tolist() == [[2, 11, 12, 1], [4, 11, 12, 3], [2, 21, 22, 1], [4, 21, 22, 3]]
    assert np.array_equal(got, CR.expand_tuples(CTX[:2], [3, 0], cand))


def test_ref_per_context_lists_with_a_gap_in_the_stride():
    # nf = 2, N = 2, stride 4 + 3: the 99s lie in the gap and must never show
    flat = np.array([1, 2, 3, 4, 99, 99, 99, 5, 6, 7, 8, 99, 99, 99, 9, 10, 11, 12, 99, 99, 99], dtype=np.int32)
    got = CR.expand_ex_ref(CTX, [0, 1], flat, 7, 2, 0, 6)
    assert got.tolist() == [[1, 2, 12, 13], [3, 4, 12, 13], [5, 6, 22, 23], [7, 8, 22, 23], [9, 10, 32, 33], [11, 12, 32, 33]]
    lists = np.arange(1, 13, dtype=np.int32).reshape(3, 2, 2)
    assert np.array_equal(CR.flat_lists(lists, 7, 99), flat)
    assert np.array_equal(got, CR.expand_tuples(CTX, [0, 1], lists))


def test_ref_a_piece_that_crosses_a_context_boundary():
    # nf = 1, per-context lists of N = 3 at stride 3: rows 2..4 are (context 0, n 2), (context 1, n 0), (context 1, n 1)
    flat = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9], dtype=np.int32)
    got = CR.expand_ex_ref(CTX, [1], flat, 3, 3, 2, 3)
    assert got.tolist() == [[10, 3, 12, 13], [20, 4, 22, 23], [20, 5, 22, 23]]
    last = CR.expand_ex_ref(CTX, [1], flat, 3, 3, 8, 1)                     # the last row alone
    assert last.tolist() == [[30, 9, 32, 33]]
