"""The candidate-ranking entry points (cffm_expand_candidates, cffm_topk_scratch_bytes, cffm_topk, cffm_rank_of): what they return
before any device work, through both bindings.  Every refusal include/cffm_hip.h lists comes back as CFFM_ERR_BAD_SHAPE ahead of
the first launch or HIP call, so the pointers here are dummies that are never read - a case that got any further would fault on
them - and no GPU is needed."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cffm_amd import hip  # noqa: E402

BASE = dict(M=10, F=3, K=8, D=8, act=0, linear_att=1, inner_conv=1, outer_conv=1, loss=0, lamda_att=1.0, beta_outer=1.0, lr=0.05)
BAD, P = 10001, 0x1000            # P: a non-NULL address nobody may read


@pytest.fixture(scope='module', params=['ctypes', 'pybind11'])
def lib(request):
    hip.load()
    if request.param == 'ctypes':
        return hip.load()
    assert hip.binding_name() == 'pybind11', 'cffm_amd/lib/_cffm_pybind*.so is not built (make)'
    return hip.fast()


@pytest.fixture(scope='module')
def shape():
    s = hip.Shape(optimizer=0, **BASE)
    bad = hip.Shape(optimizer=0, **dict(BASE, F=1))
    return s, bad


def test_the_entry_points_are_declared_in_both_bindings():
    for name in ('cffm_expand_candidates', 'cffm_topk_scratch_bytes', 'cffm_topk', 'cffm_rank_of'):
        assert name in hip.PROTOTYPES and hasattr(hip.load(), name) and hasattr(hip.fast(), name), name
    assert hip.load().cffm_abi_version() == 9                              # additive: the version stays
    header = open(os.path.join(ROOT, 'include', 'cffm_hip.h')).read()
    assert 'Additive entry points: CFFM_ABI_VERSION stays 9' in header


def expand(lib, s, ctx=P, C_=4, field=1, cand=P, N=5, first=0, rows=20, out=P):
    return lib.cffm_expand_candidates(C.addressof(s) if s is not None else 0, ctx, C_, field, cand, N, first, rows, out, 0)


def test_expand_refusals(lib, shape):
    s, bad = shape
    assert expand(lib, None) == BAD and expand(lib, bad) == BAD
    for kw in (dict(ctx=0), dict(cand=0), dict(out=0),                       # a NULL pointer that would be read or written
               dict(field=-1), dict(field=3),                                # field outside [0, F)
               dict(N=0), dict(N=-5),
               dict(first=-1), dict(rows=-1), dict(first=1, rows=20), dict(first=20, rows=1), dict(first=2 ** 40, rows=1),
               dict(C_=-1)):
        assert expand(lib, s, **kw) == BAD, kw
    # nothing to do: 0 without a launch (the pointers may then be anything, NULL included)
    assert expand(lib, s, rows=0) == 0 and expand(lib, s, rows=0, first=20) == 0
    assert expand(lib, s, C_=0, rows=0, ctx=0, cand=0, out=0) == 0
    assert expand(lib, s, C_=0, rows=1) == BAD                               # first + rows > C * N = 0


def topk(lib, scores=P, row_stride=9, skip=0, skip_stride=0, C_=2, N=9, k=3, scratch=P, idx=P, val=P, count=P):
    return lib.cffm_topk(scores, row_stride, skip, skip_stride, C_, N, k, scratch, idx, val, count, 0)


def test_topk_refusals(lib):
    for kw in (dict(scores=0), dict(scratch=0), dict(idx=0), dict(val=0), dict(count=0),
               dict(N=0), dict(k=0), dict(k=-1), dict(k=1025), dict(C_=-1),
               dict(row_stride=8), dict(skip=P, skip_stride=8), dict(skip=P, skip_stride=0)):
        assert topk(lib, **kw) == BAD, kw
    assert topk(lib, C_=0) == 0 and topk(lib, C_=0, scores=0, scratch=0, idx=0, val=0, count=0) == 0
    assert topk(lib, C_=0, k=1025) == BAD                                    # the arguments are checked before the empty batch


def rank_of(lib, scores=P, row_stride=9, skip=0, skip_stride=0, C_=2, N=9, target=P, out=P):
    return lib.cffm_rank_of(scores, row_stride, skip, skip_stride, C_, N, target, out, 0)


def test_rank_of_refusals(lib):
    for kw in (dict(scores=0), dict(target=0), dict(out=0), dict(N=0), dict(C_=-1),
               dict(row_stride=8), dict(skip=P, skip_stride=8)):
        assert rank_of(lib, **kw) == BAD, kw
    assert rank_of(lib, C_=0) == 0 and rank_of(lib, C_=0, scores=0, target=0, out=0) == 0


def test_scratch_bytes(lib):
    f = lib.cffm_topk_scratch_bytes
    for args in ((1, 0, 1), (1, 5, 0), (1, 5, 1025), (-1, 5, 3), (1, -1, 3)):
        assert f(*args) < 0, args
    assert f(0, 5, 3) > 0
    for C_, k in ((1, 1), (1, 1024), (3, 7), (130, 64)):
        last = 0
        for N in (1, 63, 64, 65, 8191, 8192, 8193, 16401, 70001, 1 << 20, (1 << 31) - 1):
            b = f(C_, N, k)
            assert b > 0 and b >= last, (C_, N, k, b, last)
            last = b
    # two levels: the k survivors of both chunks of every row; three levels (the second still has two chunks): a second buffer
    assert f(3, 8193, 7) >= 3 * 2 * 7 * 8
    assert f(1, 70001, 1024) >= (9 + 2) * 1024 * 8
