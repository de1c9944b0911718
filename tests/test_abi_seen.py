"""cffm_seen_mask: what it returns before any device work, through both bindings.  Every refusal include/cffm_hip.h lists comes back
ahead of the launch, so the device pointers here are NULL or a poison address that is never read - a case that got any further would
fault on them - and no GPU is needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cffm_amd import hip  # noqa: E402

BAD, P, Q = 10001, 0x1000, 0x2000             # P, Q: non-NULL addresses nobody may read
I32 = 2 ** 31 - 1


@pytest.fixture(scope='module', params=['ctypes', 'pybind11'])
def lib(request):
    hip.load()
    if request.param == 'ctypes':
        return hip.load()
    assert hip.binding_name() == 'pybind11', 'cffm_amd/lib/_cffm_pybind*.so is not built (make)'
    return hip.fast()


def test_the_entry_point_is_declared_in_both_bindings():
    import ctypes as C
    assert 'cffm_seen_mask' in hip.PROTOTYPES and hasattr(hip.load(), 'cffm_seen_mask') and hasattr(hip.fast(), 'cffm_seen_mask')
    res, args = hip.PROTOTYPES['cffm_seen_mask']
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                       C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    assert hip.load().cffm_abi_version() == hip.fast().cffm_abi_version() == hip.ABI_VERSION == 9      # additive: the version stays
    header = open(os.path.join(ROOT, 'include', 'cffm_hip.h')).read()
    start = header.index('the skip mask of a ranking call from a sparse "seen" relation')
    assert header.index('int cffm_train_step_lists_logq(') < start < header.index('peak probes')       # a section of its own, in place
    section = header[start:]
    assert 'Additive entry point: CFFM_ABI_VERSION stays 9' in section[:section.index('int cffm_seen_mask(')]
    assert section.index('int cffm_seen_mask(') < section.index('/* ----')
    assert '#define CFFM_ABI_VERSION 9' in header
    src = open(os.path.join(ROOT, 'cffm_amd', 'csrc_host', 'pybind_module.cpp')).read()
    assert 'CFFM_BIND(cffm_seen_mask);' in src
    assert os.path.exists(os.path.join(ROOT, 'cffm_amd', 'csrc', 'seen.hip'))


def mask(lib, off=P, pos=P, R=3, nnz=5, row=P, skip_in=0, skip_in_stride=0, C=4, N=7, mask_out=Q, mask_stride=7):
    return lib.cffm_seen_mask(off, pos, R, nnz, row, skip_in, skip_in_stride, C, N, mask_out, mask_stride, 0)


def test_refusals_in_the_order_of_the_contract(lib):
    # 1. a NULL pointer that would be read or written, whatever the sizes are; pos may be NULL only with nnz == 0
    for kw in (dict(off=0), dict(row=0), dict(mask_out=0), dict(pos=0), dict(pos=0, nnz=1), dict(pos=0, nnz=-1),
               dict(off=0, pos=0, row=0, mask_out=0)):
        assert mask(lib, **kw) == BAD, kw
        assert mask(lib, **dict(kw, C=0)) == BAD, kw                             # ahead of the empty call
        assert mask(lib, **dict(kw, skip_in=P, skip_in_stride=7)) == BAD, kw
    # 2. the sizes
    for kw in (dict(N=0), dict(N=-1), dict(N=-(2 ** 31)), dict(C=-1), dict(C=-(2 ** 31)), dict(R=-1), dict(R=-(2 ** 31)), dict(nnz=-1),
               dict(nnz=-(2 ** 63))):
        assert mask(lib, **kw) == BAD, kw
        if 'C' not in kw:
            assert mask(lib, **dict(kw, C=0)) == BAD, kw
    # 3. mask_stride < N
    for kw in (dict(mask_stride=6), dict(mask_stride=0), dict(mask_stride=-7), dict(N=I32, mask_stride=I32 - 1)):
        assert mask(lib, **kw) == BAD and mask(lib, **dict(kw, C=0)) == BAD, kw
    # 4. skip_in_stride < N with a skip_in; without one the stride is not looked at
    for st in (6, 0, -1):
        assert mask(lib, skip_in=P, skip_in_stride=st) == BAD and mask(lib, skip_in=P, skip_in_stride=st, C=0) == BAD, st
        assert mask(lib, skip_in=0, skip_in_stride=st, C=0) == 0, st
    # 5. the mask in place of its own input
    assert mask(lib, skip_in=Q, skip_in_stride=7) == BAD and mask(lib, skip_in=Q, skip_in_stride=7, C=0) == BAD


def test_the_empty_call_returns_0_without_a_launch(lib):
    # every pointer is poison: a launch would fault
    assert mask(lib, C=0) == 0
    assert mask(lib, C=0, pos=0, nnz=0) == 0                                      # an empty relation needs no pos
    assert mask(lib, C=0, R=0, nnz=0, N=1, mask_stride=1) == 0
    assert mask(lib, C=0, R=I32, nnz=2 ** 62, N=I32, mask_stride=2 ** 62, skip_in=P, skip_in_stride=I32) == 0
