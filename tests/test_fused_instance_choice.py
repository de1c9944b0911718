"""cffm_fused_instance on the CPU (include/cffm_hip.h): which launches of the fused train step run the kernel instance that has the
frappe command's shape compiled in (frappe_shape() in csrc/conv.hip: F = 10, K = 32, D = 32, selu).  Over a grid of (F, K, D, act, B)
and through both bindings: only that tuple sets a bit, and B enters only through the predicates the launches themselves ask -
cffm_fwd_all_ok (exported as cffm_dp_runs_ok) for the forward, bwd_fused01_ok (common.hpp: the fused top runs, D = 32, Pp <= 48,
64 <= B <= 256) and a loss other than square_l2 for the launch below the fused top.  Nothing is launched."""
import ctypes as C

import pytest

from cffm_amd import hip

BAD_SHAPE = 10001
FWD, BWD_TOP, CONV01 = 1, 2, 4                    # CFFM_FUSED_INSTANCE_*
SELU, LOSS_SQUARE_L2 = 3, 4
FS = (2, 9, 10, 11, 12)
KS = (4, 16, 28, 32, 36, 64)
DS = (16, 32, 64)
ACTS = (0, 1, 2, 3, 4)
BS = (1, 3, 63, 64, 65, 255, 256, 257, 300, 409, 410, 4096)


def _shape(F, K, D, act, loss=0, inner=1, outer=1):
    return hip.Shape(M=5000, F=F, K=K, D=D, act=act, linear_att=1, inner_conv=inner, outer_conv=outer, loss=loss, lamda_att=1.3,
                     beta_outer=1.0, lr=0.05, lamda=0.0, optimizer=0)


def _bindings():
    fast = hip.fast()
    assert hip.binding_name() == 'pybind11', 'cffm_amd/lib/_cffm_pybind*.so is not built (make)'
    return (('ctypes', lambda sh, B: hip.load().cffm_fused_instance(C.byref(sh), B)),
            ('pybind11', lambda sh, B: fast.cffm_fused_instance(C.addressof(sh), B)))


def _want(F, K, D, act, B, sh):
    if (F, K, D, act) != (10, 32, 32, SELU):
        return 0
    bits = FWD if hip.load().cffm_dp_runs_ok(C.byref(sh), B) else 0
    if sh.inner_conv and sh.outer_conv and 64 <= B <= 256 and sh.loss != LOSS_SQUARE_L2:
        bits |= CONV01
    return bits


def test_constants_match_the_header():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'cffm_hip.h')).read()
    got = dict(re.findall(r'#define CFFM_FUSED_INSTANCE_(\w+) (\d+)', header))
    assert got == {'FWD': str(FWD), 'BWD_TOP': str(BWD_TOP), 'CONV01': str(CONV01)}
    assert re.search(r'CFFM_LOSS_SQUARE_L2 = %d\b' % LOSS_SQUARE_L2, header) and re.search(r'CFFM_ACT_SELU = %d\b' % SELU, header)


@pytest.mark.parametrize('name', ['ctypes', 'pybind11'])
def test_only_the_frappe_tuple_sets_bits(name):
    query = dict(_bindings())[name]
    n_set = 0
    for F in FS:
        for K in KS:
            for D in DS:
                for act in ACTS:
                    sh = _shape(F, K, D, act)
                    for B in BS:
                        got = query(sh, B)
                        assert got == _want(F, K, D, act, B, sh), (F, K, D, act, B, got)
                        n_set += got != 0
    assert n_set == sum(1 for B in BS if B <= 409)         # the frappe tuple alone, wherever the fused forward runs


@pytest.mark.parametrize('name', ['ctypes', 'pybind11'])
def test_batch_enters_through_the_launch_predicates(name):
    query = dict(_bindings())[name]
    sh = _shape(10, 32, 32, SELU)
    assert [query(sh, B) for B in (1, 3, 63, 64, 256, 257, 300, 409, 410)] == [FWD, FWD, FWD, FWD | CONV01, FWD | CONV01, FWD, FWD, FWD, 0]
    # the bit of the fused top of the backward is reserved: no compiled-shape instance of that kernel exists
    assert all(query(sh, B) & BWD_TOP == 0 for B in BS)
    # the launch below the fused top is not taken on the square_l2 path; a disabled branch takes neither fused launch
    assert query(_shape(10, 32, 32, SELU, loss=LOSS_SQUARE_L2), 64) & CONV01 == 0
    assert query(_shape(10, 32, 32, SELU, inner=0), 64) == 0
    assert query(_shape(10, 32, 32, SELU, outer=0), 64) == 0


def test_bad_arguments_are_refused():
    lib = hip.load()
    ok = _shape(10, 32, 32, SELU)
    assert lib.cffm_fused_instance(C.byref(ok), 0) == BAD_SHAPE
    assert lib.cffm_fused_instance(C.byref(ok), -5) == BAD_SHAPE
    assert lib.cffm_fused_instance(None, 64) == BAD_SHAPE
    assert lib.cffm_fused_instance(C.byref(_shape(1, 32, 32, SELU)), 64) == BAD_SHAPE
    assert lib.cffm_fused_instance(C.byref(_shape(10, 32, 24, SELU)), 64) == BAD_SHAPE
    with pytest.raises(RuntimeError):
        hip.fused_instance(ok, 0)
    assert hip.fused_instance(ok, 64) == FWD | CONV01
