"""cffm_dp_apply_opt, the multi-GPU apply of every optimizer the step classes run: what it returns before any device work.  Every
pointer is NULL, so a case that got past its early returns would read through one; no kernel is launched and no GPU is needed."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cffm_amd import hip  # noqa: E402

BASE = dict(M=10, F=3, K=8, D=8, act=0, linear_att=1, inner_conv=1, outer_conv=1, loss=0, lamda_att=1.0, beta_outer=1.0, lr=0.05)
N = None


@pytest.fixture(scope='module')
def lib():
    return hip.load()


def _call(fn, s, n_rows, n_runs):
    return fn(C.byref(s), N, N, N, N, N, 8, N, n_rows, N, 8, N, n_runs, N)


def test_the_entry_point_is_declared_in_both_bindings(lib):
    assert 'cffm_dp_apply_opt' in hip.PROTOTYPES
    assert hip.PROTOTYPES['cffm_dp_apply_opt'] == hip.PROTOTYPES['cffm_dp_apply']          # the argument list of cffm_dp_apply
    assert hasattr(hip.fast(), 'cffm_dp_apply_opt')
    assert lib.cffm_abi_version() == 9                                                     # additive: the version stays


def test_adam_is_refused_right_after_the_shape_check(lib):
    s = hip.Shape(optimizer=3, **BASE)
    for n_rows, n_runs in ((24, 0), (0, 3), (0, 0)):
        assert _call(lib.cffm_dp_apply_opt, s, n_rows, n_runs) == 10002
    bad = hip.Shape(optimizer=3, **dict(BASE, F=1))                                        # the shape check comes first
    assert _call(lib.cffm_dp_apply_opt, bad, 24, 0) == 10001
    assert lib.cffm_dp_apply_opt(N, N, N, N, N, N, 8, N, 24, N, 8, N, 0, N) == 10001


@pytest.mark.parametrize('opt', [1, 2])
def test_sgd_and_momentum_make_the_shape_checks_of_cffm_dp_apply(lib, opt):
    s = hip.Shape(optimizer=opt, **BASE)
    assert _call(lib.cffm_dp_apply_opt, s, 0, 3) == 10001                                  # runs without rows
    assert _call(lib.cffm_dp_apply_opt, s, 25, 2) == 10001                                 # rows that do not divide into the runs
    assert _call(lib.cffm_dp_apply_opt, s, 8 * 3 + 1, 0) == 10001                          # more rows than the workspace holds
    assert _call(lib.cffm_dp_apply, s, 24, 0) == 10002                                     # the Adagrad entry point still refuses them


def test_adagrad_makes_every_check_before_its_first_launch(lib):
    s = hip.Shape(optimizer=0, **BASE)
    assert _call(lib.cffm_dp_apply, s, 8 * 3 + 1, 0) == 10001                              # more rows than the workspace holds
    assert _call(lib.cffm_dp_apply, s, 24, 0) == 10001                                     # NULL pointers


def test_adagrad_forwards_to_cffm_dp_apply(lib):
    s = hip.Shape(optimizer=0, **BASE)
    for n_rows, n_runs in ((0, 3), (25, 2)):
        want = _call(lib.cffm_dp_apply, s, n_rows, n_runs)
        assert want == 10001
        assert _call(lib.cffm_dp_apply_opt, s, n_rows, n_runs) == want
