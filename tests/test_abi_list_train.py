"""cffm_backward_dout and cffm_list_loss: what they return before any device work, through both bindings.  Every refusal
include/cffm_hip.h lists comes back ahead of the first launch or HIP call, so the device pointers here are NULL or a poison address
that is never read - a case that got any further would fault on them - and no GPU is needed."""
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
    for name in ('cffm_backward_dout', 'cffm_list_loss', 'cffm_list_loss_scratch_bytes'):
        assert name in hip.PROTOTYPES and hasattr(hip.load(), name) and hasattr(hip.fast(), name), name
    assert hip.load().cffm_abi_version() == hip.fast().cffm_abi_version() == hip.ABI_VERSION == 9      # additive: the version stays
    header = open(os.path.join(ROOT, 'include', 'cffm_hip.h')).read()
    section = header[header.index('training on ranked lists'):]
    assert 'Additive entry points: CFFM_ABI_VERSION stays 9' in section[:section.index('int cffm_backward_dout(')]
    assert '#define CFFM_ABI_VERSION 9' in header
    assert 'enum { CFFM_LIST_BPR = 0, CFFM_LIST_SOFTMAX = 1 };' in header and hip.LIST_LOSS_IDS == {'bpr': 0, 'softmax': 1}


def bwd(lib, s, theta=P, dout=P, B=8, ws=P, grad=P):
    return lib.cffm_backward_dout(C.addressof(s) if s is not None else 0, theta, dout, B, ws, grad, 0)


def test_backward_dout_refusals(lib):
    s = shape()
    null = dict(theta=0, dout=0, ws=0, grad=0)
    # the shape check is the first statement: a NULL or a refused shape, whatever else is passed
    for kw in ({}, null, dict(B=0), dict(B=-3)):
        assert bwd(lib, None, **kw) == BAD and bwd(lib, shape(F=1), **kw) == BAD and bwd(lib, shape(D=24), **kw) == BAD, kw
    # an empty batch returns as cffm_backward does: 0 after the shape check, nothing read
    for B in (0, -1):
        assert bwd(lib, s, B=B) == 0 and bwd(lib, s, B=B, **null) == 0
        assert lib.cffm_backward(C.addressof(s), 0, 0, B, 8, 0, 0, 0) == 0
    for kw in (dict(theta=0), dict(dout=0), dict(ws=0), dict(grad=0), null):            # a NULL pointer
        assert bwd(lib, s, **kw) == BAD, kw
    # the LDS / route check backward_impl makes: a shape a CU's LDS cannot hold, refused as cffm_backward refuses it
    wide = shape(F=10, K=1024)
    assert bwd(lib, wide) == UNSUPPORTED
    assert lib.cffm_backward(C.addressof(wide), P, P, 8, 8, P, P, 0) == UNSUPPORTED
    # any loss id the shape check accepts is taken (it is not used): the refusals above do not depend on it
    for loss in range(6):
        assert bwd(lib, shape(loss=loss), dout=0) == BAD and bwd(lib, shape(loss=loss), B=0) == 0, loss
    assert bwd(lib, shape(loss=6)) == BAD


def ll(lib, kind=0, scores=P, G=4, Lg=5, target=P, dout=P, terms=P, loss=P, scratch=P):
    return lib.cffm_list_loss(kind, scores, G, Lg, target, dout, terms, loss, scratch, 0)


def test_list_loss_refusals(lib):
    null = dict(scores=0, target=0, dout=0, terms=0, loss=0, scratch=0)
    for kw in (dict(kind=2), dict(kind=-1), dict(kind=7),                                # unknown kind
               dict(G=-1), dict(G=-(2 ** 31)),
               dict(Lg=1), dict(Lg=0), dict(Lg=-4),
               dict(G=2 ** 30, Lg=2), dict(G=2, Lg=2 ** 30), dict(G=46341, Lg=46341), dict(G=2 ** 31 - 1, Lg=2 ** 31 - 1)):
        assert ll(lib, **kw) == BAD, kw
        assert ll(lib, **dict(null, **kw)) == BAD, kw                                    # with every pointer NULL: nothing was read
    for name in null:                                                                     # a NULL pointer that would be read or written
        for kind in (0, 1):
            assert ll(lib, kind=kind, **{name: 0}) == BAD, name
    # nothing to do: 0 without a launch, whatever the pointers; the arguments are still checked first
    for kind in (0, 1):
        assert ll(lib, kind=kind, G=0) == 0 and ll(lib, kind=kind, G=0, **null) == 0
    assert ll(lib, kind=2, G=0) == BAD and ll(lib, G=0, Lg=1) == BAD
    # the largest accepted product is 2^31 - 1: only its NULL pointers refuse it
    assert ll(lib, G=1, Lg=2 ** 31 - 1, scores=0) == BAD


def test_list_loss_scratch_bytes(lib):
    assert lib.cffm_list_loss_scratch_bytes(-1) == -1
    sizes = [lib.cffm_list_loss_scratch_bytes(G) for G in (0, 1, 4, 5, 300, 2 ** 31 - 1)]
    assert all(b > 0 and b % 8 == 0 for b in sizes) and sizes == sorted(sizes)
    assert sizes[-1] >= (2 ** 31 - 1) // 4 * 8
