"""The fused list step's entry points before any device work, through both bindings: cffm_list_step_ok (host only), and the refusals
of cffm_backward_dout_fused and cffm_train_step_lists, all of which come back ahead of the first launch - so the device pointers
here are NULL or a poison address nobody reads, and no GPU is needed."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cffm_amd import hip  # noqa: E402

RELU, ELU, SELU, GELU = 0, 2, 3, 4
SQUARE, MSE, MAE, LOG, SQUARE_L2, HYBRID = 0, 1, 2, 3, 4, 5
ADAGRAD, SGD, MOMENTUM, ADAM = 0, 1, 2, 3
BAD, UNSUPPORTED, P = 10001, 10002, 0x1000            # P: a non-NULL address nobody may read
NAMES = ('cffm_list_step_ok', 'cffm_backward_dout_fused', 'cffm_train_step_lists')


@pytest.fixture(scope='module', params=['ctypes', 'pybind11'])
def lib(request):
    hip.load()
    if request.param == 'ctypes':
        return hip.load()
    assert hip.binding_name() == 'pybind11', 'cffm_amd/lib/_cffm_pybind*.so is not built (make)'
    return hip.fast()


def shape(F=10, D=32, K=None, act=SELU, **kw):
    d = dict(M=60 * F, F=F, K=D if K is None else K, D=D, act=act, linear_att=1, inner_conv=1, outer_conv=1, loss=SQUARE, lamda_att=1.0,
             beta_outer=1.0, lr=0.05, lamda=0.0, optimizer=ADAGRAD)
    d.update(kw)
    return hip.Shape(**d)


def ok(lib, s, B):
    return lib.cffm_list_step_ok(C.addressof(s) if s is not None else 0, B)


def test_the_entry_points_are_declared_in_both_bindings():
    for name in NAMES:
        assert name in hip.PROTOTYPES and hasattr(hip.load(), name) and hasattr(hip.fast(), name), name
    assert hip.load().cffm_abi_version() == hip.fast().cffm_abi_version() == hip.ABI_VERSION == 9      # additive: the version stays
    header = open(os.path.join(ROOT, 'include', 'cffm_hip.h')).read()
    assert '#define CFFM_ABI_VERSION 9' in header
    section = header[header.index('the fused list step'):]
    assert 'Additive entry points: CFFM_ABI_VERSION stays 9' in section[:section.index('int cffm_list_step_ok(')]
    for name in NAMES:
        assert 'int %s(' % name in section, name


# (shape, B) the fused list step serves: what the issue's table names, and the edges of B
SERVED = [
    ('frappe B=256', dict(), 256),
    ('frappe B=1', dict(), 1),
    ('frappe B=64', dict(), 64),
    ('f11-d32 (Pp = 64) B=64', dict(F=11), 64),
    ('f6-d64', dict(F=6, D=64, act=ELU), 70),
    ('f4-d8 (live = 2)', dict(F=4, D=8, act=RELU), 24),
    ('f7-d32 gelu', dict(F=7, act=GELU), 63),
]


@pytest.mark.parametrize('label,kw,B', SERVED, ids=[c[0] for c in SERVED])
def test_list_step_ok_truth_table(lib, label, kw, B):
    assert ok(lib, shape(**kw), B) == 1
    # every loss but the regularised square loss and the log loss; linear_att off is no disabled branch
    for loss in (MSE, MAE, HYBRID):
        assert ok(lib, shape(loss=loss, **kw), B) == 1, loss
    assert ok(lib, shape(linear_att=0, **kw), B) == 1
    # the same shape: a disabled branch, the two losses, the other optimizers, a B beyond the fused top
    assert ok(lib, shape(inner_conv=0, **kw), B) == 0 and ok(lib, shape(outer_conv=0, **kw), B) == 0
    assert ok(lib, shape(loss=SQUARE_L2, lamda=0.01, **kw), B) == 0
    assert ok(lib, shape(loss=LOG, **kw), B) == 0
    for opt in (SGD, MOMENTUM, ADAM):
        assert ok(lib, shape(optimizer=opt, **kw), B) == 0, opt
    for b in (257, 260, 1024, 0, -1):
        assert ok(lib, shape(**kw), b) == 0, b


def test_list_step_ok_outside_the_fused_launches(lib):
    assert ok(lib, shape(), 257) == 0                         # frappe: one workgroup per example up to 256
    assert ok(lib, shape(F=4, D=4, act=RELU), 24) == 0        # live = 1: no fused top
    assert ok(lib, shape(F=32), 64) == 0                      # wide (Pp = 496)
    assert ok(lib, shape(F=12), 64) == 0                      # Pp = 80
    assert ok(lib, None, 64) == 0 and ok(lib, shape(F=1), 64) == 0 and ok(lib, shape(D=24), 64) == 0     # the shape check refuses


def bwd(lib, s, theta=P, dout=P, B=8, ws=P, grad=P):
    return lib.cffm_backward_dout_fused(C.addressof(s) if s is not None else 0, theta, dout, B, ws, grad, 0)


def test_backward_dout_fused_refusals(lib):
    s = shape()
    null = dict(theta=0, dout=0, ws=0, grad=0)
    for kw in ({}, null, dict(B=0)):
        assert bwd(lib, None, **kw) == BAD and bwd(lib, shape(F=1), **kw) == BAD, kw
    for B in (0, -1):
        assert bwd(lib, s, B=B) == 0 and bwd(lib, s, B=B, **null) == 0
    for kw in (dict(theta=0), dict(dout=0), dict(ws=0), dict(grad=0), null):
        assert bwd(lib, s, **kw) == BAD, kw
    # where cffm_backward does not take the fused top: refused before anything is read or launched
    for other, B in ((shape(), 257), (shape(F=12), 8), (shape(F=32), 8), (shape(F=4, D=4), 8), (shape(inner_conv=0), 8),
                     (shape(outer_conv=0), 8), (shape(loss=SQUARE_L2, lamda=0.01), 8), (shape(K=1024), 8)):
        assert bwd(lib, other, B=B) == UNSUPPORTED, (other.F, other.D, B)


def step(lib, s, G=4, Lg=4, kind=0, nf=1, fields=None, stride=None, **ptr):
    p = dict(tab=P, tab_acc=P, theta=P, theta_acc=P, grad=P, ctx=P, cand=P, target=P, ids_out=P, dout=P, terms=P, ws=P, loss=P, scratch=P)
    p.update(ptr)
    host = (C.c_int32 * max(nf, 1))(*(fields if fields is not None else range(max(nf, 1))))
    fp = ptr.get('fields_ptr', C.addressof(host))
    return lib.cffm_train_step_lists(C.addressof(s) if s is not None else 0, p['tab'], p['tab_acc'], p['theta'], p['theta_acc'],
                                     p['grad'], p['ctx'], G, fp, nf, p['cand'], Lg * nf if stride is None else stride, Lg, p['target'],
                                     kind, p['ids_out'], p['dout'], p['terms'], p['ws'], p['loss'], p['scratch'], 0)


def test_train_step_lists_refusals(lib):
    s = shape()
    assert step(lib, None) == BAD and step(lib, shape(F=1)) == BAD
    assert step(lib, s, G=0) == 0 and step(lib, s, G=-2) == 0
    for kw in (dict(Lg=1), dict(Lg=0), dict(kind=2), dict(kind=-1)):
        assert step(lib, s, **kw) == BAD, kw
    # not served: nothing launched, whatever the pointers
    for other, G, Lg in ((s, 65, 4), (s, 2 ** 30, 4), (shape(F=12), 4, 4), (shape(optimizer=ADAM), 4, 4), (shape(loss=LOG), 4, 4),
                         (shape(loss=SQUARE_L2, lamda=0.01), 4, 4), (shape(inner_conv=0), 4, 4)):
        assert lib.cffm_list_step_ok(C.addressof(other), min(G * Lg, 2 ** 31 - 1)) == 0
        assert step(lib, other, G=G, Lg=Lg) == UNSUPPORTED, (G, Lg)
    for name in ('tab', 'tab_acc', 'theta', 'theta_acc', 'grad', 'ctx', 'cand', 'target', 'ids_out', 'dout', 'terms', 'ws', 'loss',
                 'scratch'):
        assert step(lib, s, **{name: 0}) == BAD, name
    assert step(lib, s, fields_ptr=0) == BAD
    # what the expansion refuses, before its launch (the first of the step)
    assert step(lib, s, nf=0) == BAD and step(lib, s, nf=11) == BAD
    assert step(lib, s, nf=2, fields=[3, 3]) == BAD and step(lib, s, fields=[10]) == BAD and step(lib, s, fields=[-1]) == BAD
    assert step(lib, s, stride=3) == BAD and step(lib, s, stride=-4) == BAD
