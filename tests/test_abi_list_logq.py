"""cffm_list_loss_logq and cffm_train_step_lists_logq: what they return before any device work, through both bindings.  Every refusal
include/cffm_hip.h lists comes back ahead of the launch, in the stated order, so the device pointers here are NULL or a poison
address that is never read - a case that got any further would fault on them - and no GPU is needed."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cffm_amd import hip  # noqa: E402
from cffm_amd.spec import CFFMConfig  # noqa: E402

BAD, UNS, P = 10001, 10002, 0x1000            # P: a non-NULL, 8-byte aligned address nobody may read
BPR, SOFTMAX = hip.LIST_LOSS_IDS['bpr'], hip.LIST_LOSS_IDS['softmax']


@pytest.fixture(scope='module', params=['ctypes', 'pybind11'])
def lib(request):
    hip.load()
    if request.param == 'ctypes':
        return hip.load()
    assert hip.binding_name() == 'pybind11', 'cffm_amd/lib/_cffm_pybind*.so is not built (make)'
    return hip.fast()


def test_the_entry_points_are_declared_in_both_bindings():
    for name, nargs in (('cffm_list_loss_logq', 13), ('cffm_train_step_lists_logq', 25)):
        assert name in hip.PROTOTYPES and hasattr(hip.load(), name) and hasattr(hip.fast(), name)
        assert len(hip.PROTOTYPES[name][1]) == nargs
    # the corrected step takes every argument of the uncorrected one in its order up to scratch, then lists, corr, U, stream
    a, b = hip.PROTOTYPES['cffm_train_step_lists'][1], hip.PROTOTYPES['cffm_train_step_lists_logq'][1]
    assert b[:len(a) - 1] == a[:-1] and b[len(a) - 1:] == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    assert hip.load().cffm_abi_version() == hip.fast().cffm_abi_version() == hip.ABI_VERSION == 9      # additive: the version stays
    header = open(os.path.join(ROOT, 'include', 'cffm_hip.h')).read()
    start = header.index('logQ-corrected sampled softmax over drawn lists')
    assert header.index('int cffm_pick_hard(') < start < header.index('peak probes')                   # a section of its own, in place
    section = header[start:]
    assert 'Additive entry points: CFFM_ABI_VERSION stays 9' in section[:section.index('int cffm_list_loss_logq(')]
    assert section.index('int cffm_list_loss_logq(') < section.index('int cffm_train_step_lists_logq(') < section.index('/* ----')
    assert '#define CFFM_ABI_VERSION 9' in header
    src = open(os.path.join(ROOT, 'cffm_amd', 'csrc_host', 'pybind_module.cpp')).read()
    assert 'CFFM_BIND(cffm_list_loss_logq);' in src and 'CFFM_BIND(cffm_train_step_lists_logq);' in src


# ---- cffm_list_loss_logq -----------------------------------------------------------------------------------------------------------
def loss(lib, kind=SOFTMAX, scores=P, G=4, Lg=5, target=P, lists=P, corr=P, U=9, dout=P, terms=P, out=P, scratch=P):
    return lib.cffm_list_loss_logq(kind, scores, G, Lg, target, lists, corr, U, dout, terms, out, scratch, 0)


NULLS = dict(scores=0, target=0, lists=0, corr=0, dout=0, terms=0, out=0, scratch=0)


def test_list_loss_refusals_in_their_order(lib):
    shapes = (dict(G=-1), dict(G=-(2 ** 31)), dict(Lg=1), dict(Lg=0), dict(Lg=-7), dict(G=2 ** 16, Lg=2 ** 15), dict(G=2 ** 31 - 1, Lg=2))
    # 1. an unknown kind, ahead of everything else
    for kind in (2, -1, 7, 2 ** 31 - 1, -(2 ** 31)):
        for kw in (dict(),) + shapes + (dict(U=0), dict(G=0), NULLS, dict(NULLS, G=-1, U=0)):
            assert loss(lib, kind=kind, **kw) == BAD, (kind, kw)
    # 2. BPR is refused by name, ahead of the shape
    for kw in (dict(),) + shapes + (dict(U=0), dict(G=0), NULLS, dict(NULLS, G=-1, U=-3)):
        assert loss(lib, kind=BPR, **kw) == UNS, kw
    # 3. the G / Lg / size refusals of cffm_list_loss, ahead of U, of the empty call and of the pointers
    for kw in shapes:
        assert loss(lib, **kw) == BAD, kw
        assert loss(lib, **dict(NULLS, **kw)) == BAD and loss(lib, **dict(kw, U=0)) == BAD, kw
    assert loss(lib, G=0, Lg=1) == BAD
    assert hip.load().cffm_list_loss(SOFTMAX, P, 2 ** 16, 2 ** 15, P, P, P, P, P, 0) == BAD            # the uncorrected loss's own bound
    # 4. U < 1, ahead of the empty call
    for U in (0, -1, -(2 ** 31)):
        assert loss(lib, U=U) == BAD and loss(lib, U=U, G=0) == BAD and loss(lib, U=U, **NULLS) == BAD, U
    # 5. the empty call returns 0 whatever the pointers are
    assert loss(lib, G=0) == 0 and loss(lib, G=0, **NULLS) == 0 and loss(lib, G=0, U=2 ** 31 - 1, Lg=2 ** 31 - 1) == 0
    assert loss(lib, G=0, corr=P + 4) == 0
    # 6. every pointer that would be read or written, lists and corr included; a table that is not 8-byte aligned
    for name in NULLS:
        assert loss(lib, **{name: 0}) == BAD, name
    assert loss(lib, **NULLS) == BAD
    for off in (4, 1, 2, 12):
        assert loss(lib, corr=P + off) == BAD, off
    # the largest accepted sizes: only a NULL pointer refuses them
    assert loss(lib, G=2 ** 15, Lg=2 ** 15, U=2 ** 31 - 1, scores=0) == BAD and loss(lib, G=2 ** 30 - 1, Lg=2, U=1, terms=0) == BAD


# ---- cffm_train_step_lists_logq ----------------------------------------------------------------------------------------------------
def shape_of(**kw):
    cfg = CFFMConfig(**dict(dict(M=5382, F=10, K=32, D=32, activation='selu'), **kw))
    return hip.make_shape(cfg)


@pytest.fixture(scope='module')
def frappe():
    return shape_of()


STEP_PTRS = ('tab', 'tab_acc', 'theta', 'theta_acc', 'grad', 'ctx', 'fields', 'cand', 'target', 'ids_out', 'dout', 'terms', 'ws', 'out',
             'scratch')


def step(lib, s, G=4, nf=2, cand_stride=8, Lg=4, kind=SOFTMAX, lists=P, corr=P, U=9, **ptr):
    p = dict({n: P for n in STEP_PTRS}, **ptr)
    return lib.cffm_train_step_lists_logq(C.addressof(s) if s is not None else 0, p['tab'], p['tab_acc'], p['theta'], p['theta_acc'],
                                          p['grad'], p['ctx'], G, p['fields'], nf, p['cand'], cand_stride, Lg, p['target'], kind,
                                          p['ids_out'], p['dout'], p['terms'], p['ws'], p['out'], p['scratch'], lists, corr, U, 0)


def test_step_refusals_in_their_order(lib, frappe):
    every_null = dict({n: 0 for n in STEP_PTRS}, lists=0, corr=0)
    # the shape check first
    bad_shape = shape_of()
    bad_shape.F = 1
    assert step(lib, bad_shape) == BAD and step(lib, bad_shape, kind=BPR, G=0, **every_null) == BAD
    assert step(lib, None) == BAD
    # G <= 0 returns 0, whatever follows
    for G in (0, -1, -(2 ** 31)):
        assert step(lib, frappe, G=G) == 0 and step(lib, frappe, G=G, kind=BPR, Lg=0, U=0, **every_null) == 0
    # Lg < 2 or an unknown kind
    for kw in (dict(Lg=1), dict(Lg=0), dict(Lg=-4), dict(kind=2), dict(kind=-1), dict(kind=2 ** 31 - 1)):
        assert step(lib, frappe, **kw) == BAD and step(lib, frappe, **dict(every_null, U=0, **kw)) == BAD, kw
    assert step(lib, frappe, Lg=1, kind=BPR) == BAD
    # then BPR by name, ahead of the served domain and of the pointers
    assert step(lib, frappe, kind=BPR) == UNS and step(lib, frappe, kind=BPR, G=65) == UNS
    assert step(lib, frappe, kind=BPR, U=0, **every_null) == UNS
    # then the served domain (cffm_list_step_ok), ahead of the pointers
    assert hip.load().cffm_list_step_ok(C.addressof(frappe), 256) == 1 and hip.load().cffm_list_step_ok(C.addressof(frappe), 260) == 0
    assert step(lib, frappe, G=65) == UNS and step(lib, frappe, G=65, U=0, **every_null) == UNS
    assert step(lib, frappe, G=2 ** 30, Lg=4) == UNS                                              # G * Lg beyond int32
    for kw in (dict(F=12), dict(optimizer='AdamOptimizer'), dict(loss_type='log_loss'), dict(lamda_bilinear=0.01)):
        other = shape_of(**kw)
        assert step(lib, other) == UNS and step(lib, other, **every_null) == UNS, kw
    # then the NULL checks of cffm_train_step_lists, ahead of the three new operands
    for name in STEP_PTRS:
        assert step(lib, frappe, **{name: 0}) == BAD, name
        assert step(lib, frappe, U=0, lists=0, corr=0, **{name: 0}) == BAD, name
    # then U < 1, a NULL lists, a NULL corr, a corr that is not 8-byte aligned: nothing else was read (theta, ws, ... are poison)
    for kw in (dict(U=0), dict(U=-1), dict(U=-(2 ** 31)), dict(lists=0), dict(corr=0), dict(lists=0, corr=0), dict(corr=P + 4)):
        assert step(lib, frappe, **kw) == BAD, kw
    # the uncorrected entry point keeps its refusals: BPR passes its kind check and reaches the NULL check
    args = [C.addressof(frappe)] + [P] * 6 + [4, P, 2, P, 8, 4, P, BPR] + [P] * 5 + [0, 0]
    assert lib.cffm_train_step_lists(*args) == BAD
