"""cffm_draw_lists_weighted: what it returns before any device work, through both bindings.  Every refusal include/cffm_hip.h lists
comes back ahead of the launch, so the device pointers here are NULL or a poison address that is never read - a case that got any
further would fault on them - and no GPU is needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cffm_amd import hip, spec  # noqa: E402

BAD, P = 10001, 0x1000            # P: a non-NULL address nobody may read


@pytest.fixture(scope='module', params=['ctypes', 'pybind11'])
def lib(request):
    hip.load()
    if request.param == 'ctypes':
        return hip.load()
    assert hip.binding_name() == 'pybind11', 'cffm_amd/lib/_cffm_pybind*.so is not built (make)'
    return hip.fast()


def test_the_entry_point_is_declared_in_both_bindings():
    name = 'cffm_draw_lists_weighted'
    assert name in hip.PROTOTYPES and hasattr(hip.load(), name) and hasattr(hip.fast(), name)
    assert len(hip.PROTOTYPES[name][1]) == 13
    assert hip.load().cffm_abi_version() == hip.fast().cffm_abi_version() == hip.ABI_VERSION == 9      # additive: the version stays
    header = open(os.path.join(ROOT, 'include', 'cffm_hip.h')).read()
    uniform = header.index('ranked lists drawn on the device')
    start = header.index('weighted ranked lists drawn on the device')
    assert uniform < header.index('int cffm_draw_lists(') < start < header.index('peak probes')         # a section of its own, in place
    section = header[start:]
    assert 'Additive entry points: CFFM_ABI_VERSION stays 9' in section[:section.index('int cffm_draw_lists_weighted(')]
    assert section.index('int cffm_draw_lists_weighted(') < section.index('/* ----')                    # declared inside its section
    assert '#define CFFM_ABI_VERSION 9' in header
    src = open(os.path.join(ROOT, 'cffm_amd', 'csrc_host', 'pybind_module.cpp')).read()
    assert 'CFFM_BIND(cffm_draw_lists_weighted);' in src
    assert spec.DRAW_W_TAG == 3 and spec.draw_weighted_cap(3) == 1024 and spec.draw_weighted_cap(99) == 1536


def draw(lib, seed=7, list0=0, G=4, at=P, U=10, m=3, cdf=P, cand=P, nf=2, lists=P, tuples=P, target=P):
    return lib.cffm_draw_lists_weighted(seed, list0, G, at, U, m, cdf, cand, nf, lists, tuples, target, 0)


def test_refusals(lib):
    null = dict(at=0, cdf=0, cand=0, lists=0, tuples=0, target=0)
    i64 = 2 ** 63 - 1
    for kw in (dict(U=0, m=1), dict(U=-5, m=1), dict(U=-(2 ** 31), m=1),                 # U < 1
               dict(m=0), dict(m=-1), dict(U=1, m=0),                                    # m < 1
               dict(U=1, m=1), dict(m=10), dict(U=2, m=2), dict(U=1024, m=1024),         # m > U - 1: U = 1 serves no list
               dict(U=5000, m=1024), dict(U=2 ** 31 - 1, m=2 ** 31 - 2),                 # m > 1023
               dict(G=-1), dict(G=-(2 ** 31)),
               dict(list0=-1), dict(list0=-(2 ** 63)),
               dict(list0=i64), dict(list0=i64 - 3), dict(list0=i64 - 2 ** 20, G=2 ** 20 + 1, nf=1),      # list0 + G overflows
               dict(G=2 ** 29, nf=1), dict(G=2 ** 21, U=5000, m=1023, nf=1), dict(G=2 ** 20, m=3, nf=512), dict(G=1, m=1, nf=2 ** 30),
               dict(nf=-1), dict(nf=-(2 ** 31))):
        assert draw(lib, **kw) == BAD, kw
        assert draw(lib, **dict(null, **kw)) == BAD, kw                                  # with every pointer NULL: nothing was read
        assert draw(lib, **dict(kw, cand=0, tuples=0)) == BAD, kw                        # the indices-only mode refuses them too
    # the size bound counts max(nf, 1) in the indices-only mode as well
    assert draw(lib, G=2 ** 29, cand=0, tuples=0, nf=0) == BAD
    # nf == 0 with a table or a tuple output; exactly one of the two; no output at all; a NULL at, target_out or cdf
    for kw in (dict(nf=0), dict(nf=0, cand=0), dict(nf=0, tuples=0),
               dict(cand=0), dict(tuples=0), dict(cand=0, lists=0), dict(tuples=0, lists=0),
               dict(cand=0, tuples=0, lists=0), dict(cand=0, tuples=0, lists=0, nf=0),
               dict(at=0), dict(target=0), dict(cdf=0), dict(at=0, cand=0, tuples=0), dict(target=0, cand=0, tuples=0),
               dict(cdf=0, cand=0, tuples=0), dict(cdf=0, lists=0)):
        assert draw(lib, **kw) == BAD, kw
        assert draw(lib, **dict(kw, G=0)) == BAD, kw                                     # checked ahead of the empty call
    # the largest accepted sizes: only a NULL pointer refuses them
    assert draw(lib, list0=i64 - 4, cdf=0) == BAD and draw(lib, G=2 ** 28 - 1, m=3, nf=2, target=0) == BAD
    assert draw(lib, U=2 ** 31 - 1, m=1023, G=1, cdf=0) == BAD and draw(lib, U=2, m=1, G=1, at=0) == BAD


def test_an_empty_call_returns_zero_without_a_launch(lib):
    assert draw(lib, G=0) == 0                                                           # both modes, every output combination
    assert draw(lib, G=0, cand=0, tuples=0) == 0 and draw(lib, G=0, cand=0, tuples=0, nf=0) == 0
    assert draw(lib, G=0, lists=0) == 0
    assert draw(lib, G=0, list0=2 ** 63 - 1, U=2 ** 31 - 1, m=1023) == 0
    assert draw(lib, G=0, seed=2 ** 64 - 1) == 0 and draw(lib, G=0, U=2, m=1) == 0
