"""cffm_pick_hard: what it returns before any device work, through both bindings.  Every refusal include/cffm_hip.h lists comes back
ahead of the launch, so the device pointers here are NULL or a poison address that is never read - a case that got any further
would fault on them - and no GPU is needed."""
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
    name = 'cffm_pick_hard'
    assert name in hip.PROTOTYPES and hasattr(hip.load(), name) and hasattr(hip.fast(), name)
    assert len(hip.PROTOTYPES[name][1]) == 15
    assert hip.load().cffm_abi_version() == hip.fast().cffm_abi_version() == hip.ABI_VERSION == 9      # additive: the version stays
    header = open(os.path.join(ROOT, 'include', 'cffm_hip.h')).read()
    weighted = header.index('weighted ranked lists drawn on the device')
    start = header.index('hard negatives picked from a scored pool')
    assert weighted < header.index('int cffm_draw_lists_weighted(') < start < header.index('peak probes')  # a section of its own, in place
    section = header[start:]
    assert 'Additive entry points: CFFM_ABI_VERSION stays 9' in section[:section.index('int cffm_pick_hard(')]
    assert section.index('int cffm_pick_hard(') < section.index('/* ----')                              # declared inside its section
    assert '#define CFFM_ABI_VERSION 9' in header
    src = open(os.path.join(ROOT, 'cffm_amd', 'csrc_host', 'pybind_module.cpp')).read()
    assert 'CFFM_BIND(cffm_pick_hard);' in src
    assert spec.HARD_TAG == 4 and spec.HARD_MAX_LP == 1024
    # the key has one definition, shared by the two translation units
    csrc = os.path.join(ROOT, 'cffm_amd', 'csrc')
    assert open(os.path.join(csrc, 'rank_key.hpp')).read().count('rank_key64(unsigned u, unsigned pos)') == 1
    for unit in ('rank.hip', 'hard.hip'):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "rank_key.hpp"' in text and 'rank_key64(unsigned u' not in text


def pick(lib, seed=7, list0=0, G=4, scores=P, row_stride=9, Lp=9, target_pool=P, m=3, pool_lists=P, pool_tuples=P, nf=2, lists=P,
         tuples=P, target=P):
    return lib.cffm_pick_hard(seed, list0, G, scores, row_stride, Lp, target_pool, m, pool_lists, pool_tuples, nf, lists, tuples, target, 0)


def test_refusals(lib):
    null = dict(scores=0, target_pool=0, pool_lists=0, pool_tuples=0, lists=0, tuples=0, target=0)
    i64 = 2 ** 63 - 1
    for kw in (dict(Lp=1, row_stride=1, m=1), dict(Lp=0, m=1), dict(Lp=-3, m=1), dict(Lp=-(2 ** 31), m=1),           # Lp < 2
               dict(Lp=1025, row_stride=1025), dict(Lp=2 ** 31 - 1, row_stride=2 ** 31, m=5),                       # Lp > 1024
               dict(m=0), dict(m=-1), dict(m=-(2 ** 31)),                                                           # m < 1
               dict(m=9), dict(m=10), dict(Lp=2, row_stride=2, m=2), dict(Lp=1024, row_stride=1024, m=1024),        # m > Lp - 1
               dict(m=2 ** 31 - 1),
               dict(G=-1), dict(G=-(2 ** 31)),
               dict(list0=-1), dict(list0=-(2 ** 63)),
               dict(list0=i64), dict(list0=i64 - 3), dict(list0=i64 - 2 ** 20, G=2 ** 20 + 1, nf=1),                # list0 + G overflows
               dict(row_stride=8), dict(row_stride=0), dict(row_stride=-9), dict(row_stride=-(2 ** 63)),            # row_stride < Lp
               dict(Lp=1024, row_stride=1023),
               dict(G=2 ** 28, nf=1), dict(G=2 ** 21, Lp=1024, row_stride=1024, nf=1), dict(G=2 ** 20, nf=512),     # G Lp max(nf, 1) >= 2^31
               dict(G=1, Lp=2, row_stride=2, m=1, nf=2 ** 30), dict(G=2 ** 31 - 1, Lp=1024, row_stride=1024, nf=2 ** 31 - 1),
               dict(nf=-1), dict(nf=-(2 ** 31))):
        assert pick(lib, **kw) == BAD, kw
        assert pick(lib, **dict(null, **kw)) == BAD, kw                                  # with every pointer NULL: nothing was read
        assert pick(lib, **dict(kw, pool_tuples=0, tuples=0)) == BAD, kw                 # the indices-only mode refuses them too
        assert pick(lib, **dict(kw, pool_lists=0, lists=0)) == BAD, kw                   # and the tuples-only mode
    # the size bound counts max(nf, 1) in the indices-only mode as well
    assert pick(lib, G=2 ** 28, pool_tuples=0, tuples=0, nf=0) == BAD
    # nf == 0 with a pool or a tuple output; exactly one of a pair; no output at all; a NULL scores, target_pool or target_out
    for kw in (dict(nf=0), dict(nf=0, pool_tuples=0), dict(nf=0, tuples=0),
               dict(pool_tuples=0), dict(tuples=0), dict(pool_tuples=0, lists=0, pool_lists=0), dict(tuples=0, lists=0, pool_lists=0),
               dict(pool_lists=0), dict(lists=0), dict(pool_lists=0, tuples=0, pool_tuples=0), dict(lists=0, tuples=0, pool_tuples=0),
               dict(pool_tuples=0, tuples=0, pool_lists=0, lists=0), dict(pool_tuples=0, tuples=0, pool_lists=0, lists=0, nf=0),
               dict(tuples=0, lists=0), dict(pool_lists=0, pool_tuples=0),
               dict(scores=0), dict(target_pool=0), dict(target=0),
               dict(scores=0, pool_tuples=0, tuples=0), dict(target_pool=0, pool_lists=0, lists=0), dict(target=0, pool_tuples=0, tuples=0)):
        assert pick(lib, **kw) == BAD, kw
        assert pick(lib, **dict(kw, G=0)) == BAD, kw                                     # checked ahead of the empty call
    # the largest accepted sizes: only a NULL pointer refuses them
    assert pick(lib, list0=i64 - 4, scores=0) == BAD and pick(lib, G=2 ** 27 - 1, Lp=8, row_stride=8, nf=2, target=0) == BAD
    assert pick(lib, Lp=1024, row_stride=2 ** 62, m=1023, G=1, target_pool=0) == BAD and pick(lib, Lp=2, row_stride=2, m=1, G=1, scores=0) == BAD


def test_an_empty_call_returns_zero_without_a_launch(lib):
    assert pick(lib, G=0) == 0                                                           # every output combination
    assert pick(lib, G=0, pool_tuples=0, tuples=0) == 0 and pick(lib, G=0, pool_tuples=0, tuples=0, nf=0) == 0
    assert pick(lib, G=0, pool_lists=0, lists=0) == 0
    assert pick(lib, G=0, list0=2 ** 63 - 1, Lp=1024, row_stride=1024, m=1023) == 0
    assert pick(lib, G=0, seed=2 ** 64 - 1) == 0 and pick(lib, G=0, Lp=2, row_stride=2 ** 40, m=1) == 0
