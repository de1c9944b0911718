"""cffm_list_loss_logq on the device against its float64 twin (cffm_amd.spec.list_loss_logq, itself checked in
tests/test_list_logq_ref.py), by the criterion tests/test_gpu_list_loss.py applies to the uncorrected kernel: lists on both sides of
the 64-lane stride and of the register-kept first stride, one list, a full and a ragged workgroup and many; tables of 2, 66 and 4096
rows with corrections of both signs up to |c| ~ 20; repeated indices; targets first, last and out of range; an index at -1 and one
at U; a -inf correction.  The outputs are written inside poisoned buffers between canaries; an all-zero table gives the bits of
cffm_list_loss; the bits do not depend on the run or on what scratch held."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cffm_amd import hip, spec  # noqa: E402
from oracle.parity import close  # noqa: E402
from tests import _list_logq_ref as Q  # noqa: E402
from tests.test_gpu_list_loss import PAD, POISON, run as run_plain  # noqa: E402

pytestmark = pytest.mark.gpu
assert 'cffm_list_loss_logq' in hip.PROTOTYPES            # the entry point this file is about

GS, LGS, US = (1, 4, 5, 67), (2, 63, 64, 65, 130), (2, 66, 4096)


def run(s, t, lists, corr, scratch_fill=None):
    """-> (loss [1], dout [G, Lg], terms [G]) as numpy, each cut out of a poisoned buffer whose canaries are checked; the inputs
    come back unchanged."""
    lib = hip.fast()
    G, Lg = s.shape
    U = corr.shape[0]
    dev = torch.device('cuda')
    sd, td, ld, cd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (s, t, lists, corr))
    assert cd.data_ptr() % 8 == 0
    bufs = {n: torch.full((PAD + size + PAD,), POISON, dtype=torch.float32, device=dev) for n, size in (('dout', G * Lg), ('terms', G), ('loss', 1))}
    nbytes = int(lib.cffm_list_loss_scratch_bytes(G))
    scratch = torch.zeros(nbytes + 64, dtype=torch.uint8, device=dev)
    if scratch_fill is not None:
        scratch.view(torch.float32).fill_(scratch_fill)
    scratch[nbytes:] = 0xA5
    ptr = lambda n: bufs[n].data_ptr() + 4 * PAD
    hip.check(lib.cffm_list_loss_logq(hip.LIST_LOSS_IDS['softmax'], sd.data_ptr(), G, Lg, td.data_ptr(), ld.data_ptr(), cd.data_ptr(), U,
                                      ptr('dout'), ptr('terms'), ptr('loss'), scratch.data_ptr(),
                                      int(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    out = {}
    for n, b in bufs.items():
        h = b.cpu().numpy()
        assert (h[:PAD] == np.float32(POISON)).all() and (h[-PAD:] == np.float32(POISON)).all(), '%s: written outside its range' % n
        out[n] = h[PAD:-PAD].copy()
    assert bool((scratch[nbytes:] == 0xA5).all()), 'scratch: written beyond cffm_list_loss_scratch_bytes'
    for a, d in ((s, sd), (t, td), (lists, ld), (corr, cd)):
        assert d.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()
    return out['loss'], out['dout'].reshape(G, Lg), out['terms']


def held(got, ref, with_nan):
    """The criterion of tests/test_gpu_list_loss.py::test_list_loss_against_the_reference."""
    loss, dout, terms = got
    ref_loss, ref_dout, ref_terms = ref
    assert np.array_equal(np.isnan(dout), np.isnan(ref_dout)) and np.array_equal(np.isnan(terms), np.isnan(ref_terms))
    assert np.isnan(ref_loss) == with_nan == bool(np.isnan(loss[0]))
    ok = ~np.isnan(ref_terms)
    assert np.isfinite(dout[ok]).all() and np.isfinite(terms[ok]).all()
    close(dout[ok], ref_dout[ok], 'list_loss_logq dout')
    close(terms[ok], ref_terms[ok], 'list_loss_logq terms')
    if not with_nan:
        close(loss, np.array([ref_loss]), 'list_loss_logq loss')
    rows = np.abs(dout[ok].astype(np.float64).sum(axis=1))
    assert (rows <= 1e-5 * np.abs(dout[ok]).astype(np.float64).sum(axis=1) + 1e-30).all()


@pytest.mark.parametrize('U', US)
@pytest.mark.parametrize('Lg', LGS)
@pytest.mark.parametrize('G', GS)
def test_against_the_twin(G, Lg, U):
    s, t, lists, corr = Q.make_inputs(G, Lg, U)
    c = corr[lists, 0].astype(np.float64) - corr[lists[np.arange(G), t], 1].astype(np.float64)[:, None]
    assert np.abs(c).max() <= 20.0 and (U == 2 and G < 4 or np.abs(c).max() > 10.0) and (G * Lg < 8 or (c > 0).any() and (c < 0).any())
    held(run(s, t, lists, corr), spec.list_loss_logq(s, t, lists, corr), False)


@pytest.mark.parametrize('G,Lg,U', [(5, 2, 2), (5, 64, 66), (67, 65, 4096), (4, 130, 66), (67, 63, 2)])
def test_edge_lists(G, Lg, U):
    s, t, lists, corr = Q.make_inputs(G, Lg, U)
    clean = run(s, t, lists, corr)
    t2, l2 = t.copy(), lists.copy()
    t2[0], l2[0, 0] = Lg, -7                              # target out of range: nothing of the list is looked at, a bad index included
    t2[1] = -1 if G < 67 else -(2 ** 31)
    s2 = s.copy()
    s2[1, :] = 3.0e38
    l2[2, Lg - 1] = -1                                    # one index at -1 and one at U in otherwise valid lists
    l2[3, 0] = U
    got = run(s2, t2, l2, corr)
    assert not got[1][:4].any() and not got[2][:4].any()                        # exact zeros: rows and terms
    ref = spec.list_loss_logq(s2, t2, l2, corr)
    held(got, ref, False)
    if G > 4:                                              # the neighbours are what they were, bit for bit (dout carries the same 1 / G)
        assert np.array_equal(got[1][4:].view(np.uint32), clean[1][4:].view(np.uint32))
        assert np.array_equal(got[2][4:].view(np.uint32), clean[2][4:].view(np.uint32))
    if G > 4:
        # a -inf correction on a negative of the last list: that list is NaN, the others unaffected
        g = G - 1
        n = 0 if t[g] != 0 else 1
        j = int(lists[g, n])
        hit = (lists == j).any(axis=1)
        if lists[g, t[g]] != j and hit.sum() < G:
            c2 = corr.copy()
            c2[j, 0] = -np.inf
            got = run(s, t, lists, c2)
            ref = spec.list_loss_logq(s, t, lists, c2)
            assert np.isnan(got[2][g]) and np.isnan(got[1][g]).all()
            held(got, ref, True)
            assert np.array_equal(got[1][~hit].view(np.uint32), clean[1][~hit].view(np.uint32))
            assert np.array_equal(got[2][~hit].view(np.uint32), clean[2][~hit].view(np.uint32))
        else:
            assert U == 2                                  # two table rows: every list holds both


@pytest.mark.parametrize('G,Lg,U', [(1, 2, 2), (5, 63, 66), (4, 64, 2), (67, 65, 4096), (5, 130, 66)])
def test_an_all_zero_table_gives_the_bits_of_cffm_list_loss(G, Lg, U):
    s, t, lists, _ = Q.make_inputs(G, Lg, U)
    if G >= 5:
        t[4] = Lg                                          # and the zero row of an invalid target
    got = run(s, t, lists, np.zeros((U, 2), dtype=np.float32))
    want = run_plain('softmax', s, t)
    for a, b, name in zip(got, want, ('loss', 'dout', 'terms')):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


@pytest.mark.parametrize('G,Lg,U', [(5, 64, 66), (67, 65, 4096), (4, 130, 2)])
def test_same_bits_on_every_call_and_on_a_dirty_scratch(G, Lg, U):
    s, t, lists, corr = Q.make_inputs(G, Lg, U)
    first = run(s, t, lists, corr)
    for fill in (None, float('nan'), 3.39e38):
        again = run(s, t, lists, corr, scratch_fill=fill)
        for a, b, name in zip(again, first, ('loss', 'dout', 'terms')):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, fill)
