"""cffm_list_loss on the device against its float64 reading (tests/_list_loss_ref.py, itself checked in tests/test_list_loss_ref.py):
both kinds, lists shorter than, equal to and one longer than a wavefront, more lists than one workgroup holds and a ragged last
workgroup; targets first, last and in the middle; ties, all-equal lists, scores at +-80, a NaN list and a target out of range.  The
outputs are written inside poisoned buffers between canaries, and the bits do not depend on the run or on what scratch held."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cffm_amd import hip  # noqa: E402
from oracle.parity import close  # noqa: E402
from tests import _list_loss_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2), (7, 5), (3, 64), (3, 65), (300, 101)]
POISON, PAD = 7.25e33, 96


def make_inputs(G, Lg, with_nan, seed=0):
    rng = np.random.default_rng(seed + 1000 * G + Lg)
    s = (rng.standard_normal((G, Lg)) * 2.0).astype(np.float32)
    t = np.array([(0, Lg - 1, Lg // 2)[g % 3] for g in range(G)], dtype=np.int32)           # first, last, middle
    if G >= 3:
        s[1, :] = s[1, 0]                                                   # an all-equal list
        s[2, 1:] = np.where(np.arange(1, Lg) % 2 == 0, 80.0, -80.0)         # scores at +-80 ...
        s[2, t[2]] = -80.0                                                  # ... the positive among the low ones: differences of 160
    if G >= 7:
        s[3, Lg // 2:] = s[3, 0]                                            # ties with the positive (target 0) and among the negatives
        s[4, :] = np.round(s[4, :])                                         # ties among small integers
        t[5] = Lg                                                           # out of range: a zero row, a zero term
        t[6] = -1 if G == 7 else -(2 ** 31)
        s[6, :] = 3.0e38                                                    # and its scores are never looked at
    if with_nan:
        s[0, (Lg - 1) // 2] = np.nan                                       # one NaN score: its list's term and row are NaN, and the loss
    return s, t


def run(kind, s, t, scratch_fill=None):
    """-> (loss [1], dout [G, Lg], terms [G]) as numpy, each cut out of a poisoned buffer whose canaries are checked."""
    lib = hip.fast()
    G, Lg = s.shape
    dev = torch.device('cuda')
    sd, td = torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev)
    bufs = {n: torch.full((PAD + size + PAD,), POISON, dtype=torch.float32, device=dev) for n, size in (('dout', G * Lg), ('terms', G), ('loss', 1))}
    nbytes = int(lib.cffm_list_loss_scratch_bytes(G))
    assert nbytes >= 8 * ((G + 3) // 4)
    scratch = torch.zeros(nbytes + 64, dtype=torch.uint8, device=dev)
    if scratch_fill is not None:
        scratch.fill_(scratch_fill)
    scratch[nbytes:] = 0xA5
    ptr = lambda n: bufs[n].data_ptr() + 4 * PAD
    hip.check(lib.cffm_list_loss(hip.LIST_LOSS_IDS[kind], sd.data_ptr(), G, Lg, td.data_ptr(), ptr('dout'), ptr('terms'), ptr('loss'),
                                 scratch.data_ptr(), int(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    out = {}
    for n, b in bufs.items():
        h = b.cpu().numpy()
        assert (h[:PAD] == np.float32(POISON)).all() and (h[-PAD:] == np.float32(POISON)).all(), '%s: written outside its range' % n
        out[n] = h[PAD:-PAD].copy()
    assert bool((scratch[nbytes:] == 0xA5).all()), 'scratch: written beyond cffm_list_loss_scratch_bytes'
    assert np.array_equal(sd.cpu().numpy().view(np.uint32), s.view(np.uint32)) and np.array_equal(td.cpu().numpy(), t)
    return out['loss'], out['dout'].reshape(G, Lg), out['terms']


@pytest.mark.parametrize('with_nan', [False, True])
@pytest.mark.parametrize('G,Lg', SHAPES)
@pytest.mark.parametrize('kind', LR.KINDS)
def test_list_loss_against_the_reference(kind, G, Lg, with_nan):
    s, t = make_inputs(G, Lg, with_nan)
    ref_loss, ref_dout, ref_terms = LR.list_loss_ref(kind, s, t)
    loss, dout, terms = run(kind, s, t)
    # NaN exactly where the reference has it: the NaN list's row and term (and the loss), nowhere else
    assert np.array_equal(np.isnan(dout), np.isnan(ref_dout)) and np.array_equal(np.isnan(terms), np.isnan(ref_terms))
    assert np.isnan(ref_loss) == with_nan == bool(np.isnan(loss[0]))
    ok = ~np.isnan(ref_terms)
    assert np.isfinite(dout[ok]).all() and np.isfinite(terms[ok]).all()
    close(dout[ok], ref_dout[ok], 'list_loss dout %s' % kind)
    close(terms[ok], ref_terms[ok], 'list_loss terms %s' % kind)
    if not with_nan:
        close(loss, np.array([ref_loss]), 'list_loss loss %s' % kind)
    # an out-of-range target: exact zeros, and the lists around it are the reference's (held above)
    out_of_range = (t < 0) | (t >= Lg)
    assert out_of_range.sum() == (2 if G >= 7 else 0)
    assert not dout[out_of_range].any() and not terms[out_of_range].any()
    # dout is a gradient of a mean over lists: every row sums to 0 to rounding
    rows = np.abs(dout[ok].astype(np.float64).sum(axis=1))
    assert (rows <= 1e-5 * np.abs(dout[ok]).astype(np.float64).sum(axis=1) + 1e-30).all()


@pytest.mark.parametrize('G,Lg', [(7, 5), (3, 65), (300, 101)])
@pytest.mark.parametrize('kind', LR.KINDS)
def test_same_bits_on_every_call_and_on_a_dirty_scratch(kind, G, Lg):
    s, t = make_inputs(G, Lg, False)
    first = run(kind, s, t)
    for fill in (None, 0xFF, 0x7F):                                       # 0xFF: NaN doubles, 0x7F: huge ones
        again = run(kind, s, t, scratch_fill=fill)
        for a, b, name in zip(again, first, ('loss', 'dout', 'terms')):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, fill)
