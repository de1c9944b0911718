"""tests/_list_loss_ref.py, the float64 reading of cffm_list_loss the GPU tests compare against, is itself checked here: against
torch's float64 autograd of logsigmoid / log_softmax, and by planting four mistakes that oracle.parity.close must catch on the
same inputs - so a device kernel with one of them would not pass tests/test_gpu_list_loss.py."""
import numpy as np
import pytest
import torch

from cffm_amd import hip
from oracle.parity import close
from tests import _list_loss_ref as LR

G = 6
KINDS = sorted(hip.LIST_LOSS_IDS)          # the kinds the library knows: the reference reads exactly those
assert KINDS == sorted(LR.KINDS)


def _inputs(Lg, where, seed=0, big=False):
    rng = np.random.default_rng(seed + Lg)
    s = rng.standard_normal((G, Lg)) * 1.5
    t = {'first': 0, 'last': Lg - 1, 'middle': Lg // 2}[where]
    if big:                                                    # scores at +-80: the positive at -80 with a negative at +80 next to it
        s[:, ::2] += 80.0
        s[:, 1::2] -= 80.0
        s[:, t] = -80.0 + rng.standard_normal(G)
        s[:, (t + 1) % Lg] = 80.0 + rng.standard_normal(G)
    return s, np.full(G, t, dtype=np.int32)


def _torch_loss(kind, s, target):
    st = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(target, dtype=torch.long)
    if kind == 'bpr':
        pos = st.gather(1, tt[:, None])
        keep = torch.ones_like(st, dtype=torch.bool).scatter(1, tt[:, None], False)
        terms = -(torch.nn.functional.logsigmoid(pos - st) * keep).sum(dim=1) / (st.shape[1] - 1)
    else:
        terms = -torch.log_softmax(st, dim=1).gather(1, tt[:, None])[:, 0]
    loss = terms.mean()
    loss.backward()
    return float(loss.detach()), st.grad.numpy(), terms.detach().numpy()


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(float(np.abs(b).max()), 1e-300))


@pytest.mark.parametrize('big', [False, True])
@pytest.mark.parametrize('where', ['first', 'last', 'middle'])
@pytest.mark.parametrize('Lg', [2, 5, 65])
@pytest.mark.parametrize('kind', KINDS)
def test_reference_agrees_with_torch_float64_autograd(kind, Lg, where, big):
    s, t = _inputs(Lg, where, big=big)
    loss, dout, terms = LR.list_loss_ref(kind, s, t)
    tl, td, tt = _torch_loss(kind, s, t)
    assert abs(loss - tl) <= 1e-12 * abs(tl)
    assert _rel(terms, tt) <= 1e-12 and _rel(dout, td) <= 1e-12
    assert np.isfinite(dout).all() and np.isfinite(terms).all()


def _missed(got, ref):
    """True when close() refuses at least one of (dout, terms, loss) of `got` against `ref`."""
    for a, b, name in zip(got[::-1], ref[::-1], ('terms', 'dout', 'loss')):
        try:
            close(np.atleast_1d(a), np.atleast_1d(b), 'planted ' + name)
        except AssertionError:
            return True
    return False


@pytest.mark.parametrize('where', ['first', 'last', 'middle'])
@pytest.mark.parametrize('Lg', [2, 5, 65])
@pytest.mark.parametrize('kind', KINDS)
def test_planted_faults_miss_the_criterion(kind, Lg, where):
    s, t = _inputs(Lg, where)
    ref = LR.list_loss_ref(kind, s, t)
    assert not _missed(ref, ref)
    assert _missed(LR.list_loss_ref(kind, s, t, fault='sign'), ref)                 # the sign of dout[t]
    if kind == 'bpr' and Lg > 2:                                                     # G instead of G m (m = 1 at Lg = 2: the same number)
        assert _missed(LR.list_loss_ref(kind, s, t, fault='normaliser'), ref)
    if where != 'first':                                                             # the target fixed at 0
        assert _missed(LR.list_loss_ref(kind, s, t, fault='target0'), ref)
    # the exponentials taken of the raw argument, as float32 would: at scores of +-80 the BPR differences reach 160 and
    # log(1 + exp(x)) is inf.  exp(+-80) itself is finite in float32 (5.5e34), so the softmax without its maximum is still RIGHT
    # at +-80 - the reference says so - and is shown to be caught where it first goes wrong, at +-90.
    sb, tb = _inputs(Lg, where, big=True)
    refb = LR.list_loss_ref(kind, sb, tb)
    if kind == 'bpr':
        assert _missed(LR.list_loss_ref(kind, sb, tb, fault='no_max'), refb)
    else:
        assert not _missed(LR.list_loss_ref(kind, sb, tb, fault='no_max'), refb)
        s90 = sb * (90.0 / 80.0)
        assert _missed(LR.list_loss_ref(kind, s90, tb, fault='no_max'), LR.list_loss_ref(kind, s90, tb))


def test_nan_and_out_of_range_targets():
    s, t = _inputs(5, 'middle')
    s[1, 3] = np.nan
    t[4] = 5
    t[5] = -1
    for kind in KINDS:
        loss, dout, terms = LR.list_loss_ref(kind, s, t)
        assert np.isnan(loss) and np.isnan(terms[1]) and np.isnan(dout[1]).all()
        assert (terms[4:] == 0).all() and (dout[4:] == 0).all()
        assert np.isfinite(dout[[0, 2, 3]]).all() and np.isfinite(terms[[0, 2, 3]]).all()
