"""tests/_b3_exact.py on the CPU: every exact case of tests/test_gpu_b3_exact.py splits into its designed pieces, satisfies the
order-independent exactness condition, and has an identically zero dropped bracket - so its integer reference is what ANY correct
bf16x3 (or fp32) kernel returns bit for bit; and the walking layout reaches every slot it is there for."""
import numpy as np
import pytest

from tests import _b3_exact as bx
from tests.test_layer_check import _split

GEOS, CASES = bx.GEOS, bx.CASES


def split(x):
    return _split(np.asarray(x, dtype=np.float32), True)


def _designed(val, n):
    """The pieces a value with n populated pieces was built from: m, m 2^-9, m 2^-18."""
    m = np.rint(np.asarray(val, dtype=np.float64))
    return [m, m * 2.0 ** -9 * (n >= 2), m * 2.0 ** -18 * (n >= 3)]


@pytest.mark.parametrize('kind', ['fwd', 'dgrad', 'wgrad'])
@pytest.mark.parametrize('geo,cls,act', CASES, ids=['%s-%s' % (c[0], c[1]) for c in CASES])
def test_case_is_exact(geo, cls, act, kind):
    g = bx.Geo(*GEOS[geo])
    case = bx.build(g, cls, kind, act)
    # (a) the float32 replay of split_bf16x3 returns the designed pieces (selu: the split of a 24-bit value is only held to be exact)
    ops = [(case['a_act'], case.get('a_n'))] + [((case['b'][1] if kind == 'wgrad' else case['W']), case.get('b_n'))]
    for val, n in ops:
        p = split(val)
        assert np.array_equal(p[0] + p[1] + p[2], val.astype(np.float64))
        if act != 'selu':
            for got, want in zip(p, _designed(val, n)):
                assert np.array_equal(got, want)
            assert np.array_equal((p[1] != 0), (n >= 2) & (val != 0)) and np.array_equal((p[2] != 0), (n >= 3) & (val != 0))
    # (b) sum |kept terms| / lowest possible bit < 2^24 for every output; (c) the dropped bracket is identically zero
    kept, dropped, ratio = bx.exactness(g, case, split)
    assert float(ratio.max()) < 2.0 ** 24, float(ratio.max())
    assert not dropped.any()
    ref = bx.expected(g, case)
    full = ref['z'] if kind == 'fwd' else ref['gW'] if kind == 'wgrad' else None
    if full is not None:
        assert np.array_equal(kept, full)                       # the six kept products ARE the product of the values
        assert np.array_equal(full.astype(np.float32).astype(np.float64), full)
        assert np.count_nonzero(full) > 0.5 * full.size or kind == 'wgrad'
    if kind == 'wgrad':
        pb = split(case['b'][1])
        unit = min(float(bx.lowbit(p).min()) for p in pb)
        assert float(ref['gb_abs'].max()) / unit < 2.0 ** 24     # the bias gradient: a plain sum of dC[1], exact in any order
        assert np.count_nonzero(ref['gW']) > 1000 and np.count_nonzero(ref['gb']) > g.P // 2
    if kind == 'dgrad':
        assert np.array_equal(ref['dA'].astype(np.float32).astype(np.float64), ref['dA'])
        assert 0.05 < float((case['gate'] == 0).mean()) < 0.2


@pytest.mark.parametrize('cls', bx.LIMITED_CLASSES)
def test_full_weight_gradient_case_is_exact(cls):
    """The second weight-gradient data of the classes whose dC[1] has a third piece: every row populated.  The weight gradient meets
    the three conditions; the bias gradient of that run does not (and is not checked on the device)."""
    g = bx.Geo(*GEOS['f16-d32-b512'])
    case = bx.build(g, cls, 'wgrad', full=True)
    assert (case['b'][1][:, 0] != 0).all()
    for val, n in ((case['a_act'], case['a_n']), (case['b'][1], case['b_n'])):
        for got, want in zip(split(val), _designed(val, n)):
            assert np.array_equal(got, want)
    kept, dropped, ratio = bx.exactness(g, case, split)
    assert float(ratio.max()) < 2.0 ** 24 and not dropped.any()
    ref = bx.expected(g, case)
    assert np.array_equal(kept, ref['gW']) and np.array_equal(ref['gW'].astype(np.float32).astype(np.float64), ref['gW'])
    assert float(ref['gb_abs'].max()) / 2.0 ** -18 >= 2.0 ** 24            # why the first data set populates few rows


def test_piece_products_of_each_class():
    """Which of the nine piece products a class populates (forward, F16): exactly the ones its name says, all six kept ones in
    'six', never a dropped one."""
    g = bx.Geo(*GEOS['f16-d32-b512'])
    want = {'a1b1': {(0, 0)}, 'a2b1': {(0, 0), (1, 0)}, 'a1b2': {(0, 0), (0, 1)}, 'a2b2': {(0, 0), (1, 0), (0, 1), (1, 1)},
            'a3b1': {(0, 0), (1, 0), (2, 0)}, 'a1b3': {(0, 0), (0, 1), (0, 2)}, 'six': set(bx.TERMS6)}
    for cls in bx.CLASSES:
        case = bx.build(g, cls, 'fwd')
        pa, pb = split(case['a_act']), split(case['W'])
        idx = case['a'][0]
        live = {(i, j) for i in range(3) for j in range(3) if (pa[i][:, :, None] * pb[j][idx]).any()}
        assert live == want[cls], (cls, live)


@pytest.mark.parametrize('geo', sorted(GEOS))
def test_walking_layout_reaches_every_slot(geo):
    g = bx.Geo(*GEOS[geo])
    idx, val, _ = bx.rows_a(g, 'six')
    assert (val != 0).all()
    # forward: every reduction index - the channel next to the pad of every tap, every (k-step, half, lane group, k) slot of the padded
    # K = 4 Pp among them - in the first and second nonzero alike, and in rows of the first and of the last 128-row tile
    for t in range(2):
        assert np.array_equal(np.unique(idx[:, t]), np.arange(g.KV))
    k = (idx // g.P) * g.Pp + idx % g.P
    nks = (4 * g.Pp + 31) // 32
    assert np.array_equal(np.unique(k // 32), np.arange(nks)) and np.array_equal(np.unique(k[:, 0] % 32), np.arange(32))
    assert {g.P - 1, 2 * g.P - 1, 3 * g.P - 1, 4 * g.P - 1} <= set(idx[:, 0].tolist())
    W, _ = bx.filter_w(g, 'six', 'kv')
    assert np.unique(W, axis=0).shape[0] == g.KV and np.unique(W.T, axis=0).shape[0] == g.P      # a wrong slot is a different record
    # input gradient: every q, the last channel, and (F22: Pp / 16 = 15) the odd last k-step, whose second half is padding
    qi, qv, _ = bx.rows_g(g, 'six', 0, 'q')
    assert np.array_equal(np.unique(qi), np.arange(g.P)) and (qv != 0).all()
    if geo == 'f22-d32-b512':
        assert (g.Pp // 16) % 2 == 1 and (qi >= 32 * ((g.Pp // 16) // 2)).any()
    # weight gradient: the populated rows cover every position of a 32-row step, the first and the last step, and every column
    for limited in (False, True):
        bi, bv, _ = bx.rows_g(g, 'six', 1, 'm', limited=limited)
        rows = np.nonzero(bv[:, 0])[0]
        assert np.array_equal(np.unique(rows % 32), np.arange(32)) and rows[0] < 32 and rows[-1] >= g.rows - 32
        assert np.array_equal(np.unique(bi[rows, 0]), np.arange(g.P))
        assert np.unique(rows // 32).size >= (g.rows // 32 if not limited else 1000)


def test_device_layouts_round_trip():
    g = bx.Geo(5, 8, 3)
    rows = np.random.default_rng(0).standard_normal((g.rows, g.KV)).astype(np.float32)
    c0 = bx.to_c0(g, rows)
    assert c0.shape == (g.B, g.Sin, g.Sin, g.Pp) and not c0[..., g.P:].any()
    assert np.array_equal(bx.from_c0(g, c0), rows)
    # row m = (b, y, x), kv = (2 dy + dx) P + p  <->  C[0][b, 2 y + dy, 2 x + dx, p]
    m, kv = 7, 2 * g.P + 3
    b, y, x = m // (g.So * g.So), (m // g.So) % g.So, m % g.So
    assert c0[b, 2 * y + 1, 2 * x + 0, 3] == rows[m, kv]
    W = np.arange(g.KV * g.P, dtype=np.float32).reshape(g.KV, g.P)
    assert bx.to_theta_w(g, W)[2, 3, 4] == W[2 * g.P + 3, 4]
