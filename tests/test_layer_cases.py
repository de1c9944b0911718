"""The case list of tests/test_gpu_layers.py, on the CPU: every case still selects the kernel instances it is there for ('want', asked
of cffm_conv_choice), stays below the file's workspace cap (cffm_ws_layout), and the large-row-count cases have the rows per layer
their comments state: the half-full 128-row tile, the odd count of 16-row tiles under two row groups, the partial 64-row block.
A case that a dispatch change has emptied, or whose comment is wrong, fails here without a GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cffm_amd import hip  # noqa: E402
from tests import test_gpu_layers as gl  # noqa: E402

# case -> {layer: rows}: the layers the case is there for
ROWS = {
    'f12-d16-b513-gelu': {0: 32832},
    'f16-d16-b513-relu': {0: 32832},
    'f2-d16-b513-elu': {0: 32832},
    'f11-d32-b65-selu': {0: 16640},
    'f7-d32-b256-relu': {1: 16384},
    'f7-d32-b509-gelu': {1: 32576},
    'f7-d32-b513-elu': {1: 32832},
    'f11-d16-b509-relu': {1: 8144},
    'f11-d32-b509-selu': {1: 32576},
    'f11-d32-b513-gelu': {1: 32832},
    'f2-d32-b509-elu': {1: 32576},
    'f10-d32-b509-selu': {1: 32576},
    'f7-d32-b1025-selu': {2: 16400, 3: 4100},
    'f7-d32-b2049-relu': {2: 32784, 3: 8196},
}
TAPS_RM2 = range(16 * 1024, 16 * 2048)          # rows at which the tap-split forward runs two row groups (conv_fwd_choice)
ROWS_MIN = 16 * 2048                            # ... and from which the narrow forward is conv_fwd_rows, the direct kernels RM = 2


def _lib():
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return hip.load()


def layer_rows(name, layer):
    c = gl.CASES[name]
    return c['B'] * (c['D'] >> (layer + 1)) ** 2


@pytest.mark.parametrize('name', list(gl.CASES))
def test_case_selects_its_instances(name):
    _lib()
    cfg = gl.case_config(name)
    gl.check_instances(name, cfg, gl.CASES[name]['B'])


def test_large_row_cases_name_their_layers():
    """Every case of ROWS asserts an instance on each layer it lists, with the ledger's b3 and paired, and the row counts are the stated
    ones and lie in the range that selects the family."""
    assert set(ROWS) <= set(gl.CASES)
    for name, per_layer in ROWS.items():
        want = gl.want_entries(name)
        assert want and all(extra is not None for _, _, _, extra in want), name
        assert {layer for layer, _, _, _ in want} == set(per_layer), name
        for layer, rows in per_layer.items():
            assert layer_rows(name, layer) == rows, (name, layer)
        for layer, role, (family, NT, RM, HALVES), _ in want:
            rows = per_layer[layer]
            if role == 'fwd' and family == gl.FWD_TAPS:
                assert (rows in TAPS_RM2) == (RM == 2) and rows < ROWS_MIN, (name, layer)
            if role == 'fwd' and family in (gl.FWD_ROWS, gl.FWD_DIRECT) and (family, RM) != (gl.FWD_DIRECT, 1):
                assert rows >= ROWS_MIN, (name, layer)
    # the activations: all four, and both ACTA builds of the direct kernels (selu / gelu against relu / elu) on the wide cases
    acts = {gl.CASES[n]['act'] for n in ROWS}
    assert acts == {'relu', 'elu', 'selu', 'gelu'}
    assert {gl.CASES[n]['act'] for n in ROWS if gl.CASES[n]['F'] >= 12} == {'gelu', 'relu'}
    frappe = gl.CASES['f10-d32-b509-selu']           # the product shape in its per-stage batch range 410 .. 511
    assert (frappe['F'], frappe['D'], frappe['act']) == (10, 32, 'selu') and 410 <= frappe['B'] <= 511


def test_ragged_ends_are_what_the_comments_claim():
    r = {n: ROWS[n] for n in ROWS}
    # direct layer 0, 128-row tiles: the last tile is half full
    for n in ('f12-d16-b513-gelu', 'f16-d16-b513-relu'):
        assert r[n][0] % 128 == 64
    # conv_fwd_rows, 64-row blocks: whole blocks where the case says nothing else ...
    for n, l in (('f2-d16-b513-elu', 0), ('f7-d32-b513-elu', 1), ('f11-d32-b513-gelu', 1)):
        assert r[n][l] % 64 == 0
    # ... and 16 rows in the last block of layer 2 at B = 2049, an odd count of 16-row tiles for the RM = 2 input gradient
    assert r['f7-d32-b2049-relu'][2] % 64 == 16 and r['f7-d32-b2049-relu'][2] // 16 % 2 == 1
    assert r['f7-d32-b2049-relu'][3] % 16 == 4
    # two row groups: an even count of whole 16-row tiles on every layer-1 case (S^2 = 64 per example) ...
    for n in ('f11-d32-b65-selu', 'f7-d32-b256-relu', 'f7-d32-b509-gelu', 'f11-d32-b509-selu', 'f2-d32-b509-elu', 'f10-d32-b509-selu'):
        (rows,) = r[n].values()
        assert rows % 32 == 0
    # ... and 1025 whole tiles on layer 2 at B = 1025: the last workgroup holds one; layer 3 ends in a tile of 4 rows
    assert r['f7-d32-b1025-selu'][2] % 16 == 0 and r['f7-d32-b1025-selu'][2] // 16 == 1025
    assert r['f7-d32-b1025-selu'][3] % 16 == 4


def test_a_wrong_want_fails(monkeypatch):
    """check_instances looks at the layer an entry names: the layer-1 instance of a case is not its layer-2 instance, a wrong paired
    flag is noticed, and a 5-tuple still means layer 0."""
    _lib()
    name = 'f7-d32-b509-gelu'
    cfg, B = gl.case_config(name), gl.CASES[name]['B']
    good = gl.CASES[name]['want']
    for bad in ([(2,) + good[0][1:]],                        # layer 2 has 8144 rows: one row group
                [good[0][:7] + (1,)],                          # not paired
                [good[0][:6] + (1, 0)],                        # no bf16x3
                [('fwd',) + good[0][2:6]],                     # layer 0 is the factorised kernel
                [(4,) + good[0][1:]]):                         # live_layers = 4
        monkeypatch.setitem(gl.CASES, name, dict(gl.CASES[name], want=bad))
        with pytest.raises(AssertionError):
            gl.check_instances(name, cfg, B)
    monkeypatch.setitem(gl.CASES, name, dict(gl.CASES[name], want=[good[0][:6], good[1]]))
    gl.check_instances(name, cfg, B)
    assert gl.want_entries('f7-d16-b5-selu')[0][:2] == (0, 'fwd')
