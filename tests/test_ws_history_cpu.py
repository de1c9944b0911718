"""The member map and the fills of tests/_ws_history.py, on the host (the layout query needs no GPU): the map tiles the workspace,
every field of cffm_ws_layout_t is classified, the integer fills stay in range, and every batch pair of the GPU test
(tests/test_gpu_ws_history.py) really leaves one member's bytes where the next run keeps another."""
import ctypes as C

import numpy as np
import pytest

from cffm_amd import hip
from cffm_amd.spec import CFFMConfig
from tests import _ws_history as H
from tests import test_gpu_branches as br
from tests import test_gpu_parity as par


def shape_of(c, **kw):
    cfg = CFFMConfig(M=c['M'], F=c['F'], K=c['K'], D=c['D'], activation=c['act'], lamda_att=1.3, linear_att=c.get('linear_att', 1),
                     inner_conv=c.get('inner_conv', 1), outer_conv=c.get('outer_conv', 1))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return hip.make_shape(cfg), cfg


def gpu_cases():
    """[(label, case dict, B of the leftover run, config overrides)] of every (shape, B) the GPU test enters a sequence at."""
    out = [(n, par.CASES[n], H.leftover_batch(par.CASES[n]['B']), {}) for n in H.TRAIN_CASES]
    out += [(H.pair_name(Bo, B), H.pair_case(B), Bo, {}) for Bo, B in H.FRAPPE_PAIRS]
    out += [('%s %s' % (n, o), par.CASES[n], H.leftover_batch(par.CASES[n]['B']), dict(optimizer=o)) for n in H.OPT_CASES for o in H.OPTIMIZERS]
    out += [('loss square_l2', H.LOSS_SHAPE, H.leftover_batch(H.LOSS_SHAPE['B']), dict(lamda_bilinear=0.02))]
    out += [('loss ' + l, H.LOSS_SHAPE, H.leftover_batch(H.LOSS_SHAPE['B']), dict(loss_type=l)) for l in H.LOSSES[1:]]
    out += [(n, br.CASES[n], H.leftover_batch(br.CASES[n]['B']), {}) for n in H.PACKED_CASES]
    return out


CASES = gpu_cases()
IDS = [c[0] for c in CASES]


def check_tiling(label, wl):
    mm = H.member_map(wl)
    at = 0
    for name, off, ln, kind in mm:
        assert off == at and ln >= 0, '%s: member %s starts at %d, the one before it ends at %d' % (label, name, off, at)
        assert kind in (H.FLOAT, H.INT) and off % 256 == 0
        at = off + ln
    assert at == int(wl.bytes), label
    names = [m[0] for m in mm]
    assert len(set(names)) == len(names) and names[0] == 'gpart'
    assert mm[0][2] >= 4 * int(wl.gpart_floats)
    return mm


def test_case_lists_name_existing_cases():
    assert len(H.TRAIN_CASES) == 19 and len(set(H.TRAIN_CASES)) == 19
    for n in H.TRAIN_CASES + H.OPT_CASES + H.SEQUENCE_CASES:
        assert n in par.CASES and not par.CASES[n].get('heavy'), n
    for n in H.PACKED_CASES:
        assert br.CASES[n].get('packed'), n
    assert sorted(n for n, c in br.CASES.items() if c.get('packed')) == sorted(H.PACKED_CASES)


@pytest.mark.parametrize('label,c,B_other,kw', CASES, ids=IDS)
def test_member_map_tiles_the_workspace(label, c, B_other, kw):
    shape, cfg = shape_of(c, **kw)
    for B in sorted(set(H.EVAL_BATCHES) | {c['B'], B_other}):
        mm = check_tiling('%s B=%d' % (label, B), hip.ws_layout(shape, B))
        used = {m[0] for m in mm}
        assert {'scalars', 'fb', 'out', 'dout', 'dfb', 'sort_keys', 'sort_vals', 'sort_tmp'} <= used
        assert ('Gi' in used) == (kw.get('optimizer') == 'AdamOptimizer' or 'lamda_bilinear' in kw)
        assert ('C[0]' in used) and ('C[%d]' % cfg.live_layers) not in used


def test_every_field_is_classified():
    names = [f[0] for f in hip.WsLayout._fields_]
    assert sorted(names) == sorted(H.MEMBER_KINDS)
    assert sorted(n for n, k in H.MEMBER_KINDS.items() if k == H.INT) == ['relu0', 'sort_keys', 'sort_tmp', 'sort_vals']

    class Wider(C.Structure):                                     # the struct after somebody added a member
        _fields_ = list(hip.WsLayout._fields_) + [('new_member', C.c_int64)]

    shape, _ = shape_of(par.CASES['frappe-selu'])
    wl = hip.ws_layout(shape, 256)
    wider = Wider()
    C.memmove(C.addressof(wider), C.addressof(wl), C.sizeof(wl))
    wider.new_member = int(wl.bytes) - 256
    with pytest.raises(ValueError, match='new_member'):
        H.member_map(wider)
    assert H.member_map(wl)                                       # and the real struct goes through


@pytest.mark.parametrize('label,c,B_other,kw', CASES, ids=IDS)
def test_integer_fills_stay_in_range(label, c, B_other, kw):
    shape, cfg = shape_of(c, **kw)
    B = c['B']
    n_slots = B * cfg.F
    rng = np.random.default_rng(0)
    seen = set()
    for name, off, ln, kind in H.member_map(hip.ws_layout(shape, B)):
        if kind != H.INT:
            continue
        seen.add(name)
        data = H.int_fill(name, ln, cfg.M, n_slots, rng)
        if name == 'sort_tmp':
            assert data is None
            continue
        assert data.dtype == np.uint8 and data.size == ln
        if name in ('sort_keys', 'sort_vals'):
            keys = data.view(np.int64)
            ids, slots = keys >> 32, keys & 0xffffffff
            assert ids.min() >= 0 and ids.max() < cfg.M and slots.min() >= 0 and slots.max() < n_slots
            assert keys.size >= n_slots and set(slots.tolist()) == set(range(n_slots))      # every slot is there: a permutation
            words = data.view(np.int32)                         # read as 32-bit indices they are in range too
            assert words.min() >= 0 and words.max() < max(cfg.M, n_slots)
            if name == 'sort_vals':
                assert (np.diff(keys) >= 0).all()
    assert {'sort_keys', 'sort_vals', 'sort_tmp'} <= seen
    with pytest.raises(ValueError):
        H.int_fill('Ei', 256, cfg.M, n_slots, rng)


@pytest.mark.parametrize('label,c,B_other,kw', CASES, ids=IDS)
def test_batch_pairs_move_members_onto_each_other(label, c, B_other, kw):
    """Why these pairs: at least one float member of the case's layout lies on bytes that are a DIFFERENT member in the layout of
    the leftover run in front of it (at the frappe pairs: gpart itself, whose size is what changes with the slab plan)."""
    shape, _ = shape_of(c, **kw)
    first, second = H.member_map(hip.ws_layout(shape, B_other)), H.member_map(hip.ws_layout(shape, c['B']))
    hit = H.overlaps(first, second)
    assert hit, label
    assert any(a in ('gpart', 'scalars') or b in ('gpart', 'scalars') for a, b in hit) or len(hit) > 4, (label, hit[:4])


def test_frappe_pairs_cross_the_slab_plan_changes():
    shape, _ = shape_of(H.PAIR_SHAPE)
    floats = {B: int(hip.ws_layout(shape, B).gpart_floats) for pair in H.FRAPPE_PAIRS for B in pair}
    for Bo, B in H.FRAPPE_PAIRS:
        assert floats[Bo] != floats[B] or (Bo, B) == (64, 65), (Bo, B, floats)
    assert H.FRAPPE_PAIRS == ((300, 100), (100, 300), (1024, 64), (64, 65), (256, 257))


def test_exemptions_are_pinned():
    assert H.EXEMPT == {}


def test_mismatch_message_names_history_tensor_index_and_theta_range():
    shape, _ = shape_of(par.CASES['frappe-selu'])
    tl = hip.theta_layout(shape)
    rngs = H.theta_ranges(tl)
    assert rngs[0][1] == 0 and rngs[-1][2] == int(tl.n) and all(a[2] == b[1] for a, b in zip(rngs, rngs[1:]))
    ref = np.zeros(int(tl.n), dtype=np.float32)
    ref[5] = np.nan
    got = ref.copy()
    H.assert_same('nan', 'theta', got, ref, tl)                   # NaN == NaN, as assert_array_equal has it
    i = int(tl.conv_w[1]) + 7
    got[i] = 1.0
    with pytest.raises(AssertionError, match=r'history nan: theta .* index %d \(theta range conv_w\[1\] \+ 7\)' % i):
        H.assert_same('nan', 'theta', got, ref, tl)
    assert H.first_mismatch(got, ref) == i
