"""The list steps with the logQ-corrected softmax on the device: HipEngine.train_step_lists_fused(..., lists, corr)
(cffm_train_step_lists_logq) and HipEngine.train_step_lists(..., lists, corr), at the frappe shape (F = 10, K = D = 32, selu; G = 4
lists of 4) and at one shape that takes the stage forward inside the fused step (F = 4, D = 8; G = 3 lists of 2).

1. The fused step is, bit for bit, the composition expand -> forward -> list_loss(lists, corr) -> cffm_backward_dout_fused -> update
   on a second engine of the same parameters: scores, dL/dout, terms, loss, parameters and accumulators byte-equal.  The forward is
   the label-less one the step itself runs: the single launch of cffm_predict where there is one, cffm_forward elsewhere.
2. Both routes against float64, held exactly as tests/test_gpu_list_step.py::test_one_fused_list_step holds the uncorrected step, with
   cffm_amd.spec.list_loss_logq as the loss.
3. With an all-zero table both routes are byte-equal to the uncorrected step.
4. A refused call (bpr; a missing operand; a shape the fused route does not serve) leaves parameters and accumulators alone."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cffm_amd import hip, spec  # noqa: E402
from cffm_amd.spec import init_params  # noqa: E402
from oracle import cffm_oracle as orc  # noqa: E402
from oracle import parity as T  # noqa: E402
from oracle import update_check as uc  # noqa: E402
from oracle.parity import adopt_device_kinks, close, inner_kink_slack, to64  # noqa: E402
from tests import _cand_ref as CR  # noqa: E402
from tests import _list_logq_ref as Q  # noqa: E402
from tests.test_gpu_list_step import dev, engine_for, step_case  # noqa: E402
from tests.test_gpu_update import host, pads_unchanged, row_inputs, state  # noqa: E402

pytestmark = pytest.mark.gpu
assert 'cffm_train_step_lists_logq' in hip.PROTOTYPES          # the entry point this file is about

CASES = {'f10-d32-g4x4': ('f10-d32-g16x4', dict(G=4)),          # the single-launch forward
         'f4-d8-g3x2': ('f4-d8-g6x4', dict(G=3, Lg=2))}         # the stage forward inside the fused step
U = 66


def case(name):
    """step_case at the sizes of this file, plus lists int32 [G, Lg] (a repeated index among them) and a table with corrections of
    both signs up to |c| ~ 4."""
    base, over = CASES[name]
    cfg, p32, ctx, fields, cand, target = step_case(base, **over)
    G, Lg = cand.shape[:2]
    if cfg.D == 32:
        # Under the x20 / x4 embeddings of step_case the scores of a frappe-shape list lie 800 - 2000 apart: the softmax is saturated,
        # dout is 0 or +-1 / G whatever the correction, and a step that dropped lists and corr would pass.  At the initial scale they
        # lie 2 - 5 apart (float64 oracle) and a correction of a few units moves every element of dout.
        p32 = init_params(cfg, seed=0, dtype=np.float32)
        p32['feature_bias'] = (np.random.default_rng(3).standard_normal(p32['feature_bias'].shape) * 0.3).astype(np.float32)
    rng = np.random.default_rng(17 + G)
    lists = rng.integers(0, U, size=(G, Lg)).astype(np.int32)
    lists[1, 1] = lists[1, 0]
    return cfg, p32, ctx, fields, cand, target, lists, Q.table(U, 5, span=3.0)


def same_state(label, a, b):
    for k in ('theta', 'inner', 'outer', 'fbias'):
        uc.check_exact('%s %s' % (label, k), a[k], b[k])
        uc.check_exact('%s slot %s' % (label, k), a['s1'][k], b['s1'][k])


def step_outputs(eng, G, Lg):
    B = G * Lg
    dout, terms = eng._ws[('list_out', G, Lg)]
    return {'ids': host(eng._ws[('list_ids', B)]), 'out': host(eng.ws_tensor(B, 'out', (B,))), 'dout': host(dout), 'terms': host(terms),
            'loss': host(eng.loss_buf).reshape(-1)[:1]}


# ---- 1. the fused step is the composition -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_the_fused_step_is_the_composition(name):
    cfg, p32, ctx, fields, cand, target, lists, corr = case(name)
    G, Lg = cand.shape[:2]
    B = G * Lg
    args = (dev(ctx), fields, dev(cand), dev(target), 'softmax')
    a = engine_for(cfg, p32)
    assert a.list_step_ok(B)
    pre = state(a)
    a.train_step_lists_fused(*args, lists=dev(lists), corr=dev(corr))
    got, post = step_outputs(a, G, Lg), state(a)
    assert not np.array_equal(post['theta'], pre['theta'])
    # the composition, call by call
    b = engine_for(cfg, p32)
    ids = torch.empty((B, cfg.F), dtype=torch.int32, device='cuda')
    hf = (C.c_int32 * len(fields))(*fields)
    hip.check(b.lib.cffm_expand_candidates_ex(b._s, ctx_ptr(args[0]), G, C.addressof(hf), len(fields), args[2].data_ptr(),
                                              Lg * len(fields), Lg, 0, B, ids.data_ptr(), b._stream()))
    if b.lib.cffm_dp_runs_ok(b._s, B):                       # the label-less single launch the step runs there: that of predict
        b.predict(ids)
    else:
        b.forward(ids, None)
    out = b.ws_tensor(B, 'out', (B,)).clone()
    loss, dout, terms = b.list_loss(out, args[3], G, Lg, 'softmax', lists=dev(lists), corr=dev(corr))
    b.backward_dout_fused(dout, B)
    b.apply_dense()
    dEi, dEo, dfb = b.row_grads(B)
    b.apply_sparse(ids, dEi, dEo, dfb, B)
    want = {'ids': host(ids), 'out': host(out), 'dout': host(dout), 'terms': host(terms), 'loss': host(loss).reshape(-1)[:1]}
    for k in ('ids', 'out', 'dout', 'terms', 'loss'):
        uc.check_exact('%s: fused step vs composition, %s' % (name, k), got[k], want[k])
    assert np.isfinite(want['loss']).all() and np.abs(want['dout']).max() > 0
    same_state('%s: fused step vs composition' % name, post, state(b))


def ctx_ptr(t):
    assert t.dtype == torch.int32 and t.is_contiguous()
    return t.data_ptr()


# ---- 2. both routes against float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['fused', 'stages'])
@pytest.mark.parametrize('name', list(CASES))
def test_one_corrected_step_against_float64(name, route):
    cfg, p32, ctx, fields, cand, target, lists, corr = case(name)
    G, Lg = cand.shape[:2]
    B = G * Lg
    X = CR.expand_tuples(ctx, fields, cand).astype(np.int32)
    p64 = to64(p32)
    out_ref, c = orc.forward(p64, X, cfg)
    loss_ref, dout_ref, _ = spec.list_loss_logq(out_ref.reshape(G, Lg), target, lists, corr)
    raw = spec.list_loss_logq(out_ref.reshape(G, Lg), target, lists, np.zeros_like(corr))
    assert np.abs(dout_ref - raw[1]).max() > 1e-2 * np.abs(raw[1]).max()          # the correction is felt
    eng = engine_for(cfg, p32)
    run = eng.train_step_lists_fused if route == 'fused' else eng.train_step_lists
    pre = state(eng)
    L = run(dev(ctx), fields, dev(cand), dev(target), 'softmax', lists=dev(lists), corr=dev(corr))
    post = state(eng)
    tag = '%s list step logq' % route
    assert np.array_equal(host(eng._ws[('list_ids', B)]), X)
    close(host(eng.ws_tensor(B, 'out', (B,))), out_ref, tag + ' out')
    close(host(L), np.array([loss_ref]), tag + ' loss')
    # the terms against the twin on the device's own scores: a term carries its scores' error one to one, the mean above averages it
    out_dev = host(eng.ws_tensor(B, 'out', (B,))).reshape(G, Lg)
    close(host(eng._ws[('list_out', G, Lg)][1]), spec.list_loss_logq(out_dev, target, lists, corr)[2], tag + ' terms')
    print('%s: %d relu decisions adopted from the device' % (name, adopt_device_kinks(cfg, eng, B, c)))
    dout = dout_ref.reshape(-1)
    g = orc.backward(p64, c, dout, cfg)
    slack = inner_kink_slack(p64, c, dout, cfg)
    # dL/dout is taken from scores that close() holds to delta = TOL * (|out| + rms(out)), and an unsaturated softmax passes that on:
    # d p_n / d z_k = p_n ([n = k] - p_k), so |delta p_n| <= p_n (|delta_n| + sum_k p_k |delta_k|) <= 2 p_n max_k delta_k over the list.
    # (The uncorrected file needs no such term: its frappe-shape lists are saturated, p is 0 or 1 to the last bit.)
    delta = T.TOL * (np.abs(out_ref) + float(np.sqrt(np.mean(out_ref * out_ref)))).reshape(G, Lg)
    p_ref = dout_ref * G
    p_ref[np.arange(G), target] += 1.0
    from_scores = (2.0 * p_ref * delta.max(axis=1, keepdims=True) / G).reshape(-1)
    close(host(eng.ws_tensor(B, 'dout', (B,))), dout, tag + ' dout', extra=from_scores)
    assert np.array_equal(host(eng.ws_tensor(B, 'dout', (B,))).view(np.uint32), host(eng._ws[('list_out', G, Lg)][0]).view(np.uint32))
    # the slack terms of test_one_fused_list_step: dL/dout is the device's own, held to close(), and every gradient is linear in it
    dsl = T.TOL * (np.abs(dout) + float(np.sqrt(np.mean(dout * dout)))) + from_scores
    rel_b = np.repeat(dsl / np.maximum(np.abs(dout), 1e-300), cfg.F)[:, None]
    dgs = T.dense_grad_slack(p64, c, dsl, cfg)
    rows = row_inputs(eng, B)
    ref = g['d_outer_rows'].reshape(B * cfg.F, -1)
    close(rows['dEo'], ref, tag + ' dEo', extra=rel_b * np.abs(ref))
    ref = g['d_inner_rows'].reshape(B * cfg.F, -1)
    close(rows['dEi'], ref, tag + ' dEi',
          extra=rel_b * np.abs(ref) + (slack['d_inner_rows'].reshape(B * cfg.F, -1) if 'd_inner_rows' in slack else 0.0))
    ref = g['d_bias_rows'].reshape(-1)
    close(rows['dfb'], ref, tag + ' dfb', extra=rel_b[:, 0] * np.abs(ref))
    for k, v in eng.export_grad().items():
        extra = np.asarray(dgs[k]).reshape(v.shape) + (slack[k].reshape(v.shape) if k in slack else 0.0)
        close(v, np.asarray(g[k]).reshape(v.shape), tag + ' grad ' + k, extra=extra)
    label = '%s %s' % (tag, name)
    rep = uc.replay('AdagradOptimizer', pre, host(eng.grad), X.reshape(-1), rows, cfg.M, cfg.lr)
    uc.check_update(label, pre, post, rep)
    pads_unchanged(label, eng, pre, post)


# ---- 3. an all-zero table is the uncorrected step ---------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['fused', 'stages'])
@pytest.mark.parametrize('name', list(CASES))
def test_an_all_zero_table_is_the_uncorrected_step(name, route):
    cfg, p32, ctx, fields, cand, target, lists, corr = case(name)
    G, Lg = cand.shape[:2]
    args = (dev(ctx), fields, dev(cand), dev(target), 'softmax')
    a, b = engine_for(cfg, p32), engine_for(cfg, p32)
    run = lambda e: e.train_step_lists_fused if route == 'fused' else e.train_step_lists
    for _ in range(2):                                       # two steps: the second starts from moved parameters
        run(a)(*args, lists=dev(lists), corr=dev(np.zeros_like(corr)))
        run(b)(*args)
        got, want = step_outputs(a, G, Lg), step_outputs(b, G, Lg)
        for k in got:
            uc.check_exact('%s %s zero table: %s' % (name, route, k), got[k], want[k])
        same_state('%s %s zero table' % (name, route), state(a), state(b))
    assert np.isfinite(want['loss']).all()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_a_refused_call_leaves_the_state_alone():
    cfg, p32, ctx, fields, cand, target, lists, corr = case('f10-d32-g4x4')
    eng = engine_for(cfg, p32)
    pre = state(eng)
    args = (dev(ctx), fields, dev(cand), dev(target))
    for run in (eng.train_step_lists_fused, eng.train_step_lists):
        with pytest.raises(ValueError, match="kind 'bpr' has none"):
            run(*args, 'bpr', lists=dev(lists), corr=dev(corr))
        with pytest.raises(ValueError, match='lists and corr go together: corr is missing'):
            run(*args, 'softmax', lists=dev(lists))
        with pytest.raises(ValueError, match='lists and corr go together: lists is missing'):
            run(*args, 'softmax', corr=dev(corr))
        with pytest.raises(ValueError, match=r'lists must be int32 \[G = 4, Lg = 4\]'):
            run(*args, 'softmax', lists=dev(lists[:3]), corr=dev(corr))
        with pytest.raises(ValueError, match=r'corr must be a contiguous fp32 \[U, 2\]'):
            run(*args, 'softmax', lists=dev(lists), corr=dev(corr.astype(np.float64)))
    with pytest.raises(ValueError, match="kind 'bpr' has none"):
        eng.list_loss(torch.zeros(16, device='cuda'), args[3], 4, 4, 'bpr', lists=dev(lists), corr=dev(corr))
    # the library's own refusal of bpr, through the binding
    rc = eng.lib.cffm_list_loss_logq(hip.LIST_LOSS_IDS['bpr'], 0, 4, 4, 0, 0, 0, U, 0, 0, 0, 0, 0)
    assert rc == 10002
    same_state('refused calls', state(eng), pre)
    # a size the fused route does not serve: B = 260
    cfg, p32, ctx, fields, cand, target = step_case('f10-d32-g16x4', G=65)
    eng = engine_for(cfg, p32)
    pre = state(eng)
    big = np.zeros((65, 4), dtype=np.int32)
    with pytest.raises(ValueError, match='260'):
        eng.train_step_lists_fused(dev(ctx), fields, dev(cand), dev(target), 'softmax', lists=dev(big), corr=dev(corr))
    same_state('B = 260', state(eng), pre)
