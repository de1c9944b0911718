"""GPU: the head backward inside the fused top of the backward (bwd_top_kernel, role 2) in its single-example form
(head_bwd_example_one / head_bwd_end_one, csrc/head_body.hpp): wavefront 0 carries d -> dh -> dt1 -> dC_top, wavefronts 1 and 2 the
dense(32) weight-gradient slab, wavefront 3 the attention / first-order branch, and the per-example sums are stored from the lanes
that hold them.  M = 200, so ids repeat within a batch; parameters scaled as in tests/test_gpu_frappe_instance.py so that every term is
live (non-zero feature_bias, scaled embeddings, lamda_att != 1).

Shapes: the smallest at which each lane mapping can go wrong -
  F10 K32 D32 selu, B 1 / 3 / 64 / 256   the benchmarked instance; at B = 3, 253 workgroups have no example and leave zero slabs; B < 64
                                         runs the stage layers below the top
  F11 K32 D32 relu, B 8                  Pp = 64, NT = 4: dC_top has 256 elements, four per lane of wavefront 0
  F2  K4  D8  relu, B 5                  P = 1, t1w = 14 (fewer rows of dense(32) than units), F = 2
  F6  K32 D64 elu,  B 4                  t1w = 126: two k per lane, dC_top's two dt1 values on the second k of lanes 60 / 61; the slab of
                                         wavefronts 1 and 2 takes a second batch
  F10 K32 D32 selu, linear_att off       the arm that only copies d into dfb
  F10 K32 D32 selu, log_loss / hybrid    other barrier counts in head_bwd_loss in front of the head phase

Per case:
1. one train step against the float64 oracle under step_check of tests/test_gpu_parity.py (loss, every post-update parameter, every
   accumulator): a gradient stored from the wrong lane moves its parameter;
2. two engines from the same seed are bit-identical after three steps;
3. (square_loss cases) a reference that is not the code under test: after one forward, backward_dout (the stage route: head_bwd_dout_kernel
   on the looping form of the head backward) and backward_dout_fused (the fused top, DOUT instance) from the same seeded dL/dout must
   leave the same bits in the per-example head outputs ws.dt1, ws.dfb and ws.dC[live - 1] - they do not depend on how examples map to
   slabs.  The log_loss / hybrid cases leave this out: the DOUT instances form no loss, so their barrier count is the same for every
   loss type and the square_loss cases cover them.
And once: a fused list step (bpr, G = 2, Lg = 3, frappe shape) under the criterion of tests/test_gpu_list_step.py::test_one_fused_list_step,
the DOUT instance end to end.

The hybrid case keeps the initial embeddings, with feature_bias * 0.05, bias = 0.5 and beta_outer = 0.001: log_loss on the raw out
(CFFM.py:511-513) is finite only for 0 < out < 1 (tests/test_gpu_parity.py::test_other_losses does the same at F = 4, D = 8), and at
F = 10, D = 32 the outer branch alone is about -205 at beta_outer = 1.  The case asserts 0.05 < out < 0.95 on the oracle's forward, and
its lr is 1e-4: Adagrad's first step moves every parameter by about lr, and at 0.05 the second step's out is outside (0, 1) and its
loss NaN, which no bit comparison of two runs survives."""
import numpy as np
import pytest
import torch

from cffm_amd.spec import CFFMConfig, init_params
from oracle import cffm_oracle as orc
from oracle.parity import to64
from tests import test_gpu_list_step as LS
from tests.test_gpu_backward_dout import _same_bits
from tests.test_gpu_frappe_instance import three_steps_twice
from tests.test_gpu_parity import engine_for, step_check

pytestmark = pytest.mark.gpu

M = 200
CASES = {
    'f10-d32-selu-b1': dict(F=10, K=32, D=32, act='selu', B=1),
    'f10-d32-selu-b3': dict(F=10, K=32, D=32, act='selu', B=3),
    'f10-d32-selu-b64': dict(F=10, K=32, D=32, act='selu', B=64),
    'f10-d32-selu-b256': dict(F=10, K=32, D=32, act='selu', B=256),
    'f11-d32-relu-b8': dict(F=11, K=32, D=32, act='relu', B=8),
    'f2-k4-d8-relu-b5': dict(F=2, K=4, D=8, act='relu', B=5),
    'f6-d64-elu-b4': dict(F=6, K=32, D=64, act='elu', B=4),
    'f10-d32-selu-nolinatt-b5': dict(F=10, K=32, D=32, act='selu', B=5, linear_att=0),
    'f10-d32-selu-logloss-b6': dict(F=10, K=32, D=32, act='selu', B=6, loss='log_loss'),
    'f10-d32-selu-hybrid-b6': dict(F=10, K=32, D=32, act='selu', B=6, loss='hybrid'),
}


def case(name):
    c = CASES[name]
    loss = c.get('loss', 'square_loss')
    cfg = CFFMConfig(M=M, F=c['F'], K=c['K'], D=c['D'], activation=c['act'], lamda_att=1.3, linear_att=c.get('linear_att', 1),
                     loss_type=loss, beta_outer=0.001 if loss == 'hybrid' else 1.0, lr=1e-4 if loss == 'hybrid' else 0.05)
    seed = sum(map(ord, name))
    p32 = init_params(cfg, seed=seed, dtype=np.float32)
    rng = np.random.default_rng(seed + 7)
    X = rng.integers(0, M, size=(c['B'], cfg.F)).astype(np.int32)
    y = rng.choice([-1.0, 1.0], size=(c['B'],)).astype(np.float32)
    if loss == 'hybrid':
        p32['feature_bias'] = (rng.standard_normal(p32['feature_bias'].shape) * 0.05).astype(np.float32)
        p32['bias'] = np.float32(0.5)
        out, _ = orc.forward(to64(p32), X, cfg)
        assert (out > 0.05).all() and (out < 0.95).all()
    else:
        p32['feature_bias'] = (rng.standard_normal(p32['feature_bias'].shape) * 0.3).astype(np.float32)   # 0 at init: make the term live
        p32['outer_embeddings'] = (p32['outer_embeddings'] * 20.0).astype(np.float32)
        p32['inner_embeddings'] = (p32['inner_embeddings'] * 4.0).astype(np.float32)
    if loss == 'log_loss':
        y = (y > 0).astype(np.float32)
    return cfg, p32, X, y


def head_outputs(eng, cfg, B):
    """The per-example outputs of the head backward: bits on the host."""
    top = cfg.live_layers - 1
    S = cfg.D >> (top + 1)
    torch.cuda.synchronize()
    views = {'dt1': eng.ws_tensor(B, 'dt1', (B, 2 * cfg.D - 2)), 'dfb': eng.ws_tensor(B, 'dfb', (B, cfg.F)),
             'dC[%d]' % top: eng.ws_tensor(B, 'dC', (B, S, S, eng.tl.Pp), index=top)}
    return {k: v.detach().cpu().numpy().copy() for k, v in views.items()}


@pytest.mark.parametrize('name', list(CASES))
def test_head_backward_of_the_fused_top(name):
    cfg, p32, X, y = case(name)
    B = X.shape[0]
    step_check(cfg, engine_for(cfg, p32), p32, None, X, y, 'bwd-top-head-' + name)
    three_steps_twice(cfg, p32, X, y)
    if cfg.loss_type != 'square_loss':
        return
    eng = engine_for(cfg, p32)
    assert bool(eng.lib.cffm_list_step_ok(eng._s, B))            # the fused top serves (shape, B): backward_dout_fused runs
    ids = torch.from_numpy(X).cuda()
    dout = torch.from_numpy(np.random.default_rng(B + cfg.F).standard_normal(B).astype(np.float32)).cuda()
    eng.forward(ids, None)
    eng.backward_dout(dout, B)                                   # stage route: the looping form, one kernel per stage
    want = head_outputs(eng, cfg, B)
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in want.values())
    eng.forward(ids, None)
    for k in ('dt1', 'dfb'):
        eng.ws_tensor(B, k, want[k].shape).fill_(float('nan'))
    eng.backward_dout_fused(dout, B)
    _same_bits(head_outputs(eng, cfg, B), want, name + ': fused top vs stage route')


def test_fused_list_step_at_the_frappe_shape(monkeypatch):
    """The DOUT instance of the fused top end to end: tests/test_gpu_list_step.py::test_one_fused_list_step, its checks and bounds as
    they are, on two lists of three (its own case builder needs three lists): the same context twice, a candidate repeated within a
    list and across the lists, a target at position 0 and one at Lg - 1."""
    def two_lists(name):
        cfg = CFFMConfig(M=60 * 10, F=10, K=32, D=32, activation='selu', lamda_att=1.3)
        rng = np.random.default_rng(3)
        p32 = LS.scaled_params(cfg, 0, rng)
        ctx = rng.integers(0, cfg.M, size=(2, cfg.F)).astype(np.int32)
        ctx[1] = ctx[0]
        cand = rng.integers(0, 12, size=(2, 3, 2)).astype(np.int32) * 5
        cand[0, 2] = cand[0, 0]
        cand[1, 1] = cand[0, 1]
        return cfg, p32, ctx, [2, 7], cand, np.array([0, 2], dtype=np.int32)
    monkeypatch.setattr(LS, 'step_case', two_lists)
    LS.test_one_fused_list_step('f10-d32-g2x3', 'bpr')
