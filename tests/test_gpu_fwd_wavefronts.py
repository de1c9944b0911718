"""GPU: the compiled-shape fused forward on 16 wavefronts per example (fwd_all_kernel<3, 16, selu, 10, 32, 32>, 1024 threads; the generic
instances keep 8).  The frappe shape (F = 10, K = D = 32, selu) with M = 200, built like case() of tests/test_gpu_frappe_instance.py,
at the batch sizes that file leaves open:

  B = 2     a grid of two workgroups
  B = 255   one below the grid of 256
  B = 257   workgroup 0 alone takes a second pass
  B = 409   the largest B with B F <= 4096 (cffm_fwd_all_ok): the second pass runs on 153 workgroups

Every case is one train step against the float64 oracle (step_check of tests/test_gpu_parity.py: loss, every post-update parameter and
Adagrad accumulator) and two engines of the same seed bit-identical after three steps.

What depends on the wavefront count and is checked here by value:
  - inner_out, the one sum of the forward whose operand grouping follows a thread count, is summed on 512 threads of the 1024
    (inner_fwd_body, NTS): step_check holds it, through the loss and every gradient, to the oracle.
  - the key placement keeps one row of counters per wavefront (rank_keys_body).  The forward places the keys itself when the fused top
    of the backward cannot do it later: defer_rank (csrc/api.hip) needs bwd_top_ok, i.e. B <= 256, so a train step at B = 257 is the
    smallest call on that path, and B = 257 / 409 above take it.  test_forward_places_keys_of_repeated_ids runs it on ids drawn from
    seven values, so that every id repeats across examples, within examples and across the two passes of workgroup 0: a key placed
    wrongly sends a row's gradient to another row or drops it, which the updated tables show against the oracle.
  - a predict call at B = 257 equals, bit for bit, the `out` of a train step on the same ids: cffm_predict runs the fused forward
    wherever the train step does (cffm_fwd_all_ok), without labels and without the key placement.  Before that it went through the
    per-stage kernels (inner_fwd_kernel on 256 threads, one launch per conv layer, head_fwd_kernel) and 91 of these 257 outputs
    differed from the train step's, by at most 192 ulp."""
import numpy as np
import pytest
import torch

from cffm_amd import hip
from tests.test_gpu_frappe_instance import FWD, CONV01, case, three_steps_twice
from tests.test_gpu_parity import engine_for, step_check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('B,bits', [(2, FWD), (255, FWD | CONV01), (257, FWD), (409, FWD)])
def test_step_at_the_grid_edges(B, bits):
    cfg, p32, X, y = case(10, 32, 32, B, seed=1000 + B)
    shape = hip.make_shape(cfg)
    assert hip.fused_instance(shape, B) == bits
    if B == 409:
        assert hip.fused_instance(shape, B + 1) & FWD == 0             # B F <= 4096 ends here
    step_check(cfg, engine_for(cfg, p32), p32, None, X, y, 'fwd-wavefronts-b%d' % B)
    three_steps_twice(cfg, p32, X, y)


def test_predict_equals_the_forward_of_a_train_step():
    B = 257
    cfg, p32, X, y = case(10, 32, 32, B, seed=77)
    ids, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    pred = engine_for(cfg, p32).predict(ids).clone()
    eng = engine_for(cfg, p32)
    eng.train_step(ids, yt)
    torch.cuda.synchronize()
    out = eng.ws_tensor(B, 'out', (B,))                                # square loss: `out` is the raw model output, as in predict
    a, b = pred.reshape(-1).cpu().numpy(), out.reshape(-1).cpu().numpy()
    ulps = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    print('predict against the train step forward, B = %d: %d elements differ, at most %d ulp, %.3g relative'
          % (B, int((ulps != 0).sum()), int(ulps.max()), float(np.max(np.abs(a - b) / np.abs(b)))))
    assert torch.equal(pred.reshape(-1), out.reshape(-1))


def test_forward_places_keys_of_repeated_ids():
    B = 257                                                            # the smallest B at which the forward places the keys itself
    cfg, p32, _, y = case(10, 32, 32, B, seed=78)
    rng = np.random.default_rng(78)
    pool = rng.choice(cfg.M, size=7, replace=False).astype(np.int32)
    X = pool[rng.integers(0, 7, size=(B, cfg.F))]
    X[256] = X[0]                                                      # both passes of workgroup 0 carry the same ids
    X[5, :] = pool[3]                                                  # one id in every field of an example
    assert hip.fused_instance(hip.make_shape(cfg), B) == FWD
    step_check(cfg, engine_for(cfg, p32), p32, None, X, y, 'fwd-wavefronts-keys')
    three_steps_twice(cfg, p32, X, y)
