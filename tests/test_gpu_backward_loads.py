"""GPU: the staging loops of the backward that request a thread's loads together before they consume them (loads_first / ParkFilter of
csrc/common.hpp), at the sizes where a batched loop can go wrong.  M = 200, so ids repeat within a batch.  Every case is one train step
against the float64 oracle under the criterion of oracle/parity.py (step_check of tests/test_gpu_parity.py: loss, every post-update
parameter and Adagrad accumulator) and ends with two engines of the same seed bit-identical after three steps.

* D = 16, 32, 64 at B = 64: the dense(32) weight-gradient slab of head_bwd_example has (2 D - 2) * 32 elements over 256 threads - 3.75,
  7.75 and 15.75 trips against a batch of 8: a partial batch, a partial last trip, and two batches.
* F = 2, 9, 11: the attention row lengths (one batch of 12 with 2, 9, 11 live registers), and Pp = 16, 48, 64, so that the dC tile of the
  64-row weight gradient takes 1, 3 and 4 trips.  Pp = 64 is too wide for conv01_bwd_kernel and goes through conv_bwd_pair_kernel and the
  stand-alone layer-0 kernel, which share the bodies.
* B = 3 (per-stage layers under the fused top), 64 and 256 (both ends of conv01_bwd_kernel) at F = 10, K = D = 32.
* B = 100: 156 workgroups of every role have no example - their loops take no trip, must still pad and pass their barriers, and their
  slabs must read as zeros.

No shape of this list is refused by a predicate: a shape outside a fused kernel's domain takes the per-stage launches, which run the
same bodies."""
import numpy as np
import pytest
import torch

from tests.test_gpu_frappe_instance import case, three_steps_twice
from tests.test_gpu_parity import engine_for, step_check
from tests.test_gpu_update_chains import slab_plan

pytestmark = pytest.mark.gpu

#        F   K   D   B
SHAPES = [(10, 16, 16, 64), (10, 32, 32, 64), (10, 16, 64, 64),         # slab loop: 3.75 / 7.75 / 15.75 trips
          (2, 32, 32, 64), (9, 32, 32, 64), (11, 8, 32, 64),            # attention rows of 2 / 9 / 11, dC tile of 1 / 3 / 4 trips
          (10, 32, 32, 3), (10, 32, 32, 256)]                           # per-stage layers under the fused top; the full grid


@pytest.mark.parametrize('F,K,D,B', SHAPES, ids=['f%d-k%d-d%d-b%d' % s for s in SHAPES])
def test_batched_loops_step_matches_the_oracle_and_is_reproducible(F, K, D, B):
    cfg, p32, X, y = case(F, K, D, B, seed=F + D + B)
    step_check(cfg, engine_for(cfg, p32), p32, None, X, y, 'backward-loads-f%d-k%d-d%d-b%d' % (F, K, D, B))
    three_steps_twice(cfg, p32, X, y)


def test_workgroups_without_an_example_take_no_trip_and_write_zero_slabs():
    F, K, D, B = 10, 16, 32, 100
    cfg, p32, X, y = case(F, K, D, B, seed=100)
    step_check(cfg, engine_for(cfg, p32), p32, None, X, y, 'backward-loads-b100')
    eng = engine_for(cfg, p32)
    plan, total = slab_plan(cfg, eng.tl, B)
    _, wl = eng.workspace(B)
    assert total == int(wl.gpart_floats)
    Pp = int(eng.tl.Pp)
    # head front, inner branch, layer 0, layer 1 and head back: one slab per workgroup, 156 of them without an example.  The head
    # and the inner branch zero their whole range, layer 0 its filter gradient and bias; of layer 1 the filter gradient (the first
    # 4 Pp Pp floats of the slab) is what the weight gradient behind the dC tile writes.
    ranges = {0: None, 1: None, 2: None, 3: 4 * Pp * Pp, len(plan) - 1: None}
    gpart = eng.ws_tensor(B, 'gpart', (total,))
    for r, head in ranges.items():
        off, ln, base, nslab = plan[r]
        assert nslab == 256 and B < nslab
        slabs = gpart[base:base + nslab * ln].view(nslab, ln)
        slabs[B:, :head if head else ln].fill_(float('nan'))           # what the workgroups without an example must overwrite
    eng.train_step(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda())
    torch.cuda.synchronize()
    gp = gpart.cpu().numpy()
    for r, head in ranges.items():
        off, ln, base, nslab = plan[r]
        slabs = gp[base:base + nslab * ln].reshape(nslab, ln)[:, :head if head else ln]
        assert not np.any(slabs[B:]), 'range %d: a slab past the batch is not zero' % r
        assert np.any(slabs[:B]), 'range %d: no slab of the batch was written' % r
    three_steps_twice(cfg, p32, X, y)
