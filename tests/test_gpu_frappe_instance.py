"""GPU: the kernel instances that have the frappe command's shape compiled in (F = 10, K = D = 32, selu: fwd_all_kernel<3, 8, selu, 10, 32,
32> and conv01_bwd_kernel<3, 10, 32, selu>, picked by frappe_shape() in csrc/conv.hip) and the two neighbouring shapes that must keep the
generic instances.  M = 200, so ids repeat within a batch.  Every case is one train step against the float64 oracle under the criterion
of oracle/parity.py (step_check of tests/test_gpu_parity.py: loss, every post-update parameter and Adagrad accumulator), asserts through
cffm_fused_instance which instance the launches of that (shape, B) take, and ends with two engines of the same seed bit-identical after
three steps.

B of the frappe cases: 1; 3 (grid below 256, backward below bwd_fused01_ok: per-stage layers under the fused top); 64 and 256 (both
ends of the fused backward, conv01_bwd_kernel); 300 (the forward's second pass over its grid of 256 workgroups, B F <= 4096, per-stage
backward).  The B = 64 case also runs with one id of -1 and one of M: the gather reads the clamped rows 0 and M - 1 and the update
skips the two slots, so that step must equal, bit for bit on every row but the two clamp rows, the step on the clamped ids that the
oracle was given."""
import numpy as np
import pytest
import torch

from cffm_amd import hip
from cffm_amd.spec import CFFMConfig, init_params
from tests.test_gpu_parity import engine_for, step_check

pytestmark = pytest.mark.gpu

M = 200
FWD, CONV01 = 1, 4                                     # CFFM_FUSED_INSTANCE_* (include/cffm_hip.h)
TABLES = ('inner_embeddings', 'outer_embeddings', 'feature_bias')


def case(F, K, D, B, seed):
    cfg = CFFMConfig(M=M, F=F, K=K, D=D, activation='selu', lamda_att=1.3)
    p32 = init_params(cfg, seed=seed, dtype=np.float32)
    rng = np.random.default_rng(seed + 7)
    p32['feature_bias'] = (rng.standard_normal(p32['feature_bias'].shape) * 0.3).astype(np.float32)     # 0 at init: make the term live
    p32['outer_embeddings'] = (p32['outer_embeddings'] * 20.0).astype(np.float32)
    p32['inner_embeddings'] = (p32['inner_embeddings'] * 4.0).astype(np.float32)
    X = rng.integers(0, M, size=(B, F)).astype(np.int32)
    y = rng.choice([-1.0, 1.0], size=(B,)).astype(np.float32)
    return cfg, p32, X, y


def three_steps_twice(cfg, p32, X, y):
    """Two engines from the same parameters: bit-identical losses, parameters and accumulators after three steps."""
    ids, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    runs = []
    for _ in range(2):
        eng = engine_for(cfg, p32)
        losses = [eng.train_step(ids, yt).clone() for _ in range(3)]
        torch.cuda.synchronize()
        runs.append((losses, eng.export_params(), eng.export_accumulators()))
    (la, pa, aa), (lb, pb, ab) = runs
    assert all(torch.equal(x, z) for x, z in zip(la, lb))
    for k in pa:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)
    for k in aa:
        np.testing.assert_array_equal(aa[k], ab[k], err_msg='acc ' + k)


@pytest.mark.parametrize('B,bits', [(1, FWD), (3, FWD), (64, FWD | CONV01), (256, FWD | CONV01), (300, FWD)])
def test_frappe_shape_runs_the_compiled_instances(B, bits):
    cfg, p32, X, y = case(10, 32, 32, B, seed=B)
    assert hip.fused_instance(hip.make_shape(cfg), B) == bits
    step_check(cfg, engine_for(cfg, p32), p32, None, X, y, 'frappe-instance-b%d' % B)
    if B == 64:                                        # the same step with the two slots carrying -1 and M
        Xbad = X.copy()
        (b0, f0), (b1, f1) = (5, 2), (40, 7)
        Xbad[b0, f0], Xbad[b1, f1] = -1, M
        Xc = Xbad.copy()
        Xc[b0, f0], Xc[b1, f1] = 0, M - 1              # what the gather reads for them
        ea, eb = engine_for(cfg, p32), engine_for(cfg, p32)
        yt = torch.from_numpy(y).cuda()
        la = ea.train_step(torch.from_numpy(Xbad).cuda(), yt).clone()
        lb = eb.train_step(torch.from_numpy(Xc).cuda(), yt).clone()
        torch.cuda.synchronize()
        assert torch.equal(la, lb)
        keep = np.ones(M, dtype=bool)
        keep[[0, M - 1]] = False                       # the clamp rows receive the two slots' gradients in the clamped run only
        for got_a, got_b in ((ea.export_params(), eb.export_params()), (ea.export_accumulators(), eb.export_accumulators())):
            for k in got_a:
                sel = keep if k in TABLES else Ellipsis
                np.testing.assert_array_equal(got_a[k][sel], got_b[k][sel], err_msg=k)
        X = Xbad
    three_steps_twice(cfg, p32, X, y)


@pytest.mark.parametrize('F,K', [(10, 16), (9, 32)])
def test_neighbouring_shapes_keep_the_generic_instances(F, K):
    """F = 10 with K = 16, and F = 9 with K = 32 (Pp = 48 as well): a predicate that forgets K or F would run them through kernels
    compiled for other row lengths or another pair count."""
    B = 64
    cfg, p32, X, y = case(F, K, 32, B, seed=F + K)
    assert hip.fused_instance(hip.make_shape(cfg), B) == 0
    assert hip.fused_instance(hip.make_shape(cfg), 300) == 0
    step_check(cfg, engine_for(cfg, p32), p32, None, X, y, 'frappe-neighbour-f%d-k%d' % (F, K))
    three_steps_twice(cfg, p32, X, y)
