"""The cases of the tuple-sweep tests, shared by the CPU test of the reference (tests/test_sweep_tuples_ref.py) and the GPU tests
(tests/test_gpu_sweep_tuples.py): the shape, the swept fields in the CALLER's order, the parameters and the inputs.

Parameters are oracle.sweep_check.make_params (trained-like tables, every bias non-zero and signed: every term and every relu has
work to do), beta_outer = 0.7, lamda_att = 1.3; the log_loss variant scales the two dense kernels as sweep_check's frappe log case
does, so that the raw scores stay off the flat ends of the sigmoid.  C = 2 - 3 contexts, N = 70 candidates (one full chunk of 64 and
a ragged one), ids -1 and M in every tuple column (clamped)."""
import functools

import numpy as np

from cffm_amd.spec import CFFMConfig
from oracle import sweep_check as sc

#        name: (F, K, activation, M, C, extra config, log scale, the field lists)
SHAPES = {
    'F2': (2, 8, 'relu', 60, 3, {}, None, [(0, 1)]),                                  # no context field: Zctx = U = V = 0
    'F3': (3, 8, 'relu', 60, 3, {}, None, [(0, 2), (0, 1, 2)]),                       # one context field between; nothing fixed
    'F6-K8-elu': (6, 8, 'elu', 90, 2, {}, None, [(1, 2, 3, 4)]),                      # Pp 16
    'F8-K16-prelu-noatt': (8, 16, 'prelu', 90, 2, dict(linear_att=0), None, [(3, 4), (0, 7), (0, 3, 7)]),     # Pp 32
    'F7-gelu': (7, 8, 'gelu', 90, 2, {}, None, [(2, 5)]),
    'frappe': (10, 32, 'selu', 5382, 2, {}, None, [(1, 6)]),                          # Pp 48
    'frappe-log': (10, 32, 'selu', 5382, 2, dict(loss_type='log_loss'), (0.5, 0.0025), [(1, 6)]),
}
CASES = [(name, fields) for name, v in SHAPES.items() for fields in v[-1]]
CASE_IDS = ['%s-%s' % (name, ''.join(str(f) for f in fields)) for name, fields in CASES]
CASE_N = 70


@functools.lru_cache(maxsize=None)
def shape_of(name):
    """(cfg, params) of a named shape; the parameters are shared and must not be written to."""
    F, K, act, M, _, extra, log_scale, _ = SHAPES[name]
    cfg = CFFMConfig(M=M, F=F, K=K, D=32, activation=act, beta_outer=0.7, lamda_att=1.3, **extra)
    return cfg, sc.make_params(cfg, 0, log_scale)


def inputs_of(name, fields, N=CASE_N, C=None, per_context=False, seed=0):
    """(ctx [C][F], cand [N][nf] or [C][N][nf]) - distinct tuples, with -1 and M in every column of a list of at least 2 nf tuples."""
    cfg, _ = shape_of(name)
    C = SHAPES[name][4] if C is None else C
    nf = len(fields)
    rng = np.random.default_rng(1000 * C + N + 7 * nf + seed)
    ctx = rng.integers(0, cfg.M, size=(C, cfg.F)).astype(np.int32)
    cand = rng.integers(0, cfg.M, size=((C, N, nf) if per_context else (N, nf))).astype(np.int32)
    if N >= 2 * nf:
        for a in range(nf):
            cand[..., 2 * a, a], cand[..., 2 * a + 1, a] = -1, cfg.M
    return ctx, cand
