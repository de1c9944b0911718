"""sha256 of every parameter and slot tensor and of the loss after each step of every update route, from seeded inputs: run it once
per build of the library (CFFM_HIP_LIB + CFFM_HOST_LIB_DIR pick another build, as tools/experiments/ab_old_new.sh describes), each in
its own process, and diff the two outputs - equal digests are bit-identical updates.  The shapes are the cases of
tests/test_gpu_dp_opt.py and tests/test_gpu_update.py, the smallest that reach each route.  The first line names the library mapped."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cffm_amd import hip  # noqa: E402
from cffm_amd.spec import CFFMConfig  # noqa: E402
from tests import test_gpu_dp_opt as D  # noqa: E402
from tests import test_gpu_update as U  # noqa: E402


def digest(label, eng, *extra):
    h = hashlib.sha256()

    def walk(v):
        for k in sorted(v):
            walk(v[k]) if isinstance(v[k], dict) else h.update(np.ascontiguousarray(v[k]).tobytes())
    walk(U.state(eng))
    for t in extra:
        h.update(U.host(t).tobytes())
    print('%-60s %s' % (label, h.hexdigest()), flush=True)


def dev(a):
    return torch.from_numpy(a).cuda()


def dp_routes():
    """place / merge / radix of cffm_dp_apply_opt (SGD, Momentum) and of cffm_dp_apply (Adagrad), both losses, two applies each"""
    for route in D.ROUTES:
        for opt in D.OPTS + ['AdagradOptimizer']:
            for loss in D.LOSSES:
                eng = D._engine(route, D._config(route, opt, loss))
                rng = np.random.default_rng(len(route) + len(opt) + len(loss))
                U.spread_slots(eng, rng) if opt == 'AdagradOptimizer' else D._random_slots(eng, rng)
                for k, second in enumerate((False, True)):
                    grad, rows, n_runs, Bg, _ = D._local_half(eng, route, D._batches(route, rng, second))
                    digest('dp %s %s %s apply %d' % (route, opt, loss, k + 1), eng, eng.dp_apply(grad, rows, Bg, n_runs))


def dense_image():
    """test_dp_apply_dense's shape: the scatter of the local half (the image itself is digested), then the apply"""
    cfg = CFFMConfig(M=2000, F=10, K=32, D=32, activation='selu')
    eng = U.engine(cfg)
    rng = np.random.default_rng(9)
    U.spread_slots(eng, rng)
    for step in range(2):
        X, y = U.batch(rng, cfg.M, cfg.F, 64, 150)
        flat = eng.dp_local_dense(dev(X), dev(y), 64, 64)
        digest('dense image local %d' % step, eng, flat)
        digest('dense image apply %d' % step, eng, eng.dp_apply_dense(flat, 64), flat)


def single_gpu():
    """cffm_train_step (fused, generic, radix, l2) and cffm_train_step_opt (every optimizer x plain, l2, each disabled branch)"""
    for name, (M, F, K, Dd, B, id_range, lam) in U.TRAIN.items():
        eng = U.engine(CFFMConfig(M=M, F=F, K=K, D=Dd, activation='selu', lamda_att=1.3, lamda_bilinear=lam))
        rng = np.random.default_rng(B + F)
        for step in range(3):
            X, y = U.batch(rng, M, F, B, id_range)
            digest('train %s step %d' % (name, step), eng, eng.train_step(dev(X), dev(y)))
    for opt in ('GradientDescentOptimizer', 'MomentumOptimizer', 'AdamOptimizer'):
        for variant, kw in U.OPT_CASES.items():
            cfg = CFFMConfig(M=600, F=6, K=16, D=16, activation='elu', lamda_att=1.3, optimizer=opt, **kw)
            eng = U.engine(cfg, scale_tables=cfg.lamda_bilinear == 0)
            rng = np.random.default_rng(len(opt) + len(variant))
            for step in range(3):
                X, y = U.batch(rng, 600, 6, 40)
                digest('train %s %s step %d' % (opt, variant, step), eng, eng.train_step(dev(X), dev(y)))


def sparse_alone():
    """cffm_sparse_adagrad on test_apply_sparse's shapes (bad ids, one-id segment, disabled branches)"""
    for name, (M, K, Dd, n, ic, oc) in U.SPARSE.items():
        eng = U.engine(CFFMConfig(M=M, F=8, K=K, D=Dd, activation='relu', inner_conv=ic, outer_conv=oc))
        rng = np.random.default_rng(n + M)
        U.spread_slots(eng, rng)
        ids = U.synthetic_ids(rng, M, n)
        eng.apply_sparse(dev(ids), dev(U.grads(rng, n, K)) if ic else None, dev(U.grads(rng, n, Dd)) if oc else None,
                         dev(U.grads(rng, n)), -(-n // 8))
        digest('sparse ' + name, eng)


if __name__ == '__main__':
    hip.fast()
    print('library:', sorted({os.path.relpath(l.split()[-1], ROOT) for l in open('/proc/self/maps') if 'libcffm_hip' in l}), flush=True)
    dp_routes()
    dense_image()
    single_gpu()
    sparse_alone()
