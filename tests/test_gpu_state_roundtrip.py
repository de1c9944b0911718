"""A fresh HipEngine that loads what another one exported holds the same bytes in every state tensor: theta, the three tables
and every optimizer slot, the channel pads of the conv members included (they are not part of an export: load_params puts the
initial accumulator back into the pads of the first slots and zeros into those of theta and of the second slots)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cffm_amd.spec import CFFMConfig, init_params  # noqa: E402

pytestmark = pytest.mark.gpu

STATE = ('theta', 'inner', 'outer', 'fbias')


@pytest.mark.parametrize('optimizer', ['AdagradOptimizer', 'AdamOptimizer'])
def test_fresh_engine_reproduces_every_state_tensor_from_the_exports(optimizer):
    from cffm_amd.engine import HipEngine
    # P = 6 channels in Pp = 16: ten padded lanes per conv member
    cfg = CFFMConfig(M=50, F=4, K=8, D=8, activation='relu', optimizer=optimizer)
    rng = np.random.default_rng(5)
    eng = HipEngine(cfg, params=init_params(cfg, seed=3))
    assert (int(eng.tl.P), int(eng.tl.Pp)) == (6, 16)
    for _ in range(2):
        ids = torch.from_numpy(rng.integers(0, cfg.M, size=(16, cfg.F)).astype(np.int32)).cuda()
        y = torch.from_numpy(rng.choice([-1.0, 1.0], size=16).astype(np.float32)).cuda()
        eng.train_step(ids, y)
    params, accs, second = eng.export_params(), eng.export_accumulators(), eng.export_second_moments()
    assert (second is not None) == (optimizer == 'AdamOptimizer')
    fresh = HipEngine(cfg, params=init_params(cfg, seed=4))
    fresh.load_params(params, accs, second)
    torch.cuda.synchronize()
    suffixes = ('', '_acc') + (('_acc2',) if second is not None else ())
    for suffix in suffixes:
        for name in STATE:
            a, b = getattr(eng, name + suffix), getattr(fresh, name + suffix)
            assert a.data_ptr() != b.data_ptr()
            assert torch.equal(a.view(torch.int32).cpu(), b.view(torch.int32).cpu()), name + suffix
    # the steps moved what the comparison covers: the state is not the one a fresh engine starts with
    assert not torch.equal(eng.theta_acc.cpu(), torch.full_like(eng.theta_acc, eng.acc0).cpu())
