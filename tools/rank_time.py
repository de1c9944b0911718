"""Times HipEngine.topk against torch.topk on the same device tensor, and the share of CFFM.recommend that is the forward.

    python tools/rank_time.py [--out profiles/rank_topk_vs_torch.md]

Device events around blocks of calls after a warm-up, median of the blocks (ms per call).  torch.topk is the yardstick, not the
specification: its order among equal scores is unspecified, so only the VALUES of the two results are compared here (the indices
are checked against numpy in tests/test_gpu_rank.py).  The forward share is score_candidates over the whole recommend() call at
the first shape, frappe-sized model (F 10, K = D = 32) with a vocabulary that holds the candidates."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cffm_amd.engine import HipEngine  # noqa: E402
from cffm_amd.spec import CFFMConfig  # noqa: E402

SHAPES = [(64, 226336, 10), (1, 1048576, 100), (4096, 4082, 10)]


def timed(fn, warmup=3, blocks=7, per_block=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per_block):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / per_block)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    eng = HipEngine(CFFMConfig(M=64, F=3, K=8, D=8), device='cuda:0')          # top-k does not depend on the model
    lines = ['# `HipEngine.topk` (cffm_topk) against `torch.topk`, MI355X', '',
             'ms per call: median (min - max) of 7 blocks of 5 calls after 3 warm-up calls, device events; scores ~ N(0, 1) fp32.', '',
             '| C | N | k | cffm_topk | torch.topk | faster |', '|---|---|---|---|---|---|']
    gen = torch.Generator(device='cuda').manual_seed(1)
    for C, N, k in SHAPES:
        scores = torch.randn((C, N), generator=gen, device='cuda', dtype=torch.float32)
        idx, val, count = eng.topk(scores, k)
        tv, ti = torch.topk(scores, k, dim=1)
        assert torch.equal(val, tv) and bool((count == k).all()), 'the two top-k disagree on the values'
        ours = timed(lambda: eng.topk(scores, k))
        theirs = timed(lambda: torch.topk(scores, k, dim=1))
        lines.append('| %d | %d | %d | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %s |' % (
            (C, N, k) + ours + theirs + ('cffm_topk' if ours[0] < theirs[0] else 'torch.topk',)))
        del scores
    # share of recommend() that is the forward, at the first shape
    from cffm_amd import CFFM as M
    C, N, k = SHAPES[0]
    Mf = N + 1000
    m = M.CFFM(Mf, 0, tempfile.mkdtemp(prefix='cffm_rank_time'), 32, 32, 'square_loss', 1, 256, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer', 0, 0, 0, 10, 1, 0,
               1.0, 1, 1.0, 1, 1.0, 'selu')
    m.build_graph()
    rng = np.random.default_rng(2)
    ctx = rng.integers(0, Mf, size=(C, 10)).astype(np.int32)
    cand = np.arange(N, dtype=np.int32)
    m.recommend(ctx, 1, candidates=cand, k=k)                                   # warm-up: workspace, scratch, code objects
    torch.cuda.synchronize()
    whole = []
    for _ in range(3):
        t0 = time.perf_counter()
        m.recommend(ctx, 1, candidates=cand, k=k)
        whole.append((time.perf_counter() - t0) * 1e3)                         # ends in the device-to-host copy of the result
    dctx, dcand = torch.from_numpy(ctx).cuda(), torch.from_numpy(cand).cuda()
    group = max(1, (1 << 22) // N)

    def forward():
        for c0 in range(0, C, group):
            m.engine.score_candidates(dctx[c0:c0 + group], 1, dcand)
    fwd = timed(forward, warmup=1, blocks=3, per_block=1)
    lines += ['', '## Share of `recommend()` that is the forward', '',
              'C = %d contexts x N = %d candidates, k = %d, F 10, K = D = 32 (selu), score_rows = 2^22 (groups of %d contexts):' % (C, N, k, group),
              '', '* whole call, host clock, median of 3: %.1f ms' % float(np.median(whole)),
              '* `score_candidates` of the same groups, device events, median of 3: %.1f ms (%.0f M pairs/s)' % (fwd[0], C * N / fwd[0] / 1e3),
              '* share: %.1f %%' % (100.0 * fwd[0] / float(np.median(whole)))]
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
