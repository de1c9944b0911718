"""Times HipEngine.score_candidates_shared (the sweep with the fixed-field work done once per context) against
HipEngine.score_candidates (the path it can replace) in the same process on the same device.

    python tools/sweep_time.py [--out profiles/sweep_vs_expand.md]

Each shape is a leg that runs in a child process under its own timeout.  The first leg that fails or runs out of time ends the
run: it is recorded in the table, what was gathered so far is written, no further leg is started on the device and the exit status
is 1.  Inside a leg the two paths are timed in interleaved blocks - expand, shared, expand, shared, ... - after a
warm-up call of each: device events around one call per block, median (min - max) of 7 blocks.  The yardstick is the expand path of
the same run, not a number from another box.  The shapes are those of profiles/rank_topk_vs_torch.md, all at F 10, K = D = 32, selu,
with a vocabulary that holds the candidates."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(64, 226336), (1, 1048576), (4096, 4082)]
BLOCKS = 7
LEG_TIMEOUT = 420


def leg(C, N):
    import torch
    from cffm_amd.engine import HipEngine
    from cffm_amd.spec import CFFMConfig
    M = N + 1000
    eng = HipEngine(CFFMConfig(M=M, F=10, K=32, D=32, activation='selu'), params='device', device='cuda:0')
    assert eng.sweep_ok()
    rng = np.random.default_rng(2)
    ctx = torch.from_numpy(rng.integers(0, M, size=(C, 10)).astype(np.int32)).cuda()
    cand = torch.arange(N, dtype=torch.int32, device='cuda')
    paths = {'expand': lambda: eng.score_candidates(ctx, 1, cand), 'shared': lambda: eng.score_candidates_shared(ctx, 1, cand)}
    ref = paths['expand']()                                                    # warm-up: workspace, scratch, code objects
    got = paths['shared']()
    torch.cuda.synchronize()
    scale = float(ref.abs().mean())
    diff = float((got - ref).abs().max())
    del ref, got
    ms = {k: [] for k in paths}
    for _ in range(BLOCKS):
        for k, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
            del out
    return {'C': C, 'N': N, 'ms': ms, 'max_abs_diff': diff, 'mean_abs_score': scale}


def fmt(ms, pairs):
    return '%.1f (%.1f - %.1f) | %.1f' % (float(np.median(ms)), min(ms), max(ms), pairs / float(np.median(ms)) / 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--leg', type=int, default=None, help='internal: run one shape and print its JSON line')
    args = ap.parse_args()
    if args.leg is not None:
        print('LEG ' + json.dumps(leg(*SHAPES[args.leg])))
        return
    lines = ['# `score_candidates_shared` (cffm_score_sweep) against `score_candidates` (expand + cffm_predict), MI355X', '',
             'ms per call: median (min - max) of %d interleaved blocks of one call after one warm-up call of each path, device events; '
             'F 10, K = D = 32 (selu), field 1, M = N + 1000.  Both paths in the same process on the same device.' % BLOCKS, '',
             '| C | N | expand ms | expand M pairs/s | shared ms | shared M pairs/s | shared / expand time | max abs diff (mean abs score) |',
             '|---|---|---|---|---|---|---|---|']
    wins, done, failed = [], [], None
    for i, (C, N) in enumerate(SHAPES):
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', str(i)], capture_output=True, text=True,
                                 timeout=LEG_TIMEOUT)
            row = [ln for ln in out.stdout.splitlines() if ln.startswith('LEG ')]
            if out.returncode != 0 or not row:
                raise RuntimeError('exit status %d: %s' % (out.returncode, out.stderr.strip().splitlines()[-1:] or ''))
        except (subprocess.TimeoutExpired, RuntimeError) as e:
            # a fault, an abort or a hang on the device: nothing more is started on it in this run
            failed = 'C = %d, N = %d' % (C, N)
            lines.append('| %d | %d | leg failed: %s | | | | | |' % (C, N, str(e).replace('|', '/')[:200]))
            break
        r = json.loads(row[0][4:])
        e, s = r['ms']['expand'], r['ms']['shared']
        ratio = float(np.median(s)) / float(np.median(e))
        lines.append('| %d | %d | %s | %s | %.2f | %.2e (%.2e) |' % (C, N, fmt(e, C * N), fmt(s, C * N), ratio, r['max_abs_diff'],
                                                                      r['mean_abs_score']))
        done.append((C, N, ratio, C * N / float(np.median(e)) / 1e3, C * N / float(np.median(s)) / 1e3, r['max_abs_diff'],
                     r['mean_abs_score']))
        if max(s) < min(e):                                                    # the shared path's whole range lies above expand's in pairs/s
            wins.append(N)
    lines += ['', '## Reading', '', 'Produced by `python tools/sweep_time.py --out profiles/sweep_vs_expand.md`, every line of this file.  The '
              'per-kernel split of the same legs under the profiler is kept in `profiles/sweep_kernel_split.md`.', '']
    if failed:
        lines.append('* INCOMPLETE: the leg %s failed or ran out of time; the legs behind it were not started.' % failed)
    if wins:
        lines.append('* The (min - max) range of the shared path lies wholly above expand\'s (in pairs/s) at N in %s.  `SWEEP_MIN_N` of '
                     'cffm_amd/CFFM.py is the smallest of them, N = %d: the smallest MEASURED N whose whole shared range beats expand\'s '
                     'whole range.  No smaller N was measured, so nothing is claimed below it.' % (sorted(wins), min(wins)))
    elif not failed:
        lines.append('* At no shape does the (min - max) range of the shared path lie wholly above expand\'s: `SWEEP_MIN_N` of cffm_amd/CFFM.py '
                     'is None, `sweep=\'auto\'` is `sweep=\'expand\'`, and the kernel stays the opt-in it is.')
    if done:
        lines.append('* The shared path takes %.2f - %.2f of the expand path\'s time (%.1f - %.1f against %.1f - %.1f M pairs/s).  The largest '
                     'difference between the two results is %.1e at a mean |score| of %.0f: rounding, as tests/test_gpu_sweep.py holds both '
                     'to the float64 oracle.' % (min(d[2] for d in done), max(d[2] for d in done), min(d[4] for d in done),
                                                 max(d[4] for d in done), min(d[3] for d in done), max(d[3] for d in done),
                                                 max(d[5] for d in done), float(np.mean([d[6] for d in done]))))
    lines.append('* The default of `recommend` / `evaluate_ranking` stays `sweep=\'expand\'`: this table is one box.')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)
    if failed:
        sys.exit(1)


if __name__ == '__main__':
    main()
