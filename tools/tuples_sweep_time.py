"""Times the tuple sweep (HipEngine.score_candidate_tuples_shared, cffm_score_sweep_tuples) against the only route tuples of nf > 1 had
before it: HipEngine.score_candidate_tuples (cffm_expand_candidates_ex + cffm_predict on the C * N expanded rows).

    python tools/tuples_sweep_time.py [--yardstick-root DIR] [--out FILE]

Shape: F 10, K = D = 32 (selu), nf = 2 (fields 1 and 6), M = 20000, at four (C, N): 64 x 226,336 and 1 x 1,048,576 and 4096 x 4,082 with
one list for every context, and 4096 x 100 with a list per context.  Two legs, each a child process under its own timeout; the first
leg that fails or runs out of time ends the run - it is recorded, what was gathered so far is written, no further leg is started on
the device and the exit status is 1.

  * `sweep`: score_candidate_tuples_shared of this checkout, in one process.
  * `yardstick`: score_candidate_tuples, in a process of its own that imports cffm_amd from --yardstick-root, a built checkout of the
    commit before the tuple sweep: the yardstick is the parent's code, not the code under test.  Without the option the leg is
    skipped and the table says so.

In each leg: one warm-up call per (C, N), then BLOCKS blocks that walk the four (C, N) in turn (interleaved, so that a drift of the
clocks meets all four alike), device events around every call; the table holds the median (min - max) per (C, N)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = [1, 6]
SIZES = [(64, 226336, False), (1, 1048576, False), (4096, 4082, False), (4096, 100, True)]      # (C, N, a list per context)
BLOCKS = 5
LEG_TIMEOUT = 420


def setup(root):
    sys.path.insert(0, os.path.abspath(root))
    import torch
    import cffm_amd
    from cffm_amd.engine import HipEngine
    from cffm_amd.spec import CFFMConfig
    assert os.path.dirname(os.path.abspath(cffm_amd.__file__)) == os.path.join(os.path.abspath(root), 'cffm_amd'), cffm_amd.__file__
    M = 20000
    eng = HipEngine(CFFMConfig(M=M, F=10, K=32, D=32, activation='selu'), params='device', device='cuda:0')
    rng = np.random.default_rng(2)
    cases = []
    for C, N, per_context in SIZES:
        ctx = torch.from_numpy(rng.integers(0, M, size=(C, 10)).astype(np.int32)).cuda()
        cand = torch.from_numpy(rng.integers(0, M, size=((C, N, 2) if per_context else (N, 2))).astype(np.int32)).cuda()
        cases.append((ctx, cand))
    return torch, eng, cases


def event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    del out
    return a.elapsed_time(b)


def leg(root, method):
    torch, eng, cases = setup(root)
    score = getattr(eng, method)
    sample = []
    for ctx, cand in cases:                                                    # warm-up: workspace, scratch, code objects
        out = score(ctx, FIELDS, cand)
        torch.cuda.synchronize()
        sample.append([float(v) for v in out.reshape(-1)[:64].cpu().numpy()])  # the same inputs in both legs: compared by main()
        del out
    ms = [[] for _ in cases]
    for _ in range(BLOCKS):
        for i, (ctx, cand) in enumerate(cases):
            ms[i].append(event_ms(torch, lambda: score(ctx, FIELDS, cand)))
    return {'ms': ms, 'sample': sample}


def fmt(ms, pairs):
    med = float(np.median(ms))
    return '%.1f (%.1f - %.1f) | %.1f' % (med, min(ms), max(ms), pairs / med / 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--yardstick-root', default=None, help='a built checkout of the commit before the tuple sweep')
    ap.add_argument('--leg', default=None, help='internal: run one leg and print its JSON line')
    ap.add_argument('--root', default=ROOT, help='internal: where the leg imports cffm_amd from')
    args = ap.parse_args()
    methods = {'sweep': 'score_candidate_tuples_shared', 'yardstick': 'score_candidate_tuples'}
    if args.leg is not None:
        print('LEG ' + json.dumps(leg(args.root, methods[args.leg])))
        return
    lines = ['## Timing: `score_candidate_tuples_shared` against `score_candidate_tuples`, MI355X', '',
             'F 10, K = D = 32 (selu), nf = 2 (fields %s), M = 20000.  ms per call: median (min - max) of %d blocks that walk the four (C, N) in '
             'turn, device events, after a warm-up call of each.  The tuple sweep runs in one process; the expand path in a process of its own '
             'that imports the commit before the tuple sweep.' % (FIELDS, BLOCKS), '',
             '| C x N | lists | expand (the commit before): ms | M pairs/s | tuple sweep: ms | M pairs/s | sweep / expand |', '|---|---|---|---|---|---|---|']
    legs = [('sweep', ROOT)] + ([('yardstick', args.yardstick_root)] if args.yardstick_root else [])
    failed, res = None, {}
    for name, root in legs:
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', name, '--root', root], capture_output=True, text=True,
                                 timeout=LEG_TIMEOUT)
            row = [ln for ln in out.stdout.splitlines() if ln.startswith('LEG ')]
            if out.returncode != 0 or not row:
                raise RuntimeError('exit status %d: %s' % (out.returncode, out.stderr.strip().splitlines()[-1:] or ''))
        except (subprocess.TimeoutExpired, RuntimeError) as e:
            # a fault, an abort or a hang on the device: nothing more is started on it in this run
            failed = name
            lines.append('| leg `%s` failed: %s | | | | | | |' % (name, str(e).replace('|', '/')[:200]))
            break
        res[name] = json.loads(row[0][4:])
    for i, (C, N, per_context) in enumerate(SIZES):
        yard = fmt(res['yardstick']['ms'][i], C * N) if 'yardstick' in res else 'not run | '
        new = fmt(res['sweep']['ms'][i], C * N) if 'sweep' in res else 'not run | '
        frac = '%.2f' % (np.median(res['sweep']['ms'][i]) / np.median(res['yardstick']['ms'][i])) if len(res) == 2 else ''
        lines.append('| %d x %d | %s | %s | %s | %s |' % (C, N, 'one per context' if per_context else 'one shared', yard, new, frac))
    lines.append('')
    if failed:
        lines.append('* INCOMPLETE: the leg `%s` failed or ran out of time; nothing was started after it.' % failed)
    if not args.yardstick_root:
        lines.append('* The yardstick leg was not run (no --yardstick-root): the table holds the tuple sweep only.')
    if len(res) == 2:
        a, b = np.asarray(res['sweep']['sample']), np.asarray(res['yardstick']['sample'])
        lines.append('* The first 64 scores of every (C, N) differ between the two paths by at most %.1e at a mean |score| of %.2g: rounding '
                     '(the sweep sums in another order; tests/test_gpu_sweep_tuples.py holds both to the float64 oracle).'
                     % (float(np.abs(a - b).max()), float(np.abs(b).mean())))
    lines.append('* One box, one run.  Nothing is gated on the ratio and no default moves: `sweep=\'auto\'` still sends tuples to expand.')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)
    if failed:
        sys.exit(1)


if __name__ == '__main__':
    main()
