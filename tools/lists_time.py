"""Times the two ways of scoring a candidate list PER CONTEXT (the sampled protocol: every held-out positive against its own drawn
negatives) against the only route there was before them: one HipEngine.score_candidates call per context.

    python tools/lists_time.py [--yardstick-root DIR] [--out profiles/rank_lists.md]

Shape: F 10, K = D = 32 (selu), C = 4096 contexts, N = 100 candidates each, field 1.  Two legs, each a child process under its own
timeout; the first leg that fails or runs out of time ends the run - it is recorded, what was gathered so far is written, no further
leg is started on the device and the exit status is 1.

  * `lists`: score_candidate_tuples (expand + cffm_predict) and score_candidate_lists_shared (cffm_score_sweep_lists), timed in ONE
    process in interleaved blocks - tuples, shared, tuples, shared, ... - after a warm-up call of each: device events around one
    call per block, median (min - max) of 7 blocks.
  * `yardstick`: C calls of score_candidates, one per context with its own list, device events around the whole loop, 5 blocks after a
    warm-up pass.  It uses nothing but what the commit before these entry points has, and --yardstick-root names a built checkout of
    THAT commit to import cffm_amd from, so the yardstick is measured on the parent's code and not on the code under test.  Without
    the option the leg is skipped and the table says so."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_, N_, FIELD = 4096, 100, 1
BLOCKS, YARD_BLOCKS = 7, 5
LEG_TIMEOUT = 300


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
    ctx = torch.from_numpy(rng.integers(0, M, size=(C_, 10)).astype(np.int32)).cuda()
    lists = torch.from_numpy(rng.integers(0, M, size=(C_, N_)).astype(np.int32)).cuda()
    return torch, eng, ctx, lists


def event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    del out
    return a.elapsed_time(b)


def leg_lists(root):
    torch, eng, ctx, lists = setup(root)
    assert eng.sweep_ok()
    tuples = lists.unsqueeze(-1).contiguous()
    paths = {'tuples': lambda: eng.score_candidate_tuples(ctx, [FIELD], tuples),
             'shared': lambda: eng.score_candidate_lists_shared(ctx, FIELD, lists)}
    ref, got = paths['tuples'](), paths['shared']()                           # warm-up: workspace, scratch, code objects
    torch.cuda.synchronize()
    diff, scale = float((got - ref).abs().max()), float(ref.abs().mean())
    del ref, got
    ms = {k: [] for k in paths}
    for _ in range(BLOCKS):
        for k, fn in paths.items():
            ms[k].append(event_ms(torch, fn))
    return {'ms': ms, 'max_abs_diff': diff, 'mean_abs_score': scale}


def leg_yardstick(root):
    torch, eng, ctx, lists = setup(root)

    def sweep():
        return [eng.score_candidates(ctx[c:c + 1], FIELD, lists[c]) for c in range(C_)]
    sweep()
    torch.cuda.synchronize()
    return {'ms': {'per_context': [event_ms(torch, sweep) for _ in range(YARD_BLOCKS)]}}


def fmt(ms):
    med = float(np.median(ms))
    return '%.1f (%.1f - %.1f) | %.2f' % (med, min(ms), max(ms), C_ * N_ / med / 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--yardstick-root', default=None, help='a built checkout of the commit before the per-context entry points')
    ap.add_argument('--leg', default=None, help='internal: run one leg and print its JSON line')
    ap.add_argument('--root', default=ROOT, help='internal: where the leg imports cffm_amd from')
    args = ap.parse_args()
    if args.leg is not None:
        print('LEG ' + json.dumps({'lists': leg_lists, 'yardstick': leg_yardstick}[args.leg](args.root)))
        return
    lines = ['# Candidate lists per context: `score_candidate_tuples` and `score_candidate_lists_shared` against one `score_candidates` '
             'call per context, MI355X', '',
             'C = %d contexts x N = %d candidates each, F 10, K = D = 32 (selu), field %d, M = 20000.  ms per sweep of all C x N pairs: median '
             '(min - max), device events.  The two new paths: %d interleaved blocks of one call in one process after a warm-up call of each.  '
             'The yardstick: %d blocks of C calls after a warm-up pass, in a process of its own that imports the commit before these entry '
             'points.' % (C_, N_, FIELD, BLOCKS, YARD_BLOCKS), '',
             '| path | ms | M pairs/s |', '|---|---|---|']
    legs = [('lists', ROOT)] + ([('yardstick', args.yardstick_root)] if args.yardstick_root else [])
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
            lines.append('| leg `%s` failed: %s | | |' % (name, str(e).replace('|', '/')[:200]))
            break
        res[name] = json.loads(row[0][4:])
    if 'yardstick' in res:
        lines.append('| one `score_candidates` call per context (the commit before) | %s |' % fmt(res['yardstick']['ms']['per_context']))
    if 'lists' in res:
        lines.append('| `score_candidate_tuples` (expand + `cffm_predict`) | %s |' % fmt(res['lists']['ms']['tuples']))
        lines.append('| `score_candidate_lists_shared` (`cffm_score_sweep_lists`) | %s |' % fmt(res['lists']['ms']['shared']))
    lines += ['', '## Reading', '', 'Produced by `python tools/lists_time.py --yardstick-root <parent checkout> --out profiles/rank_lists.md`, '
              'every line of this file.', '']
    if failed:
        lines.append('* INCOMPLETE: the leg `%s` failed or ran out of time; nothing was started after it.' % failed)
    if not args.yardstick_root:
        lines.append('* The yardstick leg was not run (no --yardstick-root): the table holds the two new paths only.')
    if 'lists' in res:
        r = res['lists']
        lines.append('* The two new paths differ by at most %.1e at a mean |score| of %.2g: rounding (the shared sweep sums in another '
                     'order; tests/test_gpu_sweep.py holds it to the float64 oracle).' % (r['max_abs_diff'], r['mean_abs_score']))
    lines.append('* One box.  N = %d lies below `SWEEP_MIN_N`, so `sweep=\'auto\'` does not pick the shared sweep here, and no default '
                 'changes on this table.' % N_)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)
    if failed:
        sys.exit(1)


if __name__ == '__main__':
    main()
