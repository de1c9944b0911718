"""Times cffm_draw_lists_weighted against cffm_draw_lists, and one epoch of CFFM.train_ranking(step='fused', sampler='device') with
negative_weights='popularity' against the same epoch without it.

    python tools/rank_draw_weighted_time.py [--out profiles/rank_draw_weighted_time.md]

--out takes a file of the tool's own, which it overwrites: profiles/rank_draw_weighted.md is written by hand and quotes it.

Shape: the frappe command's (F 10, K = D = 32, selu, M = 5382) on synthetic rows: P = 8192 positives whose tuples at fields (1, 6) run
over U = 4082 distinct pairs, pair u carried by 1 + (its share of the other P - U rows in proportion to 1 / rank^0.75) rows, so that
the counts are long-tailed; 64 lists of 4 per step = 256 rows, 128 steps per epoch.  Two legs, each a child process under its own
`timeout -k 10`, one after the other (one process has the GPU open at a time); the first leg that fails or runs out of time ends
the run - it is recorded, what was gathered so far is written, no further leg is started on the device and the exit status is 1.

  * `draw`: HipEngine.draw_lists_weighted (cdf of 1 / rank^0.75 over the U pairs) and HipEngine.draw_lists at the same
    (G = 8192, m, U), m = 3 and 99, tuples of nf = 2: device events around CALLS calls per block, REPEATS interleaved blocks
    uniform, weighted, uniform, ... in one process; median (min - max) in us per call.
  * `epochs`: both epochs in ONE process, each on a model of its own: one warm-up epoch of each, then REPEATS interleaved repeats of
    one epoch; wall time of the train_ranking call (it ends with the read of the epoch's loss).  Beside them, on the weighted model's
    engine: the one draw call of an epoch (G = 8192, m = 3) and the epoch's 128 fused list steps on its lists, device events around
    each, REPEATS times.  The structural condition: the draw call takes less time than the list steps."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F, K, M, FIELDS = 10, 32, 5382, (1, 6)
P, U, NEG, PER = 8192, 4082, 3, 64
MS = (3, 99)
REPEATS, CALLS = 5, 20
LEG_TIMEOUT = 300


def pairs():
    """U distinct (field 1, field 6) pairs of ids below M, in lexicographic order of (field 1, field 6)."""
    u = np.arange(U)
    return np.stack([u // 58, 71 + u % 58], axis=1).astype(np.int32)            # 71 * 58 = 4118 >= U cells, ids < 71 + 58


def rank_weights():
    return np.arange(1, U + 1, dtype=np.float64) ** -0.75


def split():
    rng = np.random.default_rng(7)
    w = rank_weights()
    extra = rng.choice(U, size=P - U, p=w / w.sum())
    which = rng.permutation(np.concatenate([np.arange(U), extra]))               # every pair at least once, long-tailed counts
    X = rng.integers(0, M, size=(P, F)).astype(np.int32)
    X[:, list(FIELDS)] = pairs()[which]
    return {'X': X.tolist(), 'Y': [1.0] * P}


def events(fn, n):
    import torch
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def leg_draw():
    sys.path.insert(0, ROOT)
    import torch
    from cffm_amd.engine import HipEngine
    from cffm_amd.spec import CFFMConfig, weight_cdf
    eng = HipEngine(CFFMConfig(M=M, F=F, K=K, D=K, activation='selu'), device='cuda:0')
    cand = torch.from_numpy(pairs()).cuda()
    cdf = torch.from_numpy(weight_cdf(rank_weights()).view(np.int32)).cuda()
    at = torch.from_numpy((np.arange(P) * 7 % U).astype(np.int32)).cuda()
    us, short = {}, {}
    for m in MS:
        calls = {'uniform': lambda c, m=m: eng.draw_lists(3, c * P, at, U, m, cand),
                 'weighted': lambda c, m=m: eng.draw_lists_weighted(3, c * P, at, cdf, m, cand)}
        for fn in calls.values():
            for c in range(3):
                fn(c)
        torch.cuda.synchronize()
        short[str(m)] = int((calls['weighted'](0)[2] < 0).sum())
        for name in calls:
            us['%s %d' % (name, m)] = []
        for _ in range(REPEATS):
            for name, fn in calls.items():
                us['%s %d' % (name, m)] += [t / CALLS for t in events(lambda: [fn(c) for c in range(CALLS)], 1)]
    return {'us': us, 'short': short}


def leg_epochs():
    sys.path.insert(0, ROOT)
    import torch
    from cffm_amd import CFFM as C
    data = split()
    tmp = tempfile.mkdtemp()
    kws = {'uniform': {}, 'popularity': {'negative_weights': 'popularity'}}
    models = {s: C.CFFM(M, 0, os.path.join(tmp, s), K, K, 'square_loss', 1, 256, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer', 0, 0, 0,
                        F, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'selu') for s in kws}

    def epoch(s, seed):
        t0 = time.perf_counter()
        means = models[s].train_ranking(data, FIELDS, negatives=NEG, loss='bpr', epochs=1, lists_per_step=PER, seed=seed, step='fused',
                                        sampler='device', **kws[s])
        dt = time.perf_counter() - t0
        if not np.isfinite(means).all():
            raise RuntimeError('%s: the epoch loss is not finite' % s)
        return dt * 1e3

    for s in models:
        epoch(s, 0)
    ms = {s: [] for s in models}
    for r in range(REPEATS):
        for s in models:
            ms[s].append(epoch(s, 1 + r))
    # beside them: the epoch's one draw call and its 128 list steps, on the weighted model's engine
    from cffm_amd.spec import weight_cdf
    eng = models['popularity'].engine
    X = np.asarray(data['X'], dtype=np.int32)
    distinct, inverse, counts = np.unique(X[:, list(FIELDS)], axis=0, return_inverse=True, return_counts=True)
    cand = torch.from_numpy(distinct.astype(np.int32)).cuda()
    cdf = torch.from_numpy(weight_cdf(counts.astype(np.float64) ** 0.75).view(np.int32)).cuda()
    at = torch.from_numpy(inverse.reshape(-1).astype(np.int32)).cuda()
    rows = torch.from_numpy(X).cuda()
    drawn = []

    def draw():
        drawn[:] = [eng.draw_lists_weighted(9, 0, at, cdf, NEG, cand)]

    def steps():
        tuples, _, target = drawn[0]
        for r0 in range(0, P, PER):
            eng.train_step_lists_fused(rows[r0:r0 + PER], list(FIELDS), tuples[r0:r0 + PER], target[r0:r0 + PER], 'bpr')

    draw()
    steps()
    torch.cuda.synchronize()
    return {'ms': ms, 'draw_us': events(draw, REPEATS), 'steps_us': events(steps, REPEATS), 'short': int((drawn[0][2] < 0).sum()),
            'U': int(distinct.shape[0]), 'max_count': int(counts.max())}


def fmt(v):
    return '%.1f (%.1f - %.1f)' % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--leg', default=None, help='internal: run one leg and print its JSON line')
    args = ap.parse_args()
    if args.leg is not None:
        print('LEG ' + json.dumps({'epochs': leg_epochs, 'draw': leg_draw}[args.leg]()))
        return
    lines = ['# The weighted list draw against the uniform one, and one epoch of train_ranking with popularity negatives, MI355X', '',
             'F %d, K = D = %d (selu), M = %d; synthetic rows, P = %d positives over U = %d distinct tuples at fields %s with long-tailed '
             "counts, `step='fused'`, `sampler='device'`, %d lists per step (%d rows, %d steps per epoch)."
             % (F, K, M, P, U, FIELDS, PER, PER * (NEG + 1), P // PER), '']
    failed, res = None, {}
    for name in ('draw', 'epochs'):
        try:
            out = subprocess.run(['timeout', '-k', '10', str(LEG_TIMEOUT), sys.executable, os.path.abspath(__file__), '--leg', name],
                                 capture_output=True, text=True)
            row = [ln for ln in out.stdout.splitlines() if ln.startswith('LEG ')]
            if out.returncode != 0 or not row:
                raise RuntimeError('exit status %d: %s' % (out.returncode, out.stderr.strip().splitlines()[-1:] or ''))
        except RuntimeError as e:
            # a fault, an abort or a hang on the device: nothing more is started on it in this run
            failed = (name, str(e).replace('|', '/')[:200])
            break
        res[name] = json.loads(row[0][4:])
    if 'draw' in res:
        us = res['draw']['us']
        lines += ['| G = %d, tuples of nf = 2 | `draw_lists` us per call | `draw_lists_weighted` us per call | ratio | incomplete lists |' % P,
                  '|---|---|---|---|---|']
        for m in MS:
            a, b = us['uniform %d' % m], us['weighted %d' % m]
            lines.append('| m = %d | %s | %s | %.2f | %d |' % (m, fmt(a), fmt(b), float(np.median(b)) / float(np.median(a)),
                                                              res['draw']['short'][str(m)]))
        lines += ['', '* Weights 1 / rank^0.75 over the %d pairs.  Device events around %d back-to-back calls per block (output allocation and '
                  'launch included), median (min - max) of %d interleaved blocks in one process.' % (U, CALLS, REPEATS), '']
    if 'epochs' in res:
        e = res['epochs']
        ms = e['ms']
        u, p = float(np.median(ms['uniform'])), float(np.median(ms['popularity']))
        d, s = float(np.median(e['draw_us'])), float(np.median(e['steps_us']))
        lines += ['| negatives | ms per epoch, wall | us per list |', '|---|---|---|',
                  '| uniform (`negative_weights=None`) | %s | %.1f |' % (fmt(ms['uniform']), u * 1e3 / P),
                  "| `negative_weights='popularity'` | %s | %.1f |" % (fmt(ms['popularity']), p * 1e3 / P), '',
                  '* Median (min - max) of %d interleaved repeats in one process after one warm-up epoch of each; wall time of the '
                  '`train_ranking` call, which ends with the read of the epoch loss; the weighted epoch also builds the cdf on the host '
                  'and reads the count of incomplete lists once.  Counts up to %d over %d distinct pairs.' % (REPEATS, e['max_count'], e['U']),
                  "* `'popularity'` takes %.2f of the time of the uniform epoch (%.1f ms more per epoch); the min - max ranges %s."
                  % (p / u, p - u, 'do not overlap' if max(ms['uniform']) < min(ms['popularity']) or max(ms['popularity']) < min(ms['uniform'])
                     else 'overlap: the order of the two is not established'), '',
                  '| beside them, device events | us |', '|---|---|',
                  '| the one `draw_lists_weighted` call of an epoch (G = %d, m = %d) | %s |' % (P, NEG, fmt(e['draw_us'])),
                  "| the epoch's %d fused list steps on those lists | %s |" % (P // PER, fmt(e['steps_us'])), '',
                  '* The structural condition - the draw call takes less time than the list steps, the draw is not the epoch again - %s: '
                  'the draw is %.3f of the steps.  %d incomplete lists.' % ('HOLDS' if max(e['draw_us']) < min(e['steps_us']) else 'DOES NOT HOLD',
                                                                           d / s, e['short']), '']
    lines += ['## Reading', '', 'Produced by `python tools/rank_draw_weighted_time.py --out <this file>`, every line of this file.', '']
    if failed:
        lines.append('* INCOMPLETE: the leg `%s` failed or ran out of time (%s); nothing was started after it.' % failed)
    lines.append('* One box, one run.  No default depends on this table: `negative_weights=None` stays the default.  Not measured: other '
                 'U, other skews, m between 3 and 99, evaluation.')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)
    if failed:
        sys.exit(1)


if __name__ == '__main__':
    main()
