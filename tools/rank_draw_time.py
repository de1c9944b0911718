"""Times one epoch of CFFM.train_ranking(step='fused') with the lists drawn on the host (sampler='host': one RandomState permutation
per positive in a Python loop, the default) and on the device (sampler='device': cffm_draw_lists), and cffm_draw_lists alone.

    python tools/rank_draw_time.py [--out profiles/rank_draw_time.md]

--out takes a file of the tool's own, which it overwrites: profiles/rank_draw.md is written by hand and quotes it.

Shape: the frappe command's (F 10, K = D = 32, selu, M = 5382) on synthetic rows: P = 8192 positives whose tuples at fields (1, 6) run
over U = 4082 distinct pairs, m = 3 negatives, 64 lists of 4 per step = 256 rows, 128 steps per epoch.  Two legs, each a child process
under its own `timeout -k 10`; the first leg that fails or runs out of time ends the run - it is recorded, what was gathered so far is
written, no further leg is started on the device and the exit status is 1.

  * `epochs`: both samplers in ONE process, each on a model of its own: one warm-up epoch of each, then REPEATS interleaved repeats
    host, device, host, ... of one epoch; wall time of the train_ranking call (it ends with the read of the epoch's loss, which waits for
    the device), median (min - max).  The host leg is the default code path, the one every earlier version ran.
  * `draw`: HipEngine.draw_lists alone, device events around CALLS calls per block, median (min - max) of REPEATS blocks, in us per
    call: the whole epoch in one call (G = 8192, what train_ranking issues), and one step's lists (G = 64)."""
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
REPEATS, CALLS = 5, 50
LEG_TIMEOUT = 300


def pairs():
    """U distinct (field 1, field 6) pairs of ids below M."""
    u = np.arange(U)
    return np.stack([u % 71, 71 + u // 71], axis=1).astype(np.int32)            # 71 * 58 = 4118 >= U cells, ids < 71 + 58


def split():
    rng = np.random.default_rng(7)
    X = rng.integers(0, M, size=(P, F)).astype(np.int32)
    X[:, list(FIELDS)] = pairs()[rng.permutation(P) % U]                         # every pair at least twice
    return {'X': X.tolist(), 'Y': [1.0] * P}


def leg_epochs():
    sys.path.insert(0, ROOT)
    from cffm_amd import CFFM as C
    data = split()
    tmp = tempfile.mkdtemp()
    models = {s: C.CFFM(M, 0, os.path.join(tmp, s), K, K, 'square_loss', 1, 256, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer', 0, 0, 0,
                        F, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'selu') for s in ('host', 'device')}

    def epoch(s, seed):
        t0 = time.perf_counter()
        means = models[s].train_ranking(data, FIELDS, negatives=NEG, loss='bpr', epochs=1, lists_per_step=PER, seed=seed, step='fused',
                                        sampler=s)
        dt = time.perf_counter() - t0
        if not np.isfinite(means).all():
            raise RuntimeError('sampler=%s: the epoch loss is not finite' % s)
        return dt * 1e3

    for s in models:
        epoch(s, 0)
    ms = {s: [] for s in models}
    for r in range(REPEATS):
        for s in models:
            ms[s].append(epoch(s, 1 + r))
    return {'ms': ms}


def leg_draw():
    sys.path.insert(0, ROOT)
    import torch
    from cffm_amd.engine import HipEngine
    from cffm_amd.spec import CFFMConfig
    eng = HipEngine(CFFMConfig(M=M, F=F, K=K, D=K, activation='selu'), device='cuda:0')
    cand = torch.from_numpy(pairs()).cuda()
    at = torch.from_numpy((np.arange(P) * 7 % U).astype(np.int32)).cuda()
    us = {}
    for G in (P, PER):
        for _ in range(5):
            eng.draw_lists(3, 0, at[:G], U, NEG, cand)
        torch.cuda.synchronize()
        us[str(G)] = []
        for _ in range(REPEATS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for c in range(CALLS):
                eng.draw_lists(3, c * G, at[:G], U, NEG, cand)
            b.record()
            b.synchronize()
            us[str(G)].append(a.elapsed_time(b) * 1e3 / CALLS)
    return {'us': us}


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
    lines = ['# One epoch of train_ranking with the lists drawn on the host and on the device, MI355X', '',
             'F %d, K = D = %d (selu), M = %d; synthetic rows, P = %d positives over U = %d distinct tuples at fields %s, m = %d negatives, '
             "`step='fused'`, %d lists per step (%d rows, %d steps per epoch)." % (F, K, M, P, U, FIELDS, NEG, PER, PER * (NEG + 1), P // PER), '']
    failed, res = None, {}
    for name in ('epochs', 'draw'):
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
    if 'epochs' in res:
        ms = res['epochs']['ms']
        h, d = float(np.median(ms['host'])), float(np.median(ms['device']))
        lines += ['| sampler | ms per epoch, wall | us per list |', '|---|---|---|',
                  "| `'host'` (default) | %s | %.1f |" % (fmt(ms['host']), h * 1e3 / P),
                  "| `'device'` | %s | %.1f |" % (fmt(ms['device']), d * 1e3 / P), '',
                  '* Median (min - max) of %d interleaved repeats in one process after one warm-up epoch of each; wall time of the '
                  '`train_ranking` call, which ends with the read of the epoch loss.' % REPEATS,
                  "* `'device'` takes %.2f of the time of `'host'` (%.1f ms less per epoch); the min - max ranges %s." % (
                      d / h, h - d, 'do not overlap' if max(ms['device']) < min(ms['host']) or max(ms['host']) < min(ms['device'])
                      else 'OVERLAP: the order of the two is not established'), '']
    if 'draw' in res:
        us = res['draw']['us']
        lines += ['| `HipEngine.draw_lists`, tuples of nf = 2 | us per call, device events | ns per list |', '|---|---|---|']
        for G in (P, PER):
            lines.append('| G = %d | %s | %.1f |' % (G, fmt(us[str(G)]), float(np.median(us[str(G)])) * 1e3 / G))
        lines += ['', '* %d back-to-back calls per block (output allocation and launch included), median (min - max) of %d blocks.' % (CALLS, REPEATS), '']
    lines += ['## Reading', '', 'Produced by `python tools/rank_draw_time.py --out <this file>`, every line of this file.', '']
    if failed:
        lines.append('* INCOMPLETE: the leg `%s` failed or ran out of time (%s); nothing was started after it.' % failed)
    lines.append("* One box, one run.  No default depends on this table: `sampler='host'` stays the default of `train_ranking` and "
                 '`evaluate_ranking_tuples`.  Not measured: the host draw on another CPU, other m, U or lists per step, evaluation.')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)
    if failed:
        sys.exit(1)


if __name__ == '__main__':
    main()
