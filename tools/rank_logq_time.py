"""Times cffm_list_loss_logq against cffm_list_loss, and one epoch of CFFM.train_ranking(step='fused', sampler='device',
negative_weights='popularity', loss='softmax') with logq=True against logq=False; with --yardstick-root the logq=False epoch also on
the commit before.

    python tools/rank_logq_time.py [--yardstick-root DIR] [--out profiles/rank_logq_time.md]

--out takes a file of the tool's own, which it overwrites: profiles/rank_logq.md is written by hand and quotes it.

Shape: the frappe command's (F 10, K = D = 32, selu, M = 5382) on the synthetic rows of tools/rank_hard_time.py: P = 8192 positives
over U = 4082 distinct pairs at fields (1, 6), long-tailed counts; 64 lists of 4 per step = 256 rows, 128 steps per epoch.  Every leg
is a child process under its own `timeout -k 10`, one after the other (one process has the GPU open at a time); the first leg that
fails or runs out of time ends the run - it is recorded, what was gathered so far is written, no further leg is started on the device
and the exit status is 1.

  * `loss`: one cffm_list_loss_logq call and one cffm_list_loss(softmax) call (two launches each) on the same scores at G = 64,
    Lg = 4 and at G = 8192, Lg = 100, the table that of the epoch legs' popularity weights.  Device events around CALLS calls per
    block, REPEATS interleaved blocks corrected, uncorrected, ... in one process; median (min - max) in us per call.
  * `epochs`: the two epochs in ONE process, each on a model of its own: one warm-up epoch of each, then REPEATS interleaved repeats
    of one epoch; wall time of the train_ranking call (it ends with the read of the epoch's loss).
  * `plain` (with --yardstick-root DIR, a built checkout of the commit before): the epoch without the keyword, a warm-up and REPEATS
    epochs per child process, PAIRS alternating pairs of processes this commit, the commit before, ..."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from rank_hard_time import F, FIELDS, K, M, NEG, P, PER, U, apart, events, fmt, model, split  # noqa: E402

LOSSES = ((64, 4), (8192, 100))
REPEATS, CALLS, PAIRS = 5, 20, 4
LEG_TIMEOUT = 300
SPREAD = 0.03                # the machine-to-machine spread of the README: the margin of the comparisons with the commit before


def table(data, m):
    from cffm_amd.spec import logq_table, weight_cdf
    counts = np.unique(np.asarray(data['X'], dtype=np.int32)[:, list(FIELDS)], axis=0, return_counts=True)[1]
    return logq_table(weight_cdf(counts.astype(np.float64) ** 0.75), m)


def leg_loss(root):
    sys.path.insert(0, root)
    import torch
    from cffm_amd.engine import HipEngine
    from cffm_amd.spec import CFFMConfig
    eng = HipEngine(CFFMConfig(M=M, F=F, K=K, D=K, activation='selu'), device='cuda:0')
    rng = np.random.default_rng(3)
    data = split()
    us = {}
    for G, Lg in LOSSES:
        corr = torch.from_numpy(table(data, Lg - 1)).cuda()
        s = torch.from_numpy(rng.standard_normal((G, Lg)).astype(np.float32)).cuda()
        t = torch.from_numpy(rng.integers(0, Lg, size=G).astype(np.int32)).cuda()
        lists = torch.from_numpy(rng.integers(0, U, size=(G, Lg)).astype(np.int32)).cuda()

        def corrected():
            return eng.list_loss(s, t, G, Lg, 'softmax', lists=lists, corr=corr)

        def plain():
            return eng.list_loss(s, t, G, Lg, 'softmax')

        if not bool(torch.isfinite(corrected()[0]).all()) or not bool(torch.isfinite(plain()[0]).all()):
            raise RuntimeError('G = %d, Lg = %d: a loss is not finite' % (G, Lg))
        for fn in (corrected, plain):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        key = '%d %d' % (G, Lg)
        us['corrected ' + key], us['plain ' + key] = [], []
        for _ in range(REPEATS):
            for name, fn in (('corrected', corrected), ('plain', plain)):
                us['%s %s' % (name, key)] += [x / CALLS for x in events(lambda: [fn() for _ in range(CALLS)], 1)]
    return {'us': us}


def epoch_ms(m, data, seed, **kw):
    t0 = time.perf_counter()
    means = m.train_ranking(data, FIELDS, negatives=NEG, loss='softmax', epochs=1, lists_per_step=PER, seed=seed, step='fused',
                            sampler='device', negative_weights='popularity', **kw)
    dt = time.perf_counter() - t0
    if not np.isfinite(means).all():
        raise RuntimeError('the epoch loss is not finite')
    return dt * 1e3


def leg_epochs(root):
    data = split()
    kws = {'logq': {'logq': True}, 'plain': {'logq': False}}
    models = {s: model(root, s) for s in kws}
    for s in models:
        epoch_ms(models[s], data, 0, **kws[s])
    ms = {s: [] for s in models}
    for r in range(REPEATS):
        for s in models:
            ms[s].append(epoch_ms(models[s], data, 1 + r, **kws[s]))
    return {'ms': ms}


def leg_plain(root):
    data = split()
    m = model(root, 'plain')
    epoch_ms(m, data, 0)
    return {'ms': [epoch_ms(m, data, 1 + r) for r in range(REPEATS)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--yardstick-root', default=None, help='a built checkout of the commit before cffm_list_loss_logq')
    ap.add_argument('--leg', default=None, help='internal: run one leg and print its JSON line')
    ap.add_argument('--root', default=ROOT, help='internal: where the leg imports cffm_amd from')
    args = ap.parse_args()
    if args.leg is not None:
        print('LEG ' + json.dumps({'loss': leg_loss, 'epochs': leg_epochs, 'plain': leg_plain}[args.leg](args.root)))
        return
    lines = ['# `cffm_list_loss_logq` against `cffm_list_loss`, and one epoch of train_ranking with and without logq, MI355X', '',
             'F %d, K = D = %d (selu), M = %d; synthetic rows, P = %d positives over U = %d distinct tuples at fields %s, '
             "`step='fused'`, `sampler='device'`, `negative_weights='popularity'`, `loss='softmax'`, %d lists of %d per step (%d rows, "
             '%d steps per epoch).' % (F, K, M, P, U, FIELDS, PER, NEG + 1, PER * (NEG + 1), P // PER), '']
    legs = [('loss', 'loss', ROOT), ('epochs', 'epochs', ROOT)]
    if args.yardstick_root:
        for i in range(PAIRS):
            legs += [('plain this %d' % i, 'plain', ROOT), ('plain parent %d' % i, 'plain', os.path.abspath(args.yardstick_root))]
    failed, res = None, {}
    for name, leg, root in legs:
        try:
            out = subprocess.run(['timeout', '-k', '10', str(LEG_TIMEOUT), sys.executable, os.path.abspath(__file__), '--leg', leg,
                                  '--root', root], capture_output=True, text=True)
            row = [ln for ln in out.stdout.splitlines() if ln.startswith('LEG ')]
            if out.returncode != 0 or not row:
                raise RuntimeError('exit status %d: %s' % (out.returncode, out.stderr.strip().splitlines()[-1:] or ''))
        except RuntimeError as e:
            # a fault, an abort or a hang on the device: nothing more is started on it in this run
            failed = (name, str(e).replace('|', '/')[:200])
            break
        res[name] = json.loads(row[0][4:])
        print('leg `%s` done' % name, file=sys.stderr, flush=True)
    if 'loss' in res:
        us = res['loss']['us']
        lines += ['| softmax, one call (two launches) | `cffm_list_loss_logq` us | `cffm_list_loss` us | corrected / uncorrected | ranges |',
                  '|---|---|---|---|---|']
        for G, Lg in LOSSES:
            a, b = us['corrected %d %d' % (G, Lg)], us['plain %d %d' % (G, Lg)]
            lines.append('| G = %d, Lg = %d | %s | %s | %.2f | %s |' % (G, Lg, fmt(a), fmt(b), float(np.median(a)) / float(np.median(b)),
                                                                      'apart' if apart(a, b) else 'overlap'))
        lines += ['', '* `HipEngine.list_loss` with and without `lists` / `corr` on the same scores; device events around %d back-to-back '
                  'calls per block (output allocation and launch included), median (min - max) of %d interleaved blocks in one process.'
                  % (CALLS, REPEATS), '']
    if 'epochs' in res:
        ms = res['epochs']['ms']
        lines += ['| epoch | ms per epoch, wall | us per list |', '|---|---|---|']
        for s, label in (('logq', '`logq=True`'), ('plain', '`logq=False`')):
            lines.append('| %s | %s | %.1f |' % (label, fmt(ms[s]), float(np.median(ms[s])) * 1e3 / P))
        ratio = float(np.median(ms['logq'])) / float(np.median(ms['plain']))
        lines += ['', '* Median (min - max) of %d interleaved repeats in one process after one warm-up epoch of each; wall time of the '
                  '`train_ranking` call, which ends with the read of the epoch loss; the corrected epoch also builds the table on the host. '
                  'Corrected / uncorrected %.3f: %s the %.0f %% margin.'
                  % (REPEATS, ratio, 'within' if ratio <= 1.0 + SPREAD else 'BEYOND', 100 * SPREAD), '']
    this = [v for i in range(PAIRS) for v in res.get('plain this %d' % i, {}).get('ms', [])]
    parent = [v for i in range(PAIRS) for v in res.get('plain parent %d' % i, {}).get('ms', [])]
    if this and parent:
        ratio = float(np.median(this)) / float(np.median(parent))
        lines += ['| the epoch without the keyword | ms per epoch, wall |', '|---|---|',
                  '| this commit | %s |' % fmt(this), '| the commit before | %s |' % fmt(parent), '',
                  '* %d alternating pairs of child processes, a warm-up epoch and %d epochs each; median (min - max) over all of a side\'s '
                  'epochs.  Per process, this commit: %s; the commit before: %s.  This commit / the commit before %.3f: %s the %.0f %% '
                  'margin; the ranges %s.'
                  % (len(parent) // REPEATS, REPEATS,
                     ', '.join('%.1f' % float(np.median(res[k]['ms'])) for k in sorted(res) if k.startswith('plain this')),
                     ', '.join('%.1f' % float(np.median(res[k]['ms'])) for k in sorted(res) if k.startswith('plain parent')),
                     ratio, 'within' if ratio <= 1.0 + SPREAD else 'BEYOND', 100 * SPREAD,
                     'are apart' if apart(this, parent) else 'overlap: no difference is established'), '']
    lines += ['## Reading', '', 'Produced by `python tools/rank_logq_time.py --yardstick-root <parent checkout> --out <this file>`, every line of '
              'this file.', '']
    if failed:
        lines.append('* INCOMPLETE: the leg `%s` failed or ran out of time (%s); nothing was started after it.' % failed)
    if not args.yardstick_root:
        lines.append('* The legs on the commit before were not run (no --yardstick-root).')
    lines.append('* One box, one run.  No default depends on this table: `logq=False` stays the default.  Not measured: other m, U or '
                 'lists per step, the stage route, the uniform table.')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)
    if failed:
        sys.exit(1)


if __name__ == '__main__':
    main()
