"""Times cffm_pick_hard against the composition of existing calls it replaces, and one epoch of CFFM.train_ranking(step='fused',
sampler='device') with hard_pool=None, 16 and 64; with --yardstick-root the hard_pool=None epoch also on the commit before.

    python tools/rank_hard_time.py [--yardstick-root DIR] [--out profiles/rank_hard_time.md]

--out takes a file of the tool's own, which it overwrites: profiles/rank_hard.md is written by hand and quotes it.

Shape: the frappe command's (F 10, K = D = 32, selu, M = 5382) on the synthetic rows of tools/rank_draw_weighted_time.py: P = 8192
positives over U = 4082 distinct pairs at fields (1, 6); 64 lists of 4 per step = 256 rows, 128 steps per epoch.  Every leg is a
child process under its own `timeout -k 10`, one after the other (one process has the GPU open at a time); the first leg that fails
or runs out of time ends the run - it is recorded, what was gathered so far is written, no further leg is started on the device and
the exit status is 1.

  * `pick`: HipEngine.pick_hard (tuples of nf = 2, m = 3) and the composition - a skip mask over the positive, HipEngine.topk, the
    slot map from a place vector computed ahead of the clock, a scatter of the positive, a gather of the tuple rows - at G = 64 with
    Lp = 17 and 65 and at G = 8192 with Lp = 17, on scores quantised to 64 values (ties).  The composition's tuples and targets are
    checked equal to the kernel's before anything is timed.  Device events around CALLS calls per block, REPEATS interleaved blocks
    kernel, composition, kernel, ... in one process; median (min - max) in us per call.
  * `epochs`: the three epochs in ONE process, each on a model of its own: one warm-up epoch of each, then REPEATS interleaved repeats
    of one epoch; wall time of the train_ranking call (it ends with the read of the epoch's loss).  Beside them, on the engine of the
    hard_pool model, for p = 16 and 64: the epoch's 128 pool forwards (score_candidate_tuples) and its 128 pick_hard calls, device
    events around each, REPEATS times.  The structural condition: the picks take less time than the pool forwards they follow.
  * `none` (with --yardstick-root DIR, a built checkout of the commit before): the epoch without the keyword, a warm-up and REPEATS
    epochs per child process, PAIRS alternating pairs of processes this commit, the commit before, ..."""
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
POOLS = (16, 64)
PICKS = ((64, 17), (64, 65), (8192, 17))
REPEATS, CALLS, PAIRS = 5, 20, 4
LEG_TIMEOUT = 300


def pairs():
    """U distinct (field 1, field 6) pairs of ids below M, in lexicographic order of (field 1, field 6)."""
    u = np.arange(U)
    return np.stack([u // 58, 71 + u % 58], axis=1).astype(np.int32)            # 71 * 58 = 4118 >= U cells, ids < 71 + 58


def split():
    rng = np.random.default_rng(7)
    w = np.arange(1, U + 1, dtype=np.float64) ** -0.75
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


def model(root, name):
    sys.path.insert(0, root)
    from cffm_amd import CFFM as C
    return C.CFFM(M, 0, os.path.join(tempfile.mkdtemp(), name), K, K, 'square_loss', 1, 256, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer', 0, 0,
                  0, F, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'selu')


def leg_pick(root):
    sys.path.insert(0, root)
    import torch
    from cffm_amd.engine import HipEngine
    from cffm_amd.spec import CFFMConfig, pick_hard
    eng = HipEngine(CFFMConfig(M=M, F=F, K=K, D=K, activation='selu'), device='cuda:0')
    rng = np.random.default_rng(3)
    us, launches = {}, {}
    for G, Lp in PICKS:
        s = (rng.integers(0, 64, size=(G, Lp)) / 8.0 - 4.0).astype(np.float32)
        t = rng.integers(0, Lp, size=G).astype(np.int32)
        pool = rng.integers(0, M, size=(G, Lp, 2)).astype(np.int32)
        d_s, d_t, d_pool = torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(pool).cuda()
        place = torch.from_numpy(pick_hard(3, 0, s, t, NEG)[1]).cuda()           # the place draw: given to the composition for free
        slot = torch.arange(NEG + 1, device='cuda')[None, :]
        t64 = d_t.long()[:, None]

        def kernel():
            return eng.pick_hard(3, 0, d_s, d_t, NEG, tuples=d_pool)

        def composed():
            skip = torch.zeros((G, Lp), dtype=torch.uint8, device='cuda').scatter_(1, t64, 1)
            idx = eng.topk(d_s, NEG, skip)[0].long()
            src = (slot - (slot > place[:, None]).long()).clamp_(max=NEG - 1)
            sel = idx.gather(1, src).scatter_(1, place[:, None], t64)
            return d_pool.gather(1, sel[:, :, None].expand(-1, -1, 2)), None, place

        a, b = kernel(), composed()
        if not (torch.equal(a[0], b[0].to(torch.int32)) and torch.equal(a[2].long(), b[2])):
            raise RuntimeError('G = %d, Lp = %d: the composition does not return what the kernel returns' % (G, Lp))
        for fn in (kernel, composed):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        key = '%d %d' % (G, Lp)
        us['kernel ' + key], us['composed ' + key] = [], []
        for _ in range(REPEATS):
            for name, fn in (('kernel', kernel), ('composed', composed)):
                us['%s %s' % (name, key)] += [x / CALLS for x in events(lambda: [fn() for _ in range(CALLS)], 1)]
    return {'us': us}


def epoch_ms(m, data, seed, **kw):
    t0 = time.perf_counter()
    means = m.train_ranking(data, FIELDS, negatives=NEG, loss='bpr', epochs=1, lists_per_step=PER, seed=seed, step='fused', sampler='device',
                            **kw)
    dt = time.perf_counter() - t0
    if not np.isfinite(means).all():
        raise RuntimeError('the epoch loss is not finite')
    return dt * 1e3


def leg_epochs(root):
    data = split()
    kws = {'none': {}, '16': {'hard_pool': 16}, '64': {'hard_pool': 64}}
    models = {s: model(root, s) for s in kws}
    import torch
    for s in models:
        epoch_ms(models[s], data, 0, **kws[s])
    ms = {s: [] for s in models}
    for r in range(REPEATS):
        for s in models:
            ms[s].append(epoch_ms(models[s], data, 1 + r, **kws[s]))
    # beside them: the epoch's 128 pool forwards and its 128 picks, on the engine of the hard_pool=64 model
    eng = models['64'].engine
    X = np.asarray(data['X'], dtype=np.int32)
    distinct, inverse = np.unique(X[:, list(FIELDS)], axis=0, return_inverse=True)
    cand = torch.from_numpy(distinct.astype(np.int32)).cuda()
    at = torch.from_numpy(inverse.reshape(-1).astype(np.int32)).cuda()
    rows = torch.from_numpy(X).cuda()
    beside = {}
    for p in POOLS:
        pool, _, target = eng.draw_lists(9, 0, at, int(distinct.shape[0]), p, cand)
        scores = []

        def forwards():
            scores[:] = [eng.score_candidate_tuples(rows[r0:r0 + PER], list(FIELDS), pool[r0:r0 + PER]) for r0 in range(0, P, PER)]

        def picks():
            for i, r0 in enumerate(range(0, P, PER)):
                eng.pick_hard(9, r0, scores[i], target[r0:r0 + PER], NEG, tuples=pool[r0:r0 + PER])

        forwards()
        picks()
        torch.cuda.synchronize()
        beside[str(p)] = {'forward_us': events(forwards, REPEATS), 'pick_us': events(picks, REPEATS)}
    return {'ms': ms, 'beside': beside}


def leg_none(root):
    data = split()
    m = model(root, 'none')
    epoch_ms(m, data, 0)
    return {'ms': [epoch_ms(m, data, 1 + r) for r in range(REPEATS)]}


def fmt(v):
    return '%.1f (%.1f - %.1f)' % (float(np.median(v)), min(v), max(v))


def apart(a, b):
    return max(a) < min(b) or max(b) < min(a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--yardstick-root', default=None, help='a built checkout of the commit before cffm_pick_hard')
    ap.add_argument('--leg', default=None, help='internal: run one leg and print its JSON line')
    ap.add_argument('--root', default=ROOT, help='internal: where the leg imports cffm_amd from')
    args = ap.parse_args()
    if args.leg is not None:
        print('LEG ' + json.dumps({'pick': leg_pick, 'epochs': leg_epochs, 'none': leg_none}[args.leg](args.root)))
        return
    lines = ['# `pick_hard` against the composition it replaces, and one epoch of train_ranking with a hard-negative pool, MI355X', '',
             'F %d, K = D = %d (selu), M = %d; synthetic rows, P = %d positives over U = %d distinct tuples at fields %s, '
             "`step='fused'`, `sampler='device'`, %d lists of %d per step (%d rows, %d steps per epoch)."
             % (F, K, M, P, U, FIELDS, PER, NEG + 1, PER * (NEG + 1), P // PER), '']
    legs = [('pick', 'pick', ROOT), ('epochs', 'epochs', ROOT)]
    if args.yardstick_root:
        for i in range(PAIRS):
            legs += [('none this %d' % i, 'none', ROOT), ('none parent %d' % i, 'none', os.path.abspath(args.yardstick_root))]
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
    if 'pick' in res:
        us = res['pick']['us']
        lines += ['| tuples of nf = 2, m = %d | `pick_hard` us per call | the composition, us per call | composition / kernel | ranges |' % NEG,
                  '|---|---|---|---|---|']
        for G, Lp in PICKS:
            a, b = us['kernel %d %d' % (G, Lp)], us['composed %d %d' % (G, Lp)]
            lines.append('| G = %d, Lp = %d | %s | %s | %.2f | %s |' % (G, Lp, fmt(a), fmt(b), float(np.median(b)) / float(np.median(a)),
                                                                      'apart' if apart(a, b) else 'overlap'))
        lines += ['', '* The composition: a zeroed skip mask with the positive scattered in, `HipEngine.topk`, the slot map from a place vector '
                  'computed ahead of the clock (the composition has no place draw of its own), a scatter of the positive, a gather of the tuple '
                  'rows; its tuples and targets were equal to the kernel\'s before the clock started.  Device events around %d back-to-back '
                  'calls per block (output allocation and launch included), median (min - max) of %d interleaved blocks in one process.'
                  % (CALLS, REPEATS), '']
    if 'epochs' in res:
        e = res['epochs']
        ms = e['ms']
        lines += ['| epoch | ms per epoch, wall | us per list |', '|---|---|---|']
        for s, label in (('none', '`hard_pool=None`'), ('16', '`hard_pool=16`'), ('64', '`hard_pool=64`')):
            lines.append('| %s | %s | %.1f |' % (label, fmt(ms[s]), float(np.median(ms[s])) * 1e3 / P))
        lines += ['', '* Median (min - max) of %d interleaved repeats in one process after one warm-up epoch of each; wall time of the '
                  '`train_ranking` call, which ends with the read of the epoch loss.' % REPEATS, '',
                  "| beside them, device events, us per epoch's %d calls | pool forwards | picks | picks / forwards | picks / epoch |" % (P // PER),
                  '|---|---|---|---|---|']
        holds = True
        for p in POOLS:
            b = e['beside'][str(p)]
            f, k = float(np.median(b['forward_us'])), float(np.median(b['pick_us']))
            holds = holds and max(b['pick_us']) < min(b['forward_us'])
            lines.append('| `hard_pool=%d` | %s | %s | %.3f | %.3f |' % (p, fmt(b['forward_us']), fmt(b['pick_us']), k / f,
                                                                     k / (float(np.median(ms[str(p)])) * 1e3)))
        lines += ['', '* The structural condition - the picks take less time than the pool forwards they follow - %s.'
                  % ('HOLDS' if holds else 'DOES NOT HOLD'), '']
    this = [v for i in range(PAIRS) for v in res.get('none this %d' % i, {}).get('ms', [])]
    parent = [v for i in range(PAIRS) for v in res.get('none parent %d' % i, {}).get('ms', [])]
    if this and parent:
        lines += ['| the epoch without the keyword | ms per epoch, wall |', '|---|---|',
                  '| this commit | %s |' % fmt(this), '| the commit before | %s |' % fmt(parent), '',
                  '* %d alternating pairs of child processes, a warm-up epoch and %d epochs each; median (min - max) over all of a side\'s '
                  'epochs.  Per process, this commit: %s; the commit before: %s.  The ranges %s.'
                  % (len(parent) // REPEATS, REPEATS,
                     ', '.join('%.1f' % float(np.median(res[k]['ms'])) for k in sorted(res) if k.startswith('none this')),
                     ', '.join('%.1f' % float(np.median(res[k]['ms'])) for k in sorted(res) if k.startswith('none parent')),
                     'are apart' if apart(this, parent) else 'overlap: no difference is established'), '']
    lines += ['## Reading', '', 'Produced by `python tools/rank_hard_time.py --yardstick-root <parent checkout> --out <this file>`, every line of '
              'this file.', '']
    if failed:
        lines.append('* INCOMPLETE: the leg `%s` failed or ran out of time (%s); nothing was started after it.' % failed)
    if not args.yardstick_root:
        lines.append('* The legs on the commit before were not run (no --yardstick-root).')
    lines.append('* One box, one run.  No default depends on this table: `hard_pool=None` stays the default.  Not measured: other m, nf, '
                 'pools between 16 and 64 or beyond, the weighted pool.')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)
    if failed:
        sys.exit(1)


if __name__ == '__main__':
    main()
