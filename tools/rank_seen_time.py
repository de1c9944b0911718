"""Times ranking without seen items: HipEngine.seen_mask alone, CFFM.recommend(exclude=..., by=...) against the
same call with the equivalent dense host skip= mask (what the commit before offers), CFFM.evaluate_ranking(exclude=...) against the
call without it, the frappe line of bench.py on this commit and the commit before, and the HR@10 / NDCG@10 of the committed frappe
slice with and without exclude.

    python tools/rank_seen_time.py [--yardstick-root DIR] [--out profiles/rank_seen_time.md]

--out takes a file of the tool's own, which it overwrites: profiles/rank_seen.md is written by hand and quotes it.

Shape: the frappe command's (F 10, K = D = 32, selu, M = 5382) on synthetic rows of frappe's proportions: 957 users at column 0,
N = 4082 apps at column 1 with long-tailed counts, a train split of 67000 positive rows (about 70 % of frappe's positives) and
C = 4096 contexts.  Every leg is a child process under its own `timeout -k 10`, one after the other (one process has the GPU open
at a time); the first leg that fails or runs out of time ends the run - it is recorded, what was gathered so far is written, no
further leg is started on the device and the exit status is 1.

  * `mask`: HipEngine.seen_mask at C = 4096, N = 4082 with the train relation, without and with a [C, N] skip to OR in.  Device
    events around CALLS calls per block, REPEATS blocks; median (min - max) in us per call, and the bytes the call writes per second.
  * `recommend`: recommend(contexts, 1, candidates, k = 10, exclude=train, by=0) against recommend(..., skip=dense) with the dense
    boolean [C, N] mask built on the host by numpy from the same rows (timed on its own: the caller of the commit before pays it
    per call) - the two results are checked equal first; wall time of the call (it ends with the copy of the result), REPEATS
    interleaved repeats after a warm-up of each.
  * `evaluate`: evaluate_ranking(split of 4096 positive rows, 1, k = 10) with exclude=train, by=0 and without, REPEATS alternating
    repeats after a warm-up of each; wall time.
  * `slice`: the seeded train() of tests/test_host_cffm.py's configuration (24 epochs, batch 16, RandomState(3)) on
    tests/golden/frappe_slice, then HR@10 / NDCG@10 of its validation and test splits with and without exclude=train, by=0.  A result.
  * `bench` (with --yardstick-root DIR, a built checkout of the commit before): python bench.py --gpus 1 --steps 300 --warmup 30,
    BENCH_RUNS interleaved runs of this commit and of the commit before."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F, K, M = 10, 32, 5382
USERS, N, C, P_TRAIN = 957, 4082, 4096, 67000
USER, FIELD, TOP = 0, 1, 10
REPEATS, CALLS, BENCH_RUNS = 7, 20, 3
LEG_TIMEOUT = 300


def rows(rng, n):
    """n rows of F ids below M: users 0 .. USERS - 1 at column 0, apps 1000 .. 1000 + N - 1 at column 1 with long-tailed counts."""
    w = np.arange(1, N + 1, dtype=np.float64) ** -0.75
    X = rng.integers(0, M, size=(n, F)).astype(np.int32)
    X[:, USER] = rng.integers(0, USERS, size=n)
    X[:, FIELD] = 1000 + rng.choice(N, size=n, p=w / w.sum())
    return X


def splits():
    rng = np.random.default_rng(7)
    train, test = rows(rng, P_TRAIN), rows(rng, C)
    return ({'X': train.tolist(), 'Y': [1.0] * P_TRAIN}, {'X': test.tolist(), 'Y': [1.0] * C}, train, test,
            np.arange(1000, 1000 + N, dtype=np.int32))


def dense_mask(train, ctx):
    """The [C, N] boolean mask a caller of the commit before builds on the host: vectorised numpy, not a Python loop."""
    seen = np.zeros((USERS, N), dtype=bool)
    seen[train[:, USER], train[:, FIELD] - 1000] = True
    return seen[ctx[:, USER]]


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
    from cffm_amd import CFFM as Cm
    m = Cm.CFFM(M, 0, os.path.join(tempfile.mkdtemp(), name), K, K, 'square_loss', 1, 256, 0.05, 0, [1.0, 1.0], 'AdagradOptimizer', 0, 0,
                0, F, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'selu')
    m.build_graph()
    return m


def leg_mask(root):
    sys.path.insert(0, root)
    import torch
    from cffm_amd.engine import HipEngine
    from cffm_amd.spec import CFFMConfig, seen_index, seen_mask
    eng = HipEngine(CFFMConfig(M=M, F=F, K=K, D=K, activation='selu'), device='cuda:0')
    _, _, train, test, _ = splits()
    keys, off, pos = seen_index(train[:, USER], train[:, FIELD] - 1000)
    at = np.searchsorted(keys, test[:, USER])
    row = np.where((at < keys.size) & (keys[np.minimum(at, keys.size - 1)] == test[:, USER]), at, -1).astype(np.int32)
    skip = np.random.default_rng(1).random((C, N)) < 0.1
    d = [torch.from_numpy(a).cuda() for a in (off, pos, row)]
    d_skip = torch.from_numpy(skip).cuda()
    us = {}
    for name, sk, h_sk in (('relation', None, None), ('relation OR a [C, N] skip', d_skip, skip)):
        got = eng.seen_mask(d[0], d[1], d[2], N, skip=sk).cpu().numpy()
        if not np.array_equal(got, seen_mask(off, pos, row, N, h_sk)):
            raise RuntimeError('%s: the mask is not the twin\'s' % name)
        torch.cuda.synchronize()
        us[name] = [x / CALLS for _ in range(REPEATS) for x in events(lambda: [eng.seen_mask(d[0], d[1], d[2], N, skip=sk) for _ in range(CALLS)], 1)]
    return {'us': us, 'nnz': int(pos.size), 'R': int(keys.size), 'seen_per_context': float(got.sum()) / C}


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def leg_recommend(root):
    train_split, _, train, test, cand = splits()
    m = model(root, 'rec')
    mask = dense_mask(train, test)
    paths = {
        'exclude': lambda: m.recommend(test, FIELD, candidates=cand, k=TOP, exclude=train_split, by=USER),
        'dense': lambda: m.recommend(test, FIELD, candidates=cand, k=TOP, skip=dense_mask(train, test)),
        'dense, mask given': lambda: m.recommend(test, FIELD, candidates=cand, k=TOP, skip=mask),
    }
    a, b = paths['exclude'](), paths['dense']()
    if not (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))):
        raise RuntimeError('recommend(exclude=) and recommend(skip=dense) differ')
    ms = {k: [] for k in paths}
    ms['host mask alone'] = []
    for _ in range(REPEATS):
        for k, fn in paths.items():
            ms[k].append(wall(fn)[0])
        ms['host mask alone'].append(wall(lambda: np.ascontiguousarray(dense_mask(train, test)))[0])
    # the share of the relation build (torch.unique over the rows of the split) in the exclude call
    import torch
    eng = m.engine
    seen = m._seen_args('recommend()', train_split, USER, [FIELD])
    d_cand = torch.from_numpy(cand).to(eng.device)

    def build():
        m._seen_relation(seen, [FIELD], d_cand)
        torch.cuda.synchronize()
    build()
    ms['relation build alone'] = [wall(build)[0] for _ in range(REPEATS)]
    return {'ms': ms, 'mask_mb': mask.nbytes / 1e6}


def leg_evaluate(root):
    train_split, test_split, _, _, cand = splits()
    m = model(root, 'eval')
    paths = {'plain': lambda: m.evaluate_ranking(test_split, FIELD, k=TOP, candidates=cand),
             'exclude': lambda: m.evaluate_ranking(test_split, FIELD, k=TOP, candidates=cand, exclude=train_split, by=USER)}
    out = {k: fn() for k, fn in paths.items()}
    ms = {k: [] for k in paths}
    for _ in range(REPEATS):
        for k, fn in paths.items():
            ms[k].append(wall(fn)[0])
    return {'ms': ms, 'metrics': out}


def leg_slice(root):
    sys.path.insert(0, root)
    import contextlib
    import io
    from cffm_amd import CFFM as Cm
    from cffm_amd.LoadData import LoadData
    with contextlib.redirect_stdout(io.StringIO()):
        data = LoadData(os.path.join(root, 'tests', 'golden', 'frappe_slice') + '/', 'frappe', 'square_loss')
    m = Cm.CFFM(data.features_M, 0, os.path.join(tempfile.mkdtemp(), 'slice'), 32, 32, 'square_loss', 24, 16, 0.05, 0, [1.0, 1.0],
                'AdagradOptimizer', 0, 0, 0, 10, 1, 0, 1.0, 1, 1.0, 1, 1.0, 'selu', batch_rng=np.random.RandomState(3))
    m.train(data)
    res = {'epochs': len(m.valid_rmse)}
    for name in ('Validation_data', 'Test_data'):
        split = getattr(data, name)
        res[name] = {'plain': m.evaluate_ranking(split, FIELD, k=TOP),
                     'exclude': m.evaluate_ranking(split, FIELD, k=TOP, exclude=data.Train_data, by=USER),
                     'rows': int((np.asarray(split['Y']) > 0).sum())}
    return res


def leg_bench(root):
    out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '300', '--warmup', '30'], cwd=root,
                         capture_output=True, text=True)
    row = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    if out.returncode != 0 or not row:
        raise RuntimeError('bench.py: exit status %d' % out.returncode)
    r = json.loads(row[-1])
    return {'value': r['value'], 'ms_per_step': r['ms_per_step']}


def fmt(v, spec='%.1f'):
    return (spec + ' (' + spec + ' - ' + spec + ')') % (float(np.median(v)), min(v), max(v))


def apart(a, b):
    return max(a) < min(b) or max(b) < min(a)


LEGS = {'mask': leg_mask, 'recommend': leg_recommend, 'evaluate': leg_evaluate, 'slice': leg_slice, 'bench': leg_bench}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--yardstick-root', default=None, help='a built checkout of the commit before cffm_seen_mask')
    ap.add_argument('--leg', default=None, help='internal: run one leg and print its JSON line')
    ap.add_argument('--root', default=ROOT, help='internal: where the leg imports cffm_amd from')
    args = ap.parse_args()
    if args.leg is not None:
        print('LEG ' + json.dumps(LEGS[args.leg](args.root)))
        return
    lines = ['# Ranking without seen items: `seen_mask`, `exclude=` / `by=`, MI355X', '',
             'F %d, K = D = %d (selu), M = %d; synthetic rows of frappe\'s proportions: %d users at column %d, N = %d apps at column %d '
             '(long-tailed), a train split of %d positive rows, C = %d contexts; k = %d.' % (F, K, M, USERS, USER, N, FIELD, P_TRAIN, C, TOP), '']
    legs = [(n, n, ROOT) for n in ('mask', 'recommend', 'evaluate', 'slice')]
    if args.yardstick_root:
        for i in range(BENCH_RUNS):
            legs += [('bench this %d' % i, 'bench', ROOT), ('bench parent %d' % i, 'bench', os.path.abspath(args.yardstick_root))]
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
    if 'mask' in res:
        r = res['mask']
        lines += ['| `HipEngine.seen_mask`, C = %d, N = %d | us per call | C * N bytes over that call time, GB/s |' % (C, N), '|---|---|---|']
        for k, v in r['us'].items():
            lines.append('| %s | %s | %.0f |' % (k, fmt(v), C * N / float(np.median(v)) / 1e3))
        lines += ['', '* The train relation: R = %d owners, nnz = %d (owner, position) pairs, %.1f seen positions per context on average.  '
                  'Device events around %d back-to-back calls per block (argument checks and launch included), median (min - max) of %d '
                  'blocks; the mask was equal to the numpy twin\'s before the clock started.  The call writes C * N = %.1f MB and, with a '
                  'skip, reads as many.  The last column is derived from the call time, which includes the launch from Python, on an output '
                  'that fits the last-level cache: it is not an HBM rate, and the kernel\'s own duration was not traced.' % (r['R'], r['nnz'], r['seen_per_context'], CALLS, REPEATS, C * N / 1e6), '']
    if 'recommend' in res:
        ms = res['recommend']['ms']
        lines += ['| `recommend`, C = %d contexts, N = %d candidates | ms per call, wall |' % (C, N), '|---|---|',
                  '| `exclude=train, by=%d` | %s |' % (USER, fmt(ms['exclude'])),
                  '| `skip=` the dense host mask, built per call (the commit before) | %s |' % fmt(ms['dense']),
                  '| `skip=` the dense host mask, given | %s |' % fmt(ms['dense, mask given']),
                  '| building the host mask alone (numpy) | %s |' % fmt(ms['host mask alone']),
                  '| building the device relation alone (inside the `exclude` call) | %s |' % fmt(ms['relation build alone']), '',
                  '* exclude / dense built per call = %.3f; the ranges %s.  exclude / dense given = %.3f; the ranges %s.  The dense mask is '
                  '%.1f MB crossing the bus per call.  %d interleaved repeats in one process after a warm-up of each; the two results were '
                  'equal bit for bit before the clock started.'
                  % (float(np.median(ms['exclude'])) / float(np.median(ms['dense'])),
                     'are apart' if apart(ms['exclude'], ms['dense']) else 'overlap: no difference is established',
                     float(np.median(ms['exclude'])) / float(np.median(ms['dense, mask given'])),
                     'are apart' if apart(ms['exclude'], ms['dense, mask given']) else 'overlap: no difference is established',
                     res['recommend']['mask_mb'], REPEATS), '']
    if 'evaluate' in res:
        ms, mt = res['evaluate']['ms'], res['evaluate']['metrics']
        lines += ['| `evaluate_ranking`, %d positive rows, N = %d | ms per call, wall |' % (C, N), '|---|---|',
                  '| without the keywords | %s |' % fmt(ms['plain']), '| `exclude=train, by=%d` | %s |' % (USER, fmt(ms['exclude'])), '',
                  '* exclude / plain = %.3f; the ranges %s.  %d alternating repeats in one process after a warm-up of each.  (The model is '
                  'untrained: HR@%d %.4f / NDCG@%d %.4f without, %.4f / %.4f with - timing material, not a result.)'
                  % (float(np.median(ms['exclude'])) / float(np.median(ms['plain'])),
                     'are apart' if apart(ms['exclude'], ms['plain']) else 'overlap: no difference is established', REPEATS,
                     TOP, mt['plain'][0], TOP, mt['plain'][1], mt['exclude'][0], mt['exclude'][1]), '']
    if 'slice' in res:
        r = res['slice']
        lines += ['| frappe slice after the seeded train() (%d epochs) | rows | HR@%d | NDCG@%d | HR@%d, exclude=train | NDCG@%d, exclude=train |'
                  % (r['epochs'], TOP, TOP, TOP, TOP), '|---|---|---|---|---|---|']
        for name in ('Validation_data', 'Test_data'):
            s = r[name]
            lines.append('| %s | %d | %.6f | %.6f | %.6f | %.6f |' % (name, s['rows'], s['plain'][0], s['plain'][1], s['exclude'][0], s['exclude'][1]))
        lines += ['', '* A result, not a gate: 120 train rows, and one positive row of each evaluated split whose user has another positive '
                  'train app.', '']
    this = [res[k]['value'] for k in sorted(res) if k.startswith('bench this')]
    parent = [res[k]['value'] for k in sorted(res) if k.startswith('bench parent')]
    if this and parent:
        lines += ['| `bench.py --gpus 1 --steps 300 --warmup 30` | examples/s |', '|---|---|',
                  '| this commit | %s; runs %s |' % (fmt(this, '%.0f'), ', '.join('%.0f' % v for v in this)),
                  '| the commit before | %s; runs %s |' % (fmt(parent, '%.0f'), ', '.join('%.0f' % v for v in parent)), '',
                  '* Interleaved runs, this commit first.  this / before = %.4f; the ranges %s.'
                  % (float(np.median(this)) / float(np.median(parent)),
                     'are apart' if apart(this, parent) else 'overlap: no difference is established'), '']
    lines += ['## Reading', '', 'Produced by `python tools/rank_seen_time.py --yardstick-root <parent checkout> --out <this file>`, every line of '
              'this file.', '']
    if failed:
        lines.append('* INCOMPLETE: the leg `%s` failed or ran out of time (%s); nothing was started after it.' % failed)
    if not args.yardstick_root:
        lines.append('* The bench legs on the commit before were not run (no --yardstick-root).')
    lines.append('* One box, one run.  No default depends on this table: `exclude=None` stays the default.  Not measured: other C, N and '
                 'relation densities, tuples, explicit lists with repeats.')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)
    if failed:
        sys.exit(1)


if __name__ == '__main__':
    main()
