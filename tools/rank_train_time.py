"""Times the list train step (HipEngine.train_step_lists: expand, forward, list loss, cffm_backward_dout on the stage launches, dense and
sparse Adagrad) and the fused list step (HipEngine.train_step_lists_fused: the same step in the launches of the pointwise step) against
the fused pointwise step (HipEngine.train_step) on the same number of rows.

    python tools/rank_train_time.py [--out profiles/rank_train_fused_time.md]

--out takes a file of the tool's own, which it overwrites: profiles/rank_train_fused.md is written by hand and quotes it.

Shape: the frappe command's (F 10, K = D = 32, selu, M = 5382); G = 64 lists of Lg = 4 tuples at fields (1, 6) = 256 rows against
train_step at B = 256.  Two legs, each a child process under its own timeout; the first leg that fails or runs out of time ends the
run - it is recorded, what was gathered so far is written, no further leg is started on the device and the exit status is 1.

  * `steps`: the steps in ONE process in interleaved blocks - lists (bpr), lists (softmax), fused lists (bpr), fused lists (softmax),
    pointwise, ... - after a warm-up of each: device events around STEPS steps per block, median (min - max) of 5 blocks, in us per step.
    The fused list step has to be faster than train_step_lists by more than the min - max spread of the blocks of either: the run says
    so, and its exit status is 1 where it is not.
  * `kernels`: each list step under torch.profiler: launches per step and device time per kernel name over STEPS steps, from which the
    share of the step that is the list-loss kernels and the head kernel (head_bwd_dout_kernel, stage step only) is read.  Kernel time
    only: the gaps between the launches of a step are in the first table and not in this one."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

G_, LG, FIELDS, B_ = 64, 4, (1, 6), 256
BLOCKS, STEPS = 5, 50
LEG_TIMEOUT = 240


def setup():
    sys.path.insert(0, ROOT)
    import torch
    from cffm_amd.engine import HipEngine
    from cffm_amd.spec import CFFMConfig
    M = 5382
    eng = HipEngine(CFFMConfig(M=M, F=10, K=32, D=32, activation='selu'), device='cuda:0')
    rng = np.random.default_rng(3)
    dev = lambda a: torch.from_numpy(a).cuda()
    ctx = dev(rng.integers(0, M, size=(G_, 10)).astype(np.int32))
    cand = dev(rng.integers(0, M, size=(G_, LG, len(FIELDS))).astype(np.int32))
    target = dev(rng.integers(0, LG, size=G_).astype(np.int32))
    ids = dev(rng.integers(0, M, size=(B_, 10)).astype(np.int32))
    y = dev(rng.choice([-1.0, 1.0], size=B_).astype(np.float32))
    paths = {'lists_bpr': lambda: eng.train_step_lists(ctx, list(FIELDS), cand, target, 'bpr'),
             'lists_softmax': lambda: eng.train_step_lists(ctx, list(FIELDS), cand, target, 'softmax'),
             'fused_bpr': lambda: eng.train_step_lists_fused(ctx, list(FIELDS), cand, target, 'bpr'),
             'fused_softmax': lambda: eng.train_step_lists_fused(ctx, list(FIELDS), cand, target, 'softmax'),
             'pointwise': lambda: eng.train_step(ids, y)}
    return torch, paths


def leg_steps():
    torch, paths = setup()
    for fn in paths.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in paths}
    for _ in range(BLOCKS):
        for k, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(STEPS):
                fn()
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3 / STEPS)
    return {'us': us}


def leg_kernels():
    torch, paths = setup()
    from torch.profiler import ProfilerActivity, profile
    out = {}
    for k in ('lists_bpr', 'lists_softmax', 'fused_bpr', 'fused_softmax'):
        for _ in range(5):
            paths[k]()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(STEPS):
                paths[k]()
            torch.cuda.synchronize()
        per, launches = {}, 0
        for ev in prof.key_averages():
            t = float(getattr(ev, 'device_time_total', 0.0) or getattr(ev, 'cuda_time_total', 0.0))
            if t > 0:
                per[ev.key] = per.get(ev.key, 0.0) + t / STEPS
                launches += int(ev.count)
        total = sum(per.values())
        pick = lambda word: sum(v for n, v in per.items() if word in n)
        out[k] = {'total_us': total, 'list_loss_us': pick('list_loss'), 'head_us': pick('head_bwd_dout'), 'kernels': len(per),
                  'launches': launches / STEPS, 'names': sorted(per)}
        if total <= 0 or out[k]['list_loss_us'] <= 0 or (out[k]['head_us'] <= 0) != k.startswith('fused'):
            raise RuntimeError('the profiler reported no device time for the kernels asked for: %r' % sorted(per)[:8])
    return out


def fmt(us):
    return '%.1f (%.1f - %.1f)' % (float(np.median(us)), min(us), max(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--leg', default=None, help='internal: run one leg and print its JSON line')
    args = ap.parse_args()
    if args.leg is not None:
        print('LEG ' + json.dumps({'steps': leg_steps, 'kernels': leg_kernels}[args.leg]()))
        return
    lines = ['# The list train step, staged and fused, against the fused pointwise step, MI355X', '',
             'F 10, K = D = 32 (selu), M = 5382.  `train_step_lists` and `train_step_lists_fused`: G = %d lists of Lg = %d tuples at fields %s '
             '= %d rows; `train_step`: '
             'B = %d.  us per step: median (min - max) of %d interleaved blocks of %d steps in one process, device events, after a warm-up '
             'of each.' % (G_, LG, FIELDS, G_ * LG, B_, BLOCKS, STEPS), '']
    failed, res, slower = None, {}, False
    for name in ('steps', 'kernels'):
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', name], capture_output=True, text=True, timeout=LEG_TIMEOUT)
            row = [ln for ln in out.stdout.splitlines() if ln.startswith('LEG ')]
            if out.returncode != 0 or not row:
                raise RuntimeError('exit status %d: %s' % (out.returncode, out.stderr.strip().splitlines()[-1:] or ''))
        except (subprocess.TimeoutExpired, RuntimeError) as e:
            # a fault, an abort or a hang on the device: nothing more is started on it in this run
            failed = (name, str(e).replace('|', '/')[:200])
            break
        res[name] = json.loads(row[0][4:])
    if 'steps' in res:
        us = res['steps']['us']
        base = float(np.median(us['pointwise']))
        lines += ['| step | us per step | x pointwise |', '|---|---|---|']
        for k, label in (('pointwise', '`train_step` (fused launches)'), ('lists_bpr', '`train_step_lists`, bpr'),
                         ('lists_softmax', '`train_step_lists`, softmax'), ('fused_bpr', '`train_step_lists_fused`, bpr'),
                         ('fused_softmax', '`train_step_lists_fused`, softmax')):
            lines.append('| %s | %s | %.2f |' % (label, fmt(us[k]), float(np.median(us[k])) / base))
        lines.append('')
        for kind in ('bpr', 'softmax'):
            a, b = us['lists_' + kind], us['fused_' + kind]
            gain = float(np.median(a)) - float(np.median(b))
            spread = max(max(a) - min(a), max(b) - min(b))
            good = gain > spread
            slower = slower or not good
            lines.append('* %s: the fused step is %.1f us faster than the stage step (%.2fx); the widest min - max spread of their blocks is '
                         '%.1f us: %s.  It stays %.1f us above `train_step`.'
                         % (kind, gain, float(np.median(a)) / float(np.median(b)), spread,
                            'faster by more than the spread' if good else 'NOT faster by more than the spread', float(np.median(b)) - base))
    if 'kernels' in res:
        lines += ['', '| list step | launches per step | kernel time, us per step | list-loss kernels | head kernel |', '|---|---|---|---|---|']
        for k, r in res['kernels'].items():
            lines.append('| %s | %.0f | %.1f over %d kernels | %.1f us = %.1f %% | %.1f us = %.1f %% |' % (
                k.replace('_', ', ').replace('lists', 'stages'), r['launches'], r['total_us'], r['kernels'], r['list_loss_us'],
                100 * r['list_loss_us'] / r['total_us'], r['head_us'], 100 * r['head_us'] / r['total_us']))
        lines += ['', 'Kernels of the fused step (bpr): ' + ', '.join('`%s`' % n.replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0][:60]
                                                                 for n in res['kernels']['fused_bpr']['names'])]
    lines += ['', '## Reading', '', 'Produced by `python tools/rank_train_time.py --out <this file>`, every line of this file.', '']
    if failed:
        lines.append('* INCOMPLETE: the leg `%s` failed or ran out of time (%s); nothing was started after it.' % failed)
    lines.append('* One box.  `train_step_lists` runs the stage launches of the backward and two separate update calls; '
                 '`train_step_lists_fused` runs the launches of `train_step` plus the id expansion and the two list-loss kernels, its fused '
                 'top reading dL/dout instead of forming it.  No default depends on this table: `train_ranking` takes the stage step '
                 'unless it is asked for `step=\'fused\'` or `\'auto\'`.')
    if 'kernels' in res:
        lines.append('* The second table is kernel time under torch.profiler; the gaps between the launches of a step are in the first '
                     'table only.  Kernel durations recorded under the profiler can add up to more than the event-timed step of the first '
                     'table: read the second table for the shares, the first for the time.')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)
    if failed or slower:
        sys.exit(1)


if __name__ == '__main__':
    main()
