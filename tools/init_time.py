"""Time of cffm_init_table_rows against the draw it stands beside, on the same tensors: config 5's per-GPU shard by default,
1.25 M rows x (64 + 64) floats.  Three ways of filling the two tables are timed with HIP events around the call (warm-up
calls first, the median of --reps runs is the figure): the by-global-row kernel, the two normal_ calls of
HipEngine(params='device'), and two zero_ calls (the plain write stream of the same bytes).  Prints one JSON line; --out writes
it to a file as well.  The figures in profiles/init_table_rows.md come from this tool.

    python tools/init_time.py [--rows 1250000] [--dim 64] [--reps 21] [--warmup 5] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cffm_amd.engine import HipEngine  # noqa: E402
from cffm_amd.spec import CFFMConfig  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    us.sort()
    return {'median_us': round(us[len(us) // 2], 2), 'min_us': round(us[0], 2), 'max_us': round(us[-1], 2)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rows', type=int, default=1250000)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    cfg = CFFMConfig(M=args.rows, F=32, K=args.dim, D=args.dim)
    eng = HipEngine(cfg, params='device_rows', seed=2021, table_rows=(3, 8))
    gen = torch.Generator(device=eng.device).manual_seed(2021)

    def torch_draw():                                  # what HipEngine(params='device') does
        eng.inner.normal_(0.0, 0.1, generator=gen)
        eng.outer.normal_(0.0, 0.01, generator=gen)

    def zero():
        eng.inner.zero_()
        eng.outer.zero_()

    nbytes = cfg.M * (cfg.K + cfg.D) * 4
    res = {'rows': cfg.M, 'K': cfg.K, 'D': cfg.D, 'bytes_written': nbytes, 'reps': args.reps, 'warmup': args.warmup,
           'device': torch.cuda.get_device_name(0),
           'cffm_init_table_rows': timed(lambda: eng.init_table_rows(2021, 3, 8), args.reps, args.warmup),
           'torch_normal_x2': timed(torch_draw, args.reps, args.warmup),
           'torch_zero_x2': timed(zero, args.reps, args.warmup)}
    for k in ('cffm_init_table_rows', 'torch_normal_x2', 'torch_zero_x2'):
        res[k]['GB_per_s'] = round(nbytes / res[k]['median_us'] / 1e3, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
    return res


if __name__ == '__main__':
    main()
