"""Compare two directories written by `bench.py --dump-outputs`: every array byte for byte.  Prints the first difference of each array
that differs (index, both values) and exits 1, or '<n> arrays identical' and exits 0.
    python tools/compare_dumps.py DIR_A DIR_B"""
import os
import sys

import numpy as np


def main(a, b):
    names_a, names_b = (sorted(f for f in os.listdir(d) if f.endswith('.npy')) for d in (a, b))
    if names_a != names_b or not names_a:
        print('the two dumps hold different arrays: %s' % sorted(set(names_a) ^ set(names_b)))
        return 1
    bad = 0
    for n in names_a:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        if x.shape != y.shape or x.dtype != y.dtype:
            print('%s: %s %s against %s %s' % (n, x.dtype, x.shape, y.dtype, y.shape))
            bad += 1
        elif x.tobytes() != y.tobytes():
            xa, ya = np.atleast_1d(x), np.atleast_1d(y)
            diff = np.flatnonzero(xa.reshape(-1).view(np.uint8 if xa.dtype.itemsize == 1 else 'u%d' % xa.dtype.itemsize)
                                  != ya.reshape(-1).view(np.uint8 if ya.dtype.itemsize == 1 else 'u%d' % ya.dtype.itemsize))
            i = int(diff[0])
            print('%s: %d of %d elements differ, first at flat index %d: %r against %r' % (n, diff.size, xa.size, i, xa.reshape(-1)[i], ya.reshape(-1)[i]))
            bad += 1
    print('%d arrays identical' % len(names_a) if not bad else '%d of %d arrays differ' % (bad, len(names_a)))
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    raise SystemExit(main(sys.argv[1], sys.argv[2]))
