#!/usr/bin/env python3
"""Generate tests/golden/ks_cases.npz: seeded two-sample pairs (heavy ties, unequal sizes, one-element samples) and
``scipy.stats.ks_2samp(x, t).statistic`` of each, so that tests/test_distdiff.py pins the integer form of the statistic to
scipy's where scipy is absent.  Needs scipy; writes a few KB."""
import os

import numpy as np
from scipy.stats import ks_2samp

HERE = os.path.dirname(os.path.abspath(__file__))


def cases(seed=20240607, count=48):
    rs = np.random.RandomState(seed)
    out = []
    for i in range(count):
        n = int(rs.choice([1, 2, 3, 7, 30, 64, 128]))
        m = int(rs.choice([1, 2, 5, 32, 100, 257]))
        kind = i % 4
        if kind == 0:        # continuous
            x, t = rs.randn(n), rs.randn(m) + 0.3
        elif kind == 1:      # rectified rates: many exact zeros
            x, t = np.maximum(rs.randn(n), 0), np.maximum(rs.randn(m) - 0.2, 0)
        elif kind == 2:      # small integers (a preferred-bandwidth index)
            x, t = rs.randint(0, 8, n).astype(float), rs.randint(0, 8, m).astype(float)
        else:                # one side constant
            x, t = np.full(n, 1.5), rs.randint(0, 3, m).astype(float)
        out.append((x.astype('float32'), t.astype('float32')))
    return out


def main():
    pairs = cases()
    arrays = {}
    stats = []
    for i, (x, t) in enumerate(pairs):
        arrays['x{}'.format(i)] = x
        arrays['t{}'.format(i)] = t
        stats.append(ks_2samp(x.astype('float64'), t.astype('float64')).statistic)
    arrays['statistic'] = np.asarray(stats, dtype='float64')
    np.savez_compressed(os.path.join(HERE, 'ks_cases.npz'), **arrays)
    print('wrote', len(pairs), 'cases')


if __name__ == '__main__':
    main()
