"""Restatements for the Wasserstein distances of the scorer (csrc/ssn_wdist.hip, analyzers/distdiff.py with wasserstein=True),
shared by tests/test_wasserstein.py and tests/test_wasserstein_gpu.py.

The kernel's weighted sum is restated in exact rational arithmetic on the float32 inputs: with the distinct finite values
p_0 < ... < p_K of the pooled sample, wnum = sum_k (p_{k+1} - p_k) |#{x <= p_k} m - #{t <= p_k} n|, the integral of
|F_x - F_t| times n m, so that W1 = wnum / (n m).  `wnum_in_kernel_order` restates the same sum with the kernel's roundings in the kernel's
order of additions (`block_sum_in_order`, shared with tests/swd_cases.py), for equality of bits.  The projection is restated as
the sequential fp64 sum it is defined as."""
from fractions import Fraction

import numpy as np


def w1_exact(x, t):
    """(wnum as a Fraction, n, m) of two samples; the values are taken as float32, non-finite ones are left out."""
    x, t = np.asarray(x, dtype='float32').reshape(-1), np.asarray(t, dtype='float32').reshape(-1)
    xs, ts = np.sort(x[np.isfinite(x)]).astype('float64'), np.sort(t[np.isfinite(t)]).astype('float64')
    n, m = len(xs), len(ts)
    if n == 0 or m == 0:
        return Fraction(0), n, m
    p = np.unique(np.concatenate([xs, ts]))                   # (a value that occurs several times is one point)
    cx = np.searchsorted(xs, p[:-1], side='right').astype(np.int64)
    ct = np.searchsorted(ts, p[:-1], side='right').astype(np.int64)
    w = np.abs(cx * m - ct * n)
    total = Fraction(0)
    for k in range(len(p) - 1):
        total += (Fraction(float(p[k + 1])) - Fraction(float(p[k]))) * int(w[k])
    return total, n, m


def w1_columns(x, t):
    """Per column of x (B, C) against t (T, C): (wnum as a list of Fractions, n, m as int64 arrays)."""
    x, t = np.asarray(x), np.asarray(t)
    got = [w1_exact(x[:, c], t[:, c]) for c in range(x.shape[1])]
    return [g[0] for g in got], np.array([g[1] for g in got], dtype=np.int64), np.array([g[2] for g in got], dtype=np.int64)


def w1_distance(x, t):
    """W1 as a Fraction (None where a side is empty)."""
    wnum, n, m = w1_exact(x, t)
    return wnum / (n * m) if n * m else None


def wnum_bound(exact, n, m):
    """|wnum - exact| of the kernel at most: every term is non-negative, every product and every partial sum carries at most one
    fp64 rounding and there are at most n + m terms."""
    return (int(n) + int(m) + 2) * Fraction(1, 2 ** 52) * exact


def block_sum_in_order(terms):
    """The fp64 sum of terms[0 .. N) in the order of the kernels' ordered block sum (csrc/ssn_sortcol_dev.h), every addition an
    IEEE fp64 addition of numpy: term i belongs to thread i % 256; a thread adds its terms in increasing i, starting from +0; the 64
    lanes of each of the four waves then do v = v + v[lane ^ off] for off = 32, 16, 8, 4, 2, 1; the result is lane 0 of wave 0
    plus lane 0 of the waves 1, 2 and 3 in that order.  An index without a term is passed as +0: the terms are non-negative, and
    +0 added to a non-negative sum leaves its bits."""
    terms = np.asarray(terms, dtype=np.float64)
    assert not (np.signbit(terms).any() or np.isnan(terms).any())
    rounds = np.concatenate([terms, np.zeros(-len(terms) % 256)]).reshape(-1, 256)
    threads = np.zeros(256)
    for r in rounds:                                          # round k: the terms 256 k + thread
        threads = threads + r
    waves = threads.reshape(4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        waves = waves + waves[:, np.arange(64) ^ off]
    return ((waves[0, 0] + waves[1, 0]) + waves[2, 0]) + waves[3, 0]


def wnum_in_kernel_order(x_col, t_col):
    """wnum of one column as ks_w1_columns_kernel computes it, operation by operation (a numpy float64).  The finite values of
    both samples, sorted; pooled index i is x's i-th value for i < n, t's (i - n)-th behind them.  With ix = #{x <= v} and
    it = #{t <= v}, index i has a term only if it is the LAST occurrence of v in the pool (an x value at ix - 1 that t does not
    hold, a t value at it - 1) and v has a successor, the smaller of xs[ix] and ts[it] where those exist:
    fl(((double) next - (double) v) * (double) |ix m - it n|), the difference exact or rounded once as fp64 does, the product
    rounded once.  The terms are summed by `block_sum_in_order`."""
    x, t = np.asarray(x_col, dtype='float32').reshape(-1), np.asarray(t_col, dtype='float32').reshape(-1)
    xs, ts = np.sort(x[np.isfinite(x)]), np.sort(t[np.isfinite(t)])
    n, m = len(xs), len(ts)
    pool = np.concatenate([xs, ts])
    i = np.arange(n + m)
    ix, it = np.searchsorted(xs, pool, side='right'), np.searchsorted(ts, pool, side='right')
    weight = np.abs(ix.astype(np.int64) * m - it.astype(np.int64) * n)
    t_holds = (it > 0) & (np.concatenate([ts, [np.float32(0)]])[it - 1] == pool)       # (read only where it > 0)
    last = np.where(i < n, (i == ix - 1) & ~t_holds, i - n == it - 1)
    inf = np.float32(np.inf)
    nxt = np.minimum(np.concatenate([xs, [inf]])[ix], np.concatenate([ts, [inf]])[it])  # (+inf where a side has no successor)
    has = last & ((ix < n) | (it < m))
    terms = np.zeros(n + m)
    terms[has] = (nxt[has].astype(np.float64) - pool[has].astype(np.float64)) * weight[has].astype(np.float64)
    return block_sum_in_order(terms)


def project_rows(x, theta):
    """float32 (rows, L): acc = 0, then acc = fma(x[r][c], theta[l][c], acc) for c in order, in fp64, rounded to float32 at the
    end.  The product of two floats is exact in fp64, so a multiplication and an addition are the fused operation; the loop runs
    over c and numpy carries all (r, l) at once."""
    x, theta = np.asarray(x, dtype='float32').astype('float64'), np.asarray(theta, dtype='float32').astype('float64')
    acc = np.zeros((x.shape[0], theta.shape[0]))
    with np.errstate(invalid='ignore', over='ignore'):
        for c in range(theta.shape[1]):
            acc = acc + x[:, c, None] * theta[None, :, c]
        return acc.astype('float32')


def lattice(rs, shape):
    """Multiples of 1/8 in [0, 64) as float32: many ties, and every gap, product and partial sum of wnum is exact in fp64."""
    return (rs.randint(0, 512, size=shape) / 8.0).astype('float32')
