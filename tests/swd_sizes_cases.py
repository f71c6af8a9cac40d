"""Restatement of the sliced Wasserstein match of two samples of DIFFERENT sizes (csrc/ssn_swd_sizes.hip,
include/ssnode_mi355x_ext.h), shared by tests/test_swd_sizes.py and tests/test_swd_sizes_gpu.py.

For float32 projections px (n, L), py (m, L) and every direction l: the pairs (px[b][l], b) sorted ascending by value, ties by
row (numpy's stable argsort; -0 counts as +0) give u_0 .. u_{n-1} with rows b_i, py[:, l] sorted ascending gives v_0 .. v_{m-1}.
On a quantile axis scaled by n m rank i of x owns [i m, (i + 1) m) and rank j of y owns [j n, (j + 1) n); the cut points of both
divide [0, n m) into at most n + m - 1 segments, each inside one (i, j) with its length w_ij as weight (`coupling`).  With
d_ij = (double) u_i - (double) v_j:

    loss_l = sum_ij w_ij |d_ij|^p / (n m)                        -- `match`: in exact rational arithmetic
    coef[b_i] = (float) ((double) c_i inv), inv = 1 / ((L n) m)  -- c_i = sum_j w_ij sign(d_ij), an integer (p = 1), or the
                                                                    sequential fp64 sum of fl(w_ij (2 d_ij)) over j (p = 2)

`loss_in_kernel_order` restates loss_l with the kernel's roundings in the kernel's order: t_i = the sequential fp64 sum over j of
fl(w_ij |d_ij|) or fl(w_ij fl(d_ij d_ij)), the t_i through `wasserstein_cases.block_sum_in_order` (rank i on thread i % 256), the
sum divided by (double) n (double) m.  A column with a value that is not finite gives NaN for its loss and its coefficients.

`match` takes three deliberate errors (`j_hi_short=True`, `unit_weights=True`, `scatter='rank'`) for the sensitivity test."""
from fractions import Fraction

import numpy as np

import swd_cases as sc
from wasserstein_cases import block_sum_in_order, project_rows


def coupling(n, m, j_hi_short=False, unit_weights=False):
    """(i, j, w) int64 arrays of the segments, ascending in i and, within an i, in j; `first[i]`, `count[i]`: where rank i's
    terms start and how many they are."""
    cuts = np.unique(np.concatenate([np.arange(n + 1, dtype=np.int64) * m, np.arange(m + 1, dtype=np.int64) * n]))
    a, w = cuts[:-1], np.diff(cuts)
    i, j = a // m, a // n
    if j_hi_short:                                            # the deliberate error: every rank stops one truth rank early
        keep = np.concatenate([i[1:] == i[:-1], [False]])
        i, j, w = i[keep], j[keep], w[keep]
    if unit_weights:                                          # the deliberate error: the overlaps are forgotten
        w = np.ones_like(w)
    count = np.bincount(i, minlength=n)
    first = np.concatenate([[0], np.cumsum(count)[:-1]])
    return i, j, w, first, count


def _sum_per_rank_in_order(terms, n, first, count):
    """t[i] = ((0 + terms[first[i]]) + terms[first[i] + 1]) + ...: one fp64 addition of numpy per term, in j order."""
    t = np.zeros(n)
    for k in range(int(count.max()) if n else 0):
        has = np.nonzero(count > k)[0]
        t[has] = t[has] + terms[first[has] + k]
    return t


def _exact_weighted_sum(w, d, power):
    """sum_k w_k |d_k|^power as a Fraction (the d_k are fp64 values, taken exactly)."""
    ratios = [abs(float(v)).as_integer_ratio() for v in d]
    den = max([r[1] for r in ratios] + [1])
    total = sum(int(wk) * (r[0] * (den // r[1])) ** power for wk, r in zip(w, ratios))
    return Fraction(total, den ** power)


def _sorted_columns(px_col, py_col):
    col = px_col + np.float32(0.0)                                # (-0 becomes +0)
    order = np.argsort(col, kind='stable')
    return order, col[order].astype('float64'), np.sort(py_col).astype('float64')


def match(px, py, power, j_hi_short=False, unit_weights=False, scatter='row'):
    """px (n, L), py (m, L) float32 -> (coef (n, L) float32, loss_l: list of L Fractions, None where the direction is not
    finite)."""
    px, py = np.asarray(px, dtype='float32'), np.asarray(py, dtype='float32')
    (n, L), m = px.shape, py.shape[0]
    inv = 1.0 / ((float(L) * float(n)) * float(m))
    i, j, w, first, count = coupling(n, m, j_hi_short, unit_weights)
    wf = w.astype('float64')
    coef = np.empty((n, L), dtype='float32')
    loss_l = []
    for l in range(L):
        if not (np.isfinite(px[:, l]).all() and np.isfinite(py[:, l]).all()):
            coef[:, l] = np.nan
            loss_l.append(None)
            continue
        order, u, v = _sorted_columns(px[:, l], py[:, l])
        d = u[i] - v[j]
        loss_l.append(_exact_weighted_sum(w, d, power) / (n * m))
        if power == 1:
            c = np.bincount(i, weights=wf * np.sign(d), minlength=n)      # (integers below 2^53: exact in any order)
        else:
            c = _sum_per_rank_in_order(wf * (2.0 * d), n, first, count)
        c = (c * inv).astype('float32')
        if scatter == 'row':
            coef[order, l] = c
        else:                                                     # the deliberate error: the coefficient stays at its rank
            coef[:, l] = c
    return coef, loss_l


def loss_in_kernel_order(px_col, py_col, power):
    """loss_l of one direction as the kernel computes it, operation by operation (a numpy float64; NaN where a value is not
    finite)."""
    px, py = np.asarray(px_col, dtype='float32').reshape(-1), np.asarray(py_col, dtype='float32').reshape(-1)
    if not (np.isfinite(px).all() and np.isfinite(py).all()):
        return np.float64('nan')
    n, m = len(px), len(py)
    i, j, w, first, count = coupling(n, m)
    _, u, v = _sorted_columns(px, py)
    d = u[i] - v[j]
    terms = w.astype('float64') * (np.abs(d) if power == 1 else d * d)
    return block_sum_in_order(_sum_per_rank_in_order(terms, n, first, count)) / (np.float64(n) * np.float64(m))


def swd(x, y, theta, power, **errors):
    """The whole chain on float32 x (n, D), y (m, D), theta (L, D): dict(px, py, coef, loss_l (Fractions), loss (float), gx)."""
    px, py = project_rows(x, theta), project_rows(y, theta)
    coef, loss_l = match(px, py, power, **errors)
    loss = float('nan') if any(v is None for v in loss_l) else float(sum(loss_l, Fraction(0)) / len(loss_l))
    return dict(px=px, py=py, coef=coef, loss_l=loss_l, loss=loss, gx=sc.backproject(coef, theta))


def loss_bound(exact, n, m):
    """|loss_l - exact| of the kernel at most: every term is non-negative; a term carries the rounding of its square, of its
    product with the weight, and of the partial sums it passes through -- at most n + m - 1 terms in all, summed first within a
    rank and then over the ranks -- and the result that of the product n m and of the division."""
    return (int(n) + int(m) + 4) * Fraction(1, 2 ** 52) * exact


def generic_inputs(rs, n, m, L, D):
    """`swd_cases.generic_inputs` at max(n, m) rows, cut to x (n, D) and y (m, D): duplicated x rows, x rows present in y, and
    -- with at least two columns and two directions -- a direction along which all projections are equal.  What the cut may have
    removed is put back: with n >= 2 the last x row repeats the first, and one row of x is in y whenever both have two."""
    x, y, theta = sc.generic_inputs(rs, max(n, m), L, D)
    x, y = x[:n].copy(), y[:m].copy()
    if n >= 2:
        x[n - 1] = x[0]
    if n >= 2 and m >= 2:
        y[min(n, m) // 2] = x[min(n, m) // 2]
    return x, y, theta


def lattice_inputs(rs, n, m, L, D):
    """x, y multiples of 1/8 in [0, 64), theta multiples of 1/8 in [-1, 1]: projections multiples of 1/64 below 64 D, so every
    d, d^2 (a multiple of 2^-12), weighted term and partial sum (below n m (128 D)^2, times 2^12 below 2^53) is exact in fp64;
    with n, m and L powers of two so are inv and the divisions.  Checked here."""
    x = (rs.randint(0, 512, size=(n, D)) / 8.0).astype('float32')
    y = (rs.randint(0, 512, size=(m, D)) / 8.0).astype('float32')
    theta = (rs.randint(-8, 9, size=(L, D)) / 8.0).astype('float32')
    for k in (n, m, L):
        assert k & (k - 1) == 0, 'n, m, L powers of two'
    bound = 64 * D
    assert bound * 64 <= 2 ** 24
    assert n * m * (2 * bound * 64) ** 2 < 2 ** 53
    return x, y, theta
