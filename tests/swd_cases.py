"""Restatement of the sliced Wasserstein loss and its gradient (csrc/ssn_swd.hip, networks/sliced_wasserstein.py), shared by
tests/test_swd.py, tests/test_swd_gpu.py and tests/test_swd_train_gpu.py.

For float32 projections px, py (B, L) and every direction l: the pairs (px[b][l], b) sorted ascending by value, ties by row
(numpy's stable argsort; -0 counts as +0), py[:, l] sorted ascending, d_i = (double) u_i - (double) v_i rank by rank,
loss_l = (sum_i |d_i|^p) / B -- here in exact rational arithmetic -- and the coefficient of the row b_i that holds u_i:
(float) (sign(d_i) inv) for p = 1, (float) ((2 d_i) inv) for p = 2 with inv = 1 / (L B), every operation an fp64 operation
numpy performs elementwise as the kernel does.  A column of px or py with a value that is not finite gives NaN for its loss and
its coefficients.  `loss_in_kernel_order` restates loss_l with the kernels' roundings in the kernels' order of additions, for
equality of bits.  The back-projection is the sequential fp64 sum of exact products it is defined as.

`match` takes three deliberate errors (`ties='reversed'`, `drop_last=True`, `scatter='rank'`) for the sensitivity test."""
from fractions import Fraction

import numpy as np

from wasserstein_cases import block_sum_in_order, project_rows


def match(px, py, power, ties='row', drop_last=False, scatter='row'):
    """px, py (B, L) float32 -> (coef (B, L) float32, loss_l: list of L Fractions, None where the direction is not finite)."""
    px, py = np.asarray(px, dtype='float32'), np.asarray(py, dtype='float32')
    B, L = px.shape
    inv = 1.0 / (float(L) * float(B))
    coef = np.empty((B, L), dtype='float32')
    loss_l = []
    for l in range(L):
        if not (np.isfinite(px[:, l]).all() and np.isfinite(py[:, l]).all()):
            coef[:, l] = np.nan
            loss_l.append(None)
            continue
        col = px[:, l] + np.float32(0.0)                          # (-0 becomes +0)
        if ties == 'row':
            order = np.argsort(col, kind='stable')
        else:                                                     # the deliberate error: equal values in descending row order
            order = np.lexsort((-np.arange(B), col))
        d = col[order].astype('float64') - np.sort(py[:, l]).astype('float64')
        used = d[:-1] if drop_last else d
        loss_l.append(sum((abs(Fraction(float(v))) ** power for v in used), Fraction(0)) / B)
        c = (np.sign(d) * inv if power == 1 else (2.0 * d) * inv).astype('float32')
        if scatter == 'row':
            coef[order, l] = c
        else:                                                     # the deliberate error: the coefficient stays at its rank
            coef[:, l] = c
    return coef, loss_l


def loss_in_kernel_order(px_col, py_col, power):
    """loss_l of one direction as the match kernels compute it, operation by operation (a numpy float64; NaN where a value is
    not finite): rank i has the term |d_i| or fl(d_i d_i) with d_i = (double) u_i - (double) v_i, the terms are summed by
    `wasserstein_cases.block_sum_in_order` over the ranks (rank i on thread i % 256) and the sum is divided by B."""
    px, py = np.asarray(px_col, dtype='float32').reshape(-1), np.asarray(py_col, dtype='float32').reshape(-1)
    if not (np.isfinite(px).all() and np.isfinite(py).all()):
        return np.float64('nan')
    col = px + np.float32(0.0)                                    # (-0 becomes +0)
    d = col[np.argsort(col, kind='stable')].astype('float64') - np.sort(py).astype('float64')
    return block_sum_in_order(np.abs(d) if power == 1 else d * d) / np.float64(len(px))


def loss_floats(loss_l):
    """The Fractions of `match` as float64 (NaN where the direction is not finite)."""
    return np.array([np.nan if v is None else float(v) for v in loss_l])


def backproject(coef, theta):
    """float32 (B, D): acc = 0, then acc = fma(coef[b][l], theta[l][c], acc) for l in order, in fp64, rounded to float32 at the end
    (the product of two floats is exact in fp64, so a multiplication and an addition are the fused operation)."""
    coef, theta = np.asarray(coef, dtype='float32').astype('float64'), np.asarray(theta, dtype='float32').astype('float64')
    acc = np.zeros((coef.shape[0], theta.shape[1]))
    with np.errstate(invalid='ignore', over='ignore'):
        for l in range(theta.shape[0]):
            acc = acc + coef[:, l, None] * theta[None, l, :]
        return acc.astype('float32')


def swd(x, y, theta, power, **errors):
    """The whole chain on float32 x, y (B, D), theta (L, D): dict(px, py, coef, loss_l (Fractions), loss (float), gx)."""
    px, py = project_rows(x, theta), project_rows(y, theta)
    coef, loss_l = match(px, py, power, **errors)
    loss = float('nan') if any(v is None for v in loss_l) else float(sum(loss_l, Fraction(0)) / len(loss_l))
    return dict(px=px, py=py, coef=coef, loss_l=loss_l, loss=loss, gx=backproject(coef, theta))


def loss_bound(exact, B):
    """|loss_l - exact| of the kernel at most: every term is non-negative, a product, a partial sum and the division carry at most
    one fp64 rounding each and a term passes through at most B of them (the derivation of `wasserstein_cases.wnum_bound`)."""
    return (int(B) + 2) * Fraction(1, 2 ** 52) * exact


def generic_inputs(rs, B, L, D):
    """float32 x, y (B, D), theta (L, D) with the cases the tie-break and the sign decide: duplicated x rows (a pair and a triple
    at non-adjacent indices), x rows equal to y rows (d = 0 where their ranks meet), and -- with at least two columns and two
    directions -- a direction along which all projections are equal (every rank tied, every d = 0)."""
    x, y = rs.randn(B, D).astype('float32'), (rs.randn(B, D) * 1.5 + 0.25).astype('float32')
    g = rs.randn(L, D)
    theta = (g / np.sqrt((g * g).sum(axis=1, keepdims=True))).astype('float32')
    if B >= 63:
        x[40] = x[5]
        x[20] = x[7]
        x[61] = x[7]
        y[3] = x[11]
        y[50] = x[2]
    elif B == 2:
        x[1] = x[0]
    if B >= 2:
        y[B // 2] = x[B // 2]                                   # one row of x in y whatever the size
    if D >= 2 and L >= 2:
        x[:, 0] = y[:, 0] = 1.5
        theta[L // 2] = 0
        theta[L // 2, 0] = 1
    return x, y, theta


def lattice_inputs(rs, B, L, D):
    """x, y multiples of 1/8 in [0, 64), theta multiples of 1/8 in [-1, 1]: every projection is a multiple of 1/64 below
    2^24 / 64, so float32 holds it; every d^2 is a multiple of 2^-12 and the sum of B of them stays below 2^53 2^-12, so every term
    and partial sum of the loss is exact in fp64; with B a power of two so is the division.  Checked here."""
    x = (rs.randint(0, 512, size=(B, D)) / 8.0).astype('float32')
    y = (rs.randint(0, 512, size=(B, D)) / 8.0).astype('float32')
    theta = (rs.randint(-8, 9, size=(L, D)) / 8.0).astype('float32')
    assert (L * B) & (L * B - 1) == 0, 'the divisions by B and by L B are exact for powers of two'
    bound = 64 * D                                               # |projection| < 64 D, a multiple of 1/64
    assert bound * 64 <= 2 ** 24
    assert B * (2 * bound * 64) ** 2 < 2 ** 53
    return x, y, theta
