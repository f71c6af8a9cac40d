"""Restatement of the sliced Wasserstein match per condition cell (csrc/ssn_swd_cells.hip, include/ssnode_mi355x_ext2.h), shared
by tests/test_swd_cells.py, tests/test_swd_cells_gpu.py and tests/test_cswd_train_gpu.py.

B generated rows carry a cell id in 0 .. C - 1; `cell_layout` groups them (stable argsort, bincount).  Cell c, with its n_c rows
in the order of `cell_rows` and its own m truth rows, is one problem of `swd_sizes_cases.match` per direction -- the sort (ties
by the LOCAL index k), the coupling, the loss as an exact rational -- and `swd_sizes_cases.loss_in_kernel_order` restates its
loss_cl[c][l] operation by operation.  What is the step's own is the scale of the coefficients,

    coef[row_k][l] = (float) ((double) c_i inv),   inv = 1 / ((L B) m)   -- B, not n_c,

the derivative of  swd = sum_c (n_c / B) (1 / L) sum_l loss_cl[c][l].  An empty cell has loss +0 and writes no coefficient.  A
value that is not finite in a cell's segment or truth block gives NaN for that (cell, direction) alone.

`match_cells` takes three deliberate errors for the sensitivity test: `inv_per_cell=True` (inv with n_c for B),
`ties='row'` (ties broken by the global row index and not by k: the same thing unless a cell's rows arrive out of order),
`empty_takes_next=True` (an empty cell is given the segment that starts where the next cell's does: it matches the next
non-empty cell's rows against its own truth)."""
from fractions import Fraction

import numpy as np

import swd_cases as sc
import swd_sizes_cases as zc
from wasserstein_cases import project_rows


def cell_layout(cells, C):
    """cells (B,) ints in 0 .. C - 1 -> (cell_rows (B,) int32: the rows grouped by cell, ascending within a cell; cell_start
    (C + 1,) int32)."""
    cells = np.asarray(cells, dtype=np.int64)
    assert cells.ndim == 1 and (len(cells) == 0 or (0 <= cells.min() and cells.max() < C))
    cell_rows = np.argsort(cells, kind='stable').astype(np.int32)
    cell_start = np.concatenate([[0], np.cumsum(np.bincount(cells, minlength=C))]).astype(np.int32)
    return cell_rows, cell_start


def _coefficients(seg, py_col, power, inv, tie_keys):
    """float32 (n,): the coefficient of every element of the segment `seg` (float32 (n,)), in the segment's order.  The sort is
    by (value with -0 as +0, tie_keys)."""
    n, m = len(seg), len(py_col)
    col = seg + np.float32(0.0)
    order = np.lexsort((tie_keys, col))
    u, v = col[order].astype('float64'), np.sort(py_col).astype('float64')
    i, j, w, first, count = zc.coupling(n, m)
    d = u[i] - v[j]
    wf = w.astype('float64')
    if power == 1:
        c = np.bincount(i, weights=wf * np.sign(d), minlength=n)          # (integers below 2^53: exact in any order)
    else:
        c = zc._sum_per_rank_in_order(wf * (2.0 * d), n, first, count)
    out = np.empty(n, dtype='float32')
    out[order] = (c * inv).astype('float32')
    return out


def match_cells(px, cell_rows, cell_start, py, power, inv_per_cell=False, ties='local', empty_takes_next=False):
    """px (B, L) float32, cell_rows (B,), cell_start (C + 1,), py (C, m, L) float32 -> (coef (B, L) float32 -- zero where no cell
    writes --, loss_cl: C lists of L Fractions, None where the (cell, direction) is not finite)."""
    px, py = np.asarray(px, dtype='float32'), np.asarray(py, dtype='float32')
    (B, L), (C, m) = px.shape, py.shape[:2]
    cell_rows, cell_start = np.asarray(cell_rows), np.asarray(cell_start)
    assert cell_start[0] == 0 and cell_start[C] == B and (np.diff(cell_start) >= 0).all()
    coef = np.zeros((B, L), dtype='float32')
    loss_cl = []
    # (cells in descending order: where the third error makes two cells write a row, the row's own cell writes last)
    for c in reversed(range(C)):
        s0, s1 = int(cell_start[c]), int(cell_start[c + 1])
        if empty_takes_next and s0 == s1:
            later = [k for k in range(c + 1, C) if cell_start[k + 1] > cell_start[k]]
            if later:
                s0, s1 = int(cell_start[later[0]]), int(cell_start[later[0] + 1])
        rows = cell_rows[s0:s1]
        n = len(rows)
        if n == 0:
            loss_cl.append([Fraction(0)] * L)
            continue
        inv = 1.0 / ((float(L) * float(n if inv_per_cell else B)) * float(m))
        _, losses = zc.match(px[rows], py[c], power)
        tie_keys = rows if ties == 'row' else np.arange(n)
        for l in range(L):
            if losses[l] is None:
                coef[rows, l] = np.nan
            else:
                coef[rows, l] = _coefficients(px[rows, l], py[c][:, l], power, inv, tie_keys)
        loss_cl.append(losses)
    return coef, loss_cl[::-1]


def loss_cl_in_kernel_order(px, cell_rows, cell_start, py, power):
    """float64 (C, L): loss_cl as the kernel computes it, operation by operation; +0 for an empty cell."""
    C, _, L = py.shape
    out = np.zeros((C, L))
    for c in range(C):
        rows = cell_rows[cell_start[c]:cell_start[c + 1]]
        if len(rows):
            out[c] = [zc.loss_in_kernel_order(px[rows, l], py[c][:, l], power) for l in range(L)]
    return out


def swd_in_host_order(loss_cl, cell_start):
    """The step's loss from float64 loss_cl (C, L) as `cswd_loss_grad` forms it: per cell the sequential sum over l divided by L,
    then the sequential sum over c ascending of (n_c / B) times that.  -> (swd, per_cell (C,))."""
    loss_cl = np.asarray(loss_cl, dtype=np.float64)
    C, L = loss_cl.shape
    n = np.diff(np.asarray(cell_start)).astype(np.float64)
    B = np.float64(cell_start[C])
    per_cell = np.array([np.cumsum(loss_cl[c])[-1] / np.float64(L) for c in range(C)])
    total = np.float64(0.0)
    for c in range(C):
        total = total + (n[c] / B) * per_cell[c]
    return float(total), per_cell


def swd_cells(x, cells, y, theta, power, **errors):
    """The whole chain on float32 x (B, D), cell ids (B,), y (C, m, D), theta (L, D): dict(px, py, cell_rows, cell_start, coef,
    loss_cl (Fractions), swd (the exact weighted mean of the Fractions, as a float; NaN where one is None), gx)."""
    y = np.asarray(y, dtype='float32')
    C, m, D = y.shape
    L, B = theta.shape[0], len(x)
    cell_rows, cell_start = cell_layout(cells, C)
    px, py = project_rows(x, theta), project_rows(y.reshape(C * m, D), theta).reshape(C, m, L)
    coef, loss_cl = match_cells(px, cell_rows, cell_start, py, power, **errors)
    if any(v is None for row in loss_cl for v in row):
        swd = float('nan')
    else:
        n = np.diff(cell_start)
        swd = float(sum((Fraction(int(n[c]), B * L) * sum(loss_cl[c], Fraction(0)) for c in range(C)), Fraction(0)))
    return dict(px=px, py=py, cell_rows=cell_rows, cell_start=cell_start, coef=coef, loss_cl=loss_cl, swd=swd,
                gx=sc.backproject(coef, theta))


def interleaved_cells(rs, sizes):
    """Cell ids (sum(sizes),) with sizes[c] rows of cell c, shuffled: the rows of the cells interleave."""
    cells = np.repeat(np.arange(len(sizes)), sizes)
    rs.shuffle(cells)
    return cells


def generic_inputs(rs, sizes, m, L, D):
    """x (B, D), cells (B,), y (C, m, D), theta (L, D) float32 with what the tie-break and the sign decide inside every cell that
    is large enough: `swd_sizes_cases.generic_inputs` per cell (duplicated rows, rows of x in y, a direction along which all
    projections are equal -- the same direction in every cell), the cells' rows then interleaved in x."""
    sizes = list(sizes)
    C, B = len(sizes), int(sum(sizes))
    cells = interleaved_cells(rs, sizes)
    x = np.zeros((B, D), dtype='float32')
    y = np.zeros((C, m, D), dtype='float32')
    theta = None
    for c, n in enumerate(sizes):
        xc, yc, th = zc.generic_inputs(rs, n, m, L, D)
        theta = th if theta is None else theta                   # (every cell's tied direction is direction L // 2 along column 0)
        x[cells == c] = xc
        y[c] = yc
    if theta is None:
        theta = zc.generic_inputs(rs, 1, m, L, D)[2]
    return x, cells, y, theta


def lattice_inputs(rs, sizes, m, L, D):
    """`swd_sizes_cases.lattice_inputs` per cell (powers of two), one theta; the cells' rows interleaved.  The whole step's B and
    L are powers of two as well: inv is exact."""
    sizes = list(sizes)
    C, B = len(sizes), int(sum(sizes))
    assert B & (B - 1) == 0
    cells = interleaved_cells(rs, sizes)
    x = np.zeros((B, D), dtype='float32')
    y = np.zeros((C, m, D), dtype='float32')
    theta = zc.lattice_inputs(rs, 1, m, L, D)[2]
    for c, n in enumerate(sizes):
        if n:
            xc, yc, _ = zc.lattice_inputs(rs, n, m, L, D)
            x[cells == c] = xc
            y[c] = yc
    return x, cells, y, theta
