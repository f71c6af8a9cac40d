/*
 * ssnode_mi355x_ext2.h -- C ABI of libssnode_ext2.so, the second companion of libssnode.so (MI355X / gfx950 build).
 *
 * What this library is for: entry points added after the surfaces of libssnode.so AND of its first companion were pinned name
 * by name (each by a literal list in its test), so neither takes a new entry point.  This library is pinned so that it can
 * GROW: its test holds header == clib.EXT2_DECLARED_SYMBOLS == the dynamic symbol table, every name under the prefix ssnx2_ and
 * none shared with the other two libraries -- there is no literal list of names.  The next feature that needs an entry point
 * declares it HERE, adds it to clib.EXT2_DECLARED_SYMBOLS, and breaks no existing test.  The conventions are those of
 * ssnode_mi355x.h: plain C, device pointers of the calling thread's current HIP device, `stream` a hipStream_t passed as void*
 * (NULL = the default stream), asynchronous calls, 0 on success and SSN_ERR_BASE + hipError_t otherwise.  The three libraries
 * share one HIP runtime and therefore device memory and streams.  This library keeps its OWN error string: a refusal of an
 * ssnx2_ entry point is read with ssnx2_last_error().
 */
#ifndef SSNODE_MI355X_EXT2_H
#define SSNODE_MI355X_EXT2_H

#include "ssnode_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 -- counted apart from the other libraries'; goes up when an exported function of THIS library changes its meaning (a new
 * entry point does not change it). */
int ssnx2_abi_version(void);
/* The calling thread's last error of this library ("entry point: why"), empty before the first. */
const char *ssnx2_last_error(void);

/* ---- Sliced Wasserstein match per condition cell (networks/conditional_sliced_wasserstein.py; csrc/ssn_swd_cells.hip) ----
 * px: device [B][L] -- the projections (ssn_project_rows_f32) of all B generated rows onto L directions; the rows of different
 * cells are interleaved.  cell_rows: device int[B] -- the row indices grouped by cell, ascending within a cell.  cell_start:
 * HOST int[C + 1] -- cell c owns cell_rows[cell_start[c] .. cell_start[c + 1]); n_c = cell_start[c + 1] - cell_start[c].  It is
 * read before the call returns (it travels in the kernel arguments).  py: device [C][m][L] -- the projections of the m truth
 * rows of every cell.  coef: device [B][L], loss_cl: device double[C][L].
 *
 * Per (cell c, direction l) the segment's values x_k = px[cell_rows[cell_start[c] + k]][l], k = 0 .. n_c - 1, are matched with
 * py[c][.][l] by the QUANTILE coupling, word for word the match of two samples of sizes n = n_c and m of the first companion
 * library:
 * Sorting.  The pairs (x_k, k) are sorted ascending by value, ties by the LOCAL index k (and hence by row: the rows of a cell
 *   ascend), -0 counted as +0: the key is the ordered float in the high word and k in the low word, padding keys above that of
 *   +inf; py[c][.][l] is sorted ascending: u_0 .. u_{n-1} with local indices k_i, and v_0 .. v_{m-1}.
 * Coupling.  On a quantile axis scaled by n m, x rank i owns [i m, (i + 1) m) and y rank j owns [j n, (j + 1) n).  For
 *   j = j_lo = floor(i m / n) .. j_hi = floor(((i + 1) m - 1) / n) the overlap
 *   w_ij = min((i + 1) m, (j + 1) n) - max(i m, j n) is a positive integer; sum_j w_ij = m.
 * Arithmetic.  d_ij = (double) u_i - (double) v_j; everything below is fp64 without contraction:
 *     p = 1:  t_i = sum_j fl((double) w_ij |d_ij|)          c_i = sum_j w_ij sign(d_ij), a 64-bit integer, sign(0) = 0
 *     p = 2:  t_i = sum_j fl((double) w_ij fl(d_ij d_ij))   c_i = sum_j fl((double) w_ij (2.0 d_ij))
 *   both sums sequentially over j ascending, starting from +0 (each product rounded on its own);
 *     loss_cl[c][l] = S / ((double) n_c (double) m), S the ordered block sum over the t_i (rank i on thread i % 256; per thread
 *                    in index order, lanes 32, 16, ... 1 apart, the four waves in order; no atomics: two calls give the same
 *                    bits): the cell's own W_p^p of direction l.  |loss_cl - exact| <= (n_c + m + 4) 2^-52 exact.
 *     coef[row][l] = (float) ((double) c_i inv), row = cell_rows[cell_start[c] + k_i],
 *                    inv = 1.0 / ((double) L (double) B (double) m), the product formed left to right -- B and NOT n_c: the
 *                    derivative by px[row][l] of the step's loss
 *                        swd = sum_c (n_c / B) (1 / L) sum_l loss_cl[c][l],
 *                    the mean over the generated rows' own conditions of the sliced distance under that condition.
 *   An empty cell (n_c == 0) writes loss_cl[c][.] = +0.0 and nothing else.
 *   A value that is not finite in the cell's px segment or in its py block gives loss_cl[c][l] = NaN and coef[row][l] = NaN for
 *   the rows of that cell (found before the sort); other cells and other directions are not touched by it.
 *   At C == 1 with cell_rows the identity, coef and loss_cl[0] are the bits of the first companion's match of sizes B and m.
 * Geometry.  Grid (L, C), one workgroup of 256 threads per (direction, cell); dynamic LDS 8 P(max_c n_c) + 4 P(m) bytes, P(k)
 *   the power of two >= max(k, 64): at the limits 96 KiB of the 160 KiB of a CU.  A row index outside [0, B) is not written.
 * Refused, each with its own message and before any HIP call: a negative size, C > SSNX2_SWD_MAX_CELLS, cell_start that does
 *   not start at 0, decreases, or does not end at B, a cell of more than SSN_SWD_MAX_BATCH rows (B itself is not limited by the
 *   sort), m > SSNX2_SWD_MAX_TRUTH, L > SSN_W1_MAX_DIRECTIONS, a power other than 1 or 2, m == 0 with a non-empty problem, a
 *   null pointer with a non-empty problem.  B == 0, L == 0 or C == 0 is success and writes nothing. */
#define SSNX2_SWD_MAX_CELLS 256
#define SSNX2_SWD_MAX_TRUTH 16384
int ssnx2_swd_match_cells_f32(const float *px, int B, const int *cell_rows, const int *cell_start, int C, const float *py, int m,
                              int L, int power, float *coef, double *loss_cl, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SSNODE_MI355X_EXT2_H */
