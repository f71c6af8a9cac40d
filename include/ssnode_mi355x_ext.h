/*
 * ssnode_mi355x_ext.h -- C ABI of libssnode_ext.so, the companion of libssnode.so (MI355X / gfx950 build).
 *
 * What this library is for: entry points added after the surface of libssnode.so was pinned at ABI version 1.  The exported
 * symbols of libssnode.so are held to ssnode_mi355x.h name by name, so that library takes no new entry point and widens no
 * refusal; a kernel feature that needs one puts it HERE, under the prefix ssnx_.  The conventions are those of ssnode_mi355x.h:
 * plain C, device pointers of the calling thread's current HIP device, `stream` a hipStream_t passed as void* (NULL = the
 * default stream), asynchronous calls, 0 on success and SSN_ERR_BASE + hipError_t otherwise.  The two libraries share one HIP
 * runtime and therefore device memory and streams: the output of an ssn_ entry point is the input of an ssnx_ one and back.
 * This library keeps its OWN error string: a refusal of an ssnx_ entry point is read with ssnx_last_error(), not with
 * ssn_last_error().
 */
#ifndef SSNODE_MI355X_EXT_H
#define SSNODE_MI355X_EXT_H

#include "ssnode_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 -- counted apart from ssn_abi_version(); goes up when an exported function of THIS library changes its meaning. */
int ssnx_abi_version(void);
/* The calling thread's last error of this library ("entry point: why"), empty before the first. */
const char *ssnx_last_error(void);

/* ---- Sliced Wasserstein match of two samples of different sizes (networks/sliced_wasserstein.py; csrc/ssn_swd_sizes.hip) ----
 * px: device [n][L], py: device [m][L] -- the projections (ssn_project_rows_f32, which takes any number of rows) of n generated
 * rows and of m truth rows onto L directions.  coef: device [n][L], loss_l: device double[L].  The loss of direction l is the
 * p-th power of the Wasserstein-p distance of the two empirical measures, by the QUANTILE coupling; for n == m it is the rank
 * coupling of ssn_swd_match_f32.
 *
 * Sorting.  The pairs (px[b][l], b) are sorted ascending by value, ties by row b, -0 counted as +0 (the key transform of
 *   ssn_swd_match_f32); py[.][l] is sorted ascending: u_0 .. u_{n-1} with rows b_i, and v_0 .. v_{m-1}.
 * Coupling.  On a quantile axis scaled by n m, x rank i owns [i m, (i + 1) m) and y rank j owns [j n, (j + 1) n).  For
 *   j = j_lo = floor(i m / n) .. j_hi = floor(((i + 1) m - 1) / n) the overlap
 *   w_ij = min((i + 1) m, (j + 1) n) - max(i m, j n) is a positive integer; sum_j w_ij = m.
 * Arithmetic.  d_ij = (double) u_i - (double) v_j; everything below is fp64 without contraction:
 *     p = 1:  t_i = sum_j fl((double) w_ij |d_ij|)          c_i = sum_j w_ij sign(d_ij), a 64-bit integer, sign(0) = 0
 *     p = 2:  t_i = sum_j fl((double) w_ij fl(d_ij d_ij))   c_i = sum_j fl((double) w_ij (2.0 d_ij))
 *   both sums sequentially over j ascending, starting from +0;
 *     loss_l[l]    = S / ((double) n (double) m), S the ordered block sum of ssn_swd_match_f32 over the t_i (rank i on thread
 *                    i % 256; per thread in index order, lanes 32, 16, ... 1 apart, the four waves in order; no atomics: two
 *                    calls give the same bits).  All terms are non-negative: |loss_l - exact| <= (n + m + 4) 2^-52 exact.
 *     coef[b_i][l] = (float) ((double) c_i inv), inv = 1.0 / ((double) L (double) n (double) m), the product formed left to
 *                    right: the derivative of (1 / L) sum_l loss_l[l] by px[b_i][l].
 *   A column of px or py that holds a value which is not finite gives loss_l[l] = NaN and coef[.][l] = NaN (found before the
 *   sort); the other directions are not touched by it.
 * Geometry.  One workgroup of 256 threads per direction; dynamic LDS 8 P(n) + 4 P(m) bytes, P(k) the power of two
 *   >= max(k, 64): at the limits 96 KiB of the 160 KiB of a CU.
 * Refused, each with its own message: n > SSN_SWD_MAX_BATCH, m > SSNX_SWD_MAX_TRUTH, L > SSN_W1_MAX_DIRECTIONS, a negative
 *   size, a power other than 1 or 2, a null pointer with a non-empty problem, m == 0 with n > 0 and L > 0 (no measure to
 *   compare with).  n == 0 or L == 0 is success and writes nothing. */
#define SSNX_SWD_MAX_TRUTH 16384
int ssnx_swd_match_sizes_f32(const float *px, int n, const float *py, int m, int L, int power, float *coef, double *loss_l,
                             void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SSNODE_MI355X_EXT_H */
