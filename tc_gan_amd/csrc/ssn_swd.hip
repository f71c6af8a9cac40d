// Sliced Wasserstein loss of a minibatch and its gradient (networks/sliced_wasserstein.py): the projections of the generated
// rows x and of the truth rows y onto L directions come from ssn_wdist.hip's project_rows_kernel; here every direction's two
// columns are sorted, matched rank by rank, and the coefficients are carried back to the rows.
//
//   match        swd_match_kernel: one workgroup per direction l.  The column px[.][l] becomes 64-bit keys -- high word an
//                order-preserving transform of the float with -0 taken as +0, low word the row index -- so that an integer sort
//                IS the stable sort by value (ties by row); py[.][l] stays floats.  Both are padded to P, the power of two
//                >= max(B, 64), with keys above every finite value, and sorted by one call of bitonic_sort_lds
//                (ssn_sortcol_dev.h).  A value that is not finite is found while loading: the workgroup then writes NaN to
//                loss_l[l] and to coef[.][l] and leaves, the sort never sees it.  Rank i: d = (double) u_i - (double) v_i, the
//                term |d| or d d (rounded on its own), the coefficient sign(d) inv or (2 d) inv scattered to coef[b_i][l].
//                The terms go through the ordered block sum of that header and are divided by B: no atomics, the same bits
//                every launch.
//   backproject  swd_backproject_kernel: gx[b][c] = (float) sum_l coef[b][l] theta[l][c], an fp64 FMA chain over l in order (the
//                products of two floats are exact in fp64).  A workgroup owns 16 rows x 16 columns and stages 64 directions of
//                coef and theta at a time in LDS; coef's rows are padded to 65 words (the 4 rows of a wave's half read one
//                direction: 4 banks), the 16 lanes of a row read one word of coef (a broadcast) and 16 consecutive of theta.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ssn_host.h"
#include "ssn_swd_dev.h"

namespace ssn {

// grid (L); dynamic LDS: P keys of 8 bytes, then P floats: swd_match_body (ssn_swd_dev.h) on direction blockIdx.x
__global__ void __launch_bounds__(256) swd_match_kernel(const float* __restrict__ px, const float* __restrict__ py, int B, int L,
                                                        int P, int power, double inv, float* __restrict__ coef,
                                                        double* __restrict__ loss_l) {
    swd_match_body(px, py, B, L, P, power, inv, coef, loss_l, blockIdx.x);
}

// grid (column tiles, row tiles): swd_backproject_body (ssn_swd_dev.h)
__global__ void __launch_bounds__(256) swd_backproject_kernel(const float* __restrict__ coef, const float* __restrict__ theta,
                                                              int B, int L, int D, float* __restrict__ gx) {
    swd_backproject_body(coef, theta, B, L, D, gx, blockIdx.x * BP_COLS, blockIdx.y, gridDim.y);
}

hipError_t launch_swd_match(const float* px, const float* py, int B, int L, int power, float* coef, double* loss_l, hipStream_t st) {
    if (B == 0 || L == 0) return hipSuccess;
    const int P = sort_slots(B);
    const double inv = 1.0 / ((double)L * (double)B);
    hipLaunchKernelGGL(swd_match_kernel, dim3(L), dim3(256), (size_t)P * (sizeof(unsigned long long) + sizeof(float)), st, px, py, B,
                       L, P, power, inv, coef, loss_l);
    return hipGetLastError();
}

hipError_t launch_swd_backproject(const float* coef, const float* theta, int B, int L, int D, float* gx, hipStream_t st) {
    if (B == 0 || D == 0) return hipSuccess;
    const int tiles = (B + BP_ROWS - 1) / BP_ROWS;
    hipLaunchKernelGGL(swd_backproject_kernel, dim3((D + BP_COLS - 1) / BP_COLS, tiles < 4096 ? tiles : 4096), dim3(256), 0, st, coef,
                       theta, B, L, D, gx);
    return hipGetLastError();
}

}  // namespace ssn
