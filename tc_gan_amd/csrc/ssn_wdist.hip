// Wasserstein distances of a run's checkpoints (analyzers/distdiff.py with wasserstein=True): what ssn_score.hip's KS kernel
// builds -- the column sorted in LDS, the two counts of every pooled point -- summed instead of maximised, and the projections
// of whole tuning-curve rows onto random directions that make the sliced distance a set of such columns.
//
//   KS and W1 per (set, column)       ks_w1_columns_kernel: ks_column_body (ssn_sortcol_dev.h) with its W1 lines -- the integers
//                                     n and num of ks_columns_kernel, and beside the maximum the sum wnum, the integral of
//                                     |F_x - F_t| times n m, so that W1 = wnum / (n m).
//   projections                       project_rows_kernel: out[r][l] = (float) sum_c x[r][c] theta[l][c], the sum an fp64 FMA
//                                     chain in column order (the products of two floats are exact in fp64: it is the sequential
//                                     fp64 sum of exact products).  A workgroup owns 32 directions, stages 128 columns of theta
//                                     and of 32 rows at a time in LDS, and a thread carries 4 rows of one direction.  Theta's
//                                     rows are padded to 129 words (32 directions read one column: 32 banks); the 32 lanes of
//                                     a half read one word of x (a broadcast).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ssn_host.h"
#include "ssn_sortcol_dev.h"
#include "ssn_swd_dev.h"

namespace ssn {

// grid (C, S); dynamic LDS: P floats, P = sort_slots(B): ks_column_body (ssn_sortcol_dev.h) with the W1 sum
__global__ void __launch_bounds__(256) ks_w1_columns_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                            const int* __restrict__ m_of, int B, int C, int T, int P,
                                                            int* __restrict__ n_out, long long* __restrict__ num_out,
                                                            double* __restrict__ wnum_out) {
    extern __shared__ float wdist_lds[];
    ks_column_body<true>(x, t, m_of, B, C, T, P, n_out, num_out, wnum_out, wdist_lds);
}

// grid (direction tiles, row tiles up to a cap): project_rows_body (ssn_swd_dev.h) on one sample
__global__ void __launch_bounds__(256) project_rows_kernel(const float* __restrict__ x, long rows, int ldx, int C,
                                                           const float* __restrict__ theta, int L, float* __restrict__ out) {
    project_rows_body(x, rows, ldx, C, theta, L, out, blockIdx.x * PJ_DIRS, blockIdx.y, gridDim.y);
}

hipError_t launch_ks_w1_columns(const float* x, const float* t, const int* m, int S, int B, int C, int T, int* n_out,
                                long long* num_out, double* wnum_out, hipStream_t st) {
    return launch_ks_kernel(ks_w1_columns_kernel, x, t, m, S, B, C, T, st, n_out, num_out, wnum_out);
}

hipError_t launch_project_rows(const float* x, long rows, int ldx, int C, const float* theta, int L, float* out, hipStream_t st) {
    if (rows == 0 || L == 0) return hipSuccess;
    const long tiles = (rows + PJ_ROWS - 1) / PJ_ROWS;
    const int gy = (int)(tiles < 4096 ? tiles : 4096);
    hipLaunchKernelGGL(project_rows_kernel, dim3((L + PJ_DIRS - 1) / PJ_DIRS, gy), dim3(256), 0, st, x, rows, ldx, C, theta, L, out);
    return hipGetLastError();
}

}  // namespace ssn
