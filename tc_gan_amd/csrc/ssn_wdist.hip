// Wasserstein distances of a run's checkpoints (analyzers/distdiff.py with wasserstein=True): what ssn_score.hip's KS kernel
// builds -- the column sorted in LDS, the two counts of every pooled point -- summed instead of maximised, and the projections
// of whole tuning-curve rows onto random directions that make the sliced distance a set of such columns.
//
//   KS and W1 per (set, column)       ks_w1_columns_kernel: ks_columns_kernel's load, sort and walk (the same integers n and
//                                     num), and beside the maximum the sum
//                                         wnum = sum_k (p_{k+1} - p_k) |#{x <= p_k} m - #{t <= p_k} n|
//                                     over the distinct finite pooled values p_0 < ... < p_K: the integral of |F_x - F_t| times
//                                     n m, so that W1 = wnum / (n m).  The owner of pooled element i adds the term of its value
//                                     only if i is the value's LAST occurrence in the pool (x first, then t): a value of x at
//                                     i = #{x <= v} - 1 that t does not hold, a value of t at #{t <= v} - 1.  The successor is
//                                     the smaller of sx[#{x <= v}] and t[#{t <= v}] where those exist; the largest pooled value
//                                     has none and adds nothing.  gap and weight are formed in fp64 (the weight is an integer
//                                     below 2^53), their product is rounded once, a thread sums its terms in index order, a
//                                     wave adds lanes 32, 16, ... 1 apart, thread 0 adds the four waves in order: no atomics,
//                                     the same bits every launch.
//   projections                       project_rows_kernel: out[r][l] = (float) sum_c x[r][c] theta[l][c], the sum an fp64 FMA
//                                     chain in column order (the products of two floats are exact in fp64: it is the sequential
//                                     fp64 sum of exact products).  A workgroup owns 32 directions, stages 128 columns of theta
//                                     and of 32 rows at a time in LDS, and a thread carries 4 rows of one direction.  Theta's
//                                     rows are padded to 129 words (32 directions read one column: 32 banks); the 32 lanes of
//                                     a half read one word of x (a broadcast).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ssn_host.h"
#include "ssn_swd_dev.h"

namespace ssn {

// #{a[0 .. n) <= v} of an ascending array
__device__ __forceinline__ int wd_count_le(const float* a, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// grid (C, S); dynamic LDS: P floats, P = the power of two >= max(B, 64).  x[S][B][C]; t[C][T] ascending with the m[c] finite
// values first; n_out[S][C] (int), num_out[S][C] (long long), wnum_out[S][C] (double)
__global__ void __launch_bounds__(256) ks_w1_columns_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                            const int* __restrict__ m_of, int B, int C, int T, int P,
                                                            int* __restrict__ n_out, long long* __restrict__ num_out,
                                                            double* __restrict__ wnum_out) {
    extern __shared__ float wdist_lds[];
    float* sx = wdist_lds;
    const int c = blockIdx.x, s = blockIdx.y;
    const float inf = __builtin_huge_valf();
    const float* xs = x + (size_t)s * B * C + c;
    for (int i = threadIdx.x; i < P; i += 256) {
        float v = inf;
        if (i < B) {
            v = xs[(size_t)i * C];
            if (!(fabsf(v) < inf)) v = inf;                   // NaN, +inf, -inf: left out of the column
        }
        sx[i] = v;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int p = threadIdx.x; p < (P >> 1); p += 256) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const float a = sx[i], b = sx[i + j];
                const bool up = (i & k) == 0;
                if ((a > b) == up) { sx[i] = b; sx[i + j] = a; }
            }
            __syncthreads();
        }
    }
    const int n = wd_count_le(sx, P, 3.4028234663852886e38f); // the finite values: everything below +inf
    const int m = min(max(m_of[c], 0), T);
    const float* tc = t + (size_t)c * T;
    long long best = 0;
    double sum = 0.0;
    for (int i = threadIdx.x; i < n + m; i += 256) {
        const float v = i < n ? sx[i] : tc[i - n];
        const int ix = wd_count_le(sx, n, v), it = wd_count_le(tc, m, v);
        long long d = (long long)ix * m - (long long)it * n;
        if (d < 0) d = -d;
        if (d > best) best = d;
        const bool last = i < n ? (i == ix - 1 && (it == 0 || tc[it - 1] != v)) : (i - n == it - 1);
        if (last && (ix < n || it < m)) {
            float nx = inf;
            if (ix < n) nx = sx[ix];
            if (it < m) nx = fminf(nx, tc[it]);
            double term;
            {
#pragma clang fp contract(off)
                term = ((double)nx - (double)v) * (double)d;  // (rounded on its own: no FMA into the sum)
            }
            sum += term;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const long long o = __shfl_xor(best, off);
        if (o > best) best = o;
        sum += __shfl_xor(sum, off);
    }
    __syncthreads();                                          // every wave is done with sx: its first words carry the reduction
    long long* red = reinterpret_cast<long long*>(sx);
    double* redw = reinterpret_cast<double*>(sx) + 4;
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = best;
        redw[threadIdx.x >> 6] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            if (red[w] > best) best = red[w];
            sum += redw[w];
        }
        n_out[(size_t)s * C + c] = n;
        num_out[(size_t)s * C + c] = best;
        wnum_out[(size_t)s * C + c] = sum;
    }
}

// grid (direction tiles, row tiles up to a cap): project_rows_body (ssn_swd_dev.h) on one sample
__global__ void __launch_bounds__(256) project_rows_kernel(const float* __restrict__ x, long rows, int ldx, int C,
                                                           const float* __restrict__ theta, int L, float* __restrict__ out) {
    project_rows_body(x, rows, ldx, C, theta, L, out, blockIdx.x * PJ_DIRS, blockIdx.y, gridDim.y);
}

hipError_t launch_ks_w1_columns(const float* x, const float* t, const int* m, int S, int B, int C, int T, int* n_out,
                                long long* num_out, double* wnum_out, hipStream_t st) {
    if (S == 0 || C == 0) return hipSuccess;
    int P = 64;
    while (P < B) P <<= 1;
    for (int s0 = 0; s0 < S; s0 += 65535) {                   // (grid.y is a 16-bit count)
        const int ns = S - s0 < 65535 ? S - s0 : 65535;
        hipLaunchKernelGGL(ks_w1_columns_kernel, dim3(C, ns), dim3(256), (size_t)P * sizeof(float), st, x + (size_t)s0 * B * C, t, m,
                           B, C, T, P, n_out + (size_t)s0 * C, num_out + (size_t)s0 * C, wnum_out + (size_t)s0 * C);
    }
    return hipGetLastError();
}

hipError_t launch_project_rows(const float* x, long rows, int ldx, int C, const float* theta, int L, float* out, hipStream_t st) {
    if (rows == 0 || L == 0) return hipSuccess;
    const long tiles = (rows + PJ_ROWS - 1) / PJ_ROWS;
    const int gy = (int)(tiles < 4096 ? tiles : 4096);
    hipLaunchKernelGGL(project_rows_kernel, dim3((L + PJ_DIRS - 1) / PJ_DIRS, gy), dim3(256), 0, st, x, rows, ldx, C, theta, L, out);
    return hipGetLastError();
}

}  // namespace ssn
