// What the kernels that sort a column in LDS and reduce the result share: the KS scorer (ssn_score.hip), the KS + W1 scorer
// (ssn_wdist.hip) and the match of the sliced Wasserstein loss (ssn_swd_dev.h, for ssn_swd.hip and ssn_ens_swd.hip).  One copy
// each of the binary search, the bitonic network, the ordered block reductions and the KS / W1 body with the host launcher of
// its two kernels (a template over the kernel, so it stands here and not in ssn_host.h).  Workgroups are 256 threads.
// The summation order (pinned bit for bit by tests/wasserstein_cases.py and tests/swd_cases.py, which restate it): element i
// belongs to thread i % 256; a thread adds its terms in increasing i, starting from +0; the 64 lanes of a wave then do
// v = v + v[lane ^ off] for off = 32, 16, 8, 4, 2, 1; thread 0 adds the results of waves 1, 2, 3 to its own in that order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ssn_host.h"

namespace ssn {

// #{a[0 .. n) <= v} of an ascending array
__device__ __forceinline__ int count_le(const float* a, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The rule of the bitonic network on the pair (i, i + j): a is the value at the lower index, b the one at the upper, and the two
// change places where (a > b) == up (up: the pair's block sorts ascending)
template <typename T>
__device__ __forceinline__ void cmp_exchange(T* s, int i, int j, bool up) {
    T* lower = s + i;
    T* upper = lower + j;
    const T a = *lower, b = *upper;
    if ((a > b) == up) { *lower = b; *upper = a; }
}

// Sorts a[0 .. P) ascending, P a power of two >= 2, every array on its own; the arrays share the barriers.  Called by all 256
// threads after a barrier behind the stores that filled the arrays; ends with a barrier.
//
// LDS banks (MI355X: ds_read_b32 / ds_write_b32 are served per 32-lane half on 32 banks of 4 bytes): a step with partner
// distance j handles pair p as elements i = 2 (p - p % j) + p % j and i + j.  For j >= 32 the 32 lanes of a half read 32
// consecutive dwords: no conflict.  For j < 32 they read j consecutive dwords out of every 2 j: 2-way on the i's, and the i + j's
// fill the other banks' second turn, so a step costs two LDS cycles per half and instruction where a conflict-free one costs
// one; the stores' 2-way costs nothing (a store's time is its register transfer).  The sort is log2(P) (log2(P) + 1) / 2 such
// steps of P / 2 pairs.
template <typename... T>
__device__ __forceinline__ void bitonic_sort_lds(int P, T*... a) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int p = threadIdx.x; p < (P >> 1); p += 256) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const bool up = (i & k) == 0;
                (cmp_exchange(a, i, j, up), ...);
            }
            __syncthreads();
        }
    }
}

// The ordered reductions.  Of a wave: every lane ends with the result.  Of the block, in two halves around ONE barrier of the
// caller's, so that several values share it: the first lane of every wave posts its wave's result to slots[4] in LDS, and
// behind the barrier thread 0 folds the slots of waves 1, 2, 3 into its own value, in that order.
__device__ __forceinline__ double wave_sum_in_order(double v) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ long long wave_max(long long v) {
    for (int off = 32; off >= 1; off >>= 1) {
        const long long o = __shfl_xor(v, off);
        if (o > v) v = o;
    }
    return v;
}
template <typename T>
__device__ __forceinline__ void post_wave_result(T* slots, T v) {
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
}
__device__ __forceinline__ double waves_sum_in_order(double v, const double* slots) {
    for (int w = 1; w < 4; ++w) v += slots[w];
    return v;
}
__device__ __forceinline__ long long waves_max(long long v, const long long* slots) {
    for (int w = 1; w < 4; ++w) if (slots[w] > v) v = slots[w];
    return v;
}
// the sum of v over the block: the result is thread 0's
__device__ __forceinline__ double block_sum_in_order(double v, double* slots) {
    v = wave_sum_in_order(v);
    post_wave_result(slots, v);
    __syncthreads();
    if (threadIdx.x == 0) v = waves_sum_in_order(v, slots);
    return v;
}

// The KS statistic of one column against its truth column and, with W1, the Wasserstein numerator beside it.  Workgroup
// (c, s) = blockIdx.(x, y); sx: P floats of LDS, P = sort_slots(B).  x[S][B][C]; t[C][T] ascending with the m[c] finite values
// first; n_out[S][C] (int), num_out[S][C] (long long), wnum_out[S][C] (double, W1 only).
//
// The B values go to LDS (non-finite ones and the padding as +inf), the sort puts the n finite values first, and every pooled
// point v -- the n values and the column's m truth values -- gets ix = #{x <= v} and it = #{t <= v} by binary search (x in LDS,
// the truth column in global memory: 4 T bytes that stay in cache); these (n + m) (log2 n + log2 m) search steps are the larger
// part at the scorer's sizes.  num = max |ix m - it n|.  wnum = sum_k (p_{k+1} - p_k) |ix m - it n| over the distinct pooled
// values p_0 < ... < p_K: the owner of pooled element i adds the term of its value only if i is the value's LAST occurrence in
// the pool (x first, then t); the successor is the smaller of sx[ix] and t[it] where those exist, the largest value has none.
// Gap and weight are formed in fp64 (the weight is an integer below 2^53), their product is rounded once.
template <bool W1>
__device__ __forceinline__ void ks_column_body(const float* __restrict__ x, const float* __restrict__ t,
                                               const int* __restrict__ m_of, int B, int C, int T, int P, int* __restrict__ n_out,
                                               long long* __restrict__ num_out, double* __restrict__ wnum_out, float* sx) {
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
    bitonic_sort_lds(P, sx);
    const int n = count_le(sx, P, 3.4028234663852886e38f);    // the finite values: everything below +inf
    const int m = min(max(m_of[c], 0), T);
    const float* tc = t + (size_t)c * T;
    long long best = 0;
    double sum = 0.0;
    for (int i = threadIdx.x; i < n + m; i += 256) {
        const float v = i < n ? sx[i] : tc[i - n];
        const int ix = count_le(sx, n, v), it = count_le(tc, m, v);
        long long d = (long long)ix * m - (long long)it * n;
        if (d < 0) d = -d;
        if (d > best) best = d;
        if constexpr (W1) {
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
    }
    best = wave_max(best);
    if constexpr (W1) sum = wave_sum_in_order(sum);
    __syncthreads();                                          // every wave is done with sx: its first words carry the reduction
    long long* red = reinterpret_cast<long long*>(sx);
    double* redw = reinterpret_cast<double*>(sx) + 4;
    post_wave_result(red, best);
    if constexpr (W1) post_wave_result(redw, sum);
    __syncthreads();
    if (threadIdx.x == 0) {
        n_out[(size_t)s * C + c] = n;
        num_out[(size_t)s * C + c] = waves_max(best, red);
        if constexpr (W1) wnum_out[(size_t)s * C + c] = waves_sum_in_order(sum, redw);
    }
}

// One launch per 65535 sets (grid.y is a 16-bit count) of a kernel over ks_column_body: grid (C, sets), the outputs [S][C]
template <typename... Out>
hipError_t launch_ks_kernel(void (*kernel)(const float*, const float*, const int*, int, int, int, int, Out*...), const float* x,
                            const float* t, const int* m, int S, int B, int C, int T, hipStream_t st, Out*... out) {
    if (S == 0 || C == 0) return hipSuccess;
    const int P = sort_slots(B);
    for (int s0 = 0; s0 < S; s0 += 65535) {
        const int ns = S - s0 < 65535 ? S - s0 : 65535;
        hipLaunchKernelGGL(kernel, dim3(C, ns), dim3(256), (size_t)P * sizeof(float), st, x + (size_t)s0 * B * C, t, m, B, C, T, P,
                           (out + (size_t)s0 * C)...);
    }
    return hipGetLastError();
}

}  // namespace ssn
