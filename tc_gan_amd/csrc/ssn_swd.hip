// Sliced Wasserstein loss of a minibatch and its gradient (networks/sliced_wasserstein.py): the projections of the generated
// rows x and of the truth rows y onto L directions come from ssn_wdist.hip's project_rows_kernel; here every direction's two
// columns are sorted, matched rank by rank, and the coefficients are carried back to the rows.
//
//   match        swd_match_kernel: one workgroup per direction l.  The column px[.][l] becomes 64-bit keys -- high word an
//                order-preserving transform of the float with -0 taken as +0, low word the row index -- so that an integer sort
//                IS the stable sort by value (ties by row); py[.][l] stays floats.  Both are padded to P, the power of two
//                >= max(B, 64), with keys above every finite value, and sorted by one bitonic network (the two arrays share
//                its barriers).  A value that is not finite is found while loading: the workgroup then writes NaN to loss_l[l]
//                and to coef[.][l] and leaves, the sort never sees it.  Rank i: d = (double) u_i - (double) v_i, the term
//                |d| or d d (rounded on its own), the coefficient sign(d) inv or (2 d) inv scattered to coef[b_i][l].  A thread
//                sums its terms in index order, a wave adds lanes 32, 16, ... 1 apart, thread 0 adds the four waves in order and
//                divides by B: no atomics, the same bits every launch.
//   backproject  swd_backproject_kernel: gx[b][c] = (float) sum_l coef[b][l] theta[l][c], an fp64 FMA chain over l in order (the
//                products of two floats are exact in fp64).  A workgroup owns 16 rows x 16 columns and stages 64 directions of
//                coef and theta at a time in LDS; coef's rows are padded to 65 words (the 4 rows of a wave's half read one
//                direction: 4 banks), the 16 lanes of a row read one word of coef (a broadcast) and 16 consecutive of theta.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ssn_host.h"

namespace ssn {

// the float as an unsigned word whose order is the float order (finite values and the infinities); -0 is taken as +0
__device__ __forceinline__ uint32_t swd_ordered(float v) {
    const uint32_t u = v == 0.f ? 0u : __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float swd_unordered(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

// grid (L); dynamic LDS: P keys of 8 bytes, then P floats.  px[B][L], py[B][L]; coef[B][L]; loss_l[L]; inv = 1 / (L B)
__global__ void __launch_bounds__(256) swd_match_kernel(const float* __restrict__ px, const float* __restrict__ py, int B, int L,
                                                        int P, int power, double inv, float* __restrict__ coef,
                                                        double* __restrict__ loss_l) {
    extern __shared__ unsigned long long swd_lds[];
    __shared__ double red[4];
    __shared__ int bad;
    unsigned long long* kx = swd_lds;
    float* sy = reinterpret_cast<float*>(swd_lds + P);
    const int l = blockIdx.x;
    const float inf = __builtin_huge_valf();
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    bool mine = false;
    for (int i = threadIdx.x; i < P; i += 256) {
        unsigned long long key = ~0ull;                       // (above the key of +inf: the padding sorts last)
        float v = inf;
        if (i < B) {
            const float u = px[(size_t)i * L + l];
            v = py[(size_t)i * L + l];
            mine |= !(fabsf(u) < inf) || !(fabsf(v) < inf);
            key = ((unsigned long long)swd_ordered(u) << 32) | (unsigned)i;
        }
        kx[i] = key;
        sy[i] = v;
    }
    if (mine) bad = 1;
    __syncthreads();
    if (bad) {                                                // NaN, +inf or -inf in either column: nothing is sorted
        const float nan = __builtin_nanf("");
        for (int i = threadIdx.x; i < B; i += 256) coef[(size_t)i * L + l] = nan;
        if (threadIdx.x == 0) loss_l[l] = __builtin_nan("");
        return;
    }
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int p = threadIdx.x; p < (P >> 1); p += 256) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const bool up = (i & k) == 0;
                const unsigned long long a = kx[i], b = kx[i + j];
                if ((a > b) == up) { kx[i] = b; kx[i + j] = a; }
                const float c = sy[i], d = sy[i + j];
                if ((c > d) == up) { sy[i] = d; sy[i + j] = c; }
            }
            __syncthreads();
        }
    }
    double sum = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) {
        const unsigned long long key = kx[i];
        const int b = (int)(unsigned)key;
        const double d = (double)swd_unordered((uint32_t)(key >> 32)) - (double)sy[i];
        double term, cf;
        {
#pragma clang fp contract(off)
            if (power == 1) {
                term = fabs(d);
                cf = (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0)) * inv;
            } else {
                term = d * d;                                 // (rounded on its own: no FMA into the sum)
                cf = (2.0 * d) * inv;
            }
        }
        sum += term;
        if (b < B) coef[(size_t)b * L + l] = (float)cf;       // (the first B ranks are rows: the padding sorts behind them)
    }
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) sum += red[w];
        loss_l[l] = sum / (double)B;
    }
}

constexpr int BP_ROWS = 16;                                   // rows of a workgroup
constexpr int BP_COLS = 16;                                   // columns of a workgroup
constexpr int BP_DIRS = 64;                                   // directions staged at a time

// grid (column tiles, row tiles): 256 threads = 16 rows x 16 columns.  coef[B][L], theta[L][D], gx[B][D]
__global__ void __launch_bounds__(256) swd_backproject_kernel(const float* __restrict__ coef, const float* __restrict__ theta,
                                                              int B, int L, int D, float* __restrict__ gx) {
    __shared__ float sc[BP_ROWS][BP_DIRS + 1];
    __shared__ float sth[BP_DIRS][BP_COLS];
    const int cc = threadIdx.x & (BP_COLS - 1), rr = threadIdx.x >> 4;
    const int c0 = blockIdx.x * BP_COLS;
    const int tiles = (B + BP_ROWS - 1) / BP_ROWS;
    for (int tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
        const int r0 = tile * BP_ROWS;
        double acc = 0.0;
        for (int l0 = 0; l0 < L; l0 += BP_DIRS) {
            const int ln = min(BP_DIRS, L - l0);
            __syncthreads();                                  // the tile before this one has been read
            for (int e = threadIdx.x; e < BP_ROWS * BP_DIRS; e += 256) {
                const int row = e / BP_DIRS, ll = e - row * BP_DIRS;
                sc[row][ll] = (ll < ln && r0 + row < B) ? coef[(size_t)(r0 + row) * L + l0 + ll] : 0.f;
                const int tl = e / BP_COLS, tcol = e - tl * BP_COLS;
                sth[tl][tcol] = (tl < ln && c0 + tcol < D) ? theta[(size_t)(l0 + tl) * D + c0 + tcol] : 0.f;
            }
            __syncthreads();
            for (int ll = 0; ll < ln; ++ll) acc = __builtin_fma((double)sc[rr][ll], (double)sth[ll][cc], acc);
        }
        if (r0 + rr < B && c0 + cc < D) gx[(size_t)(r0 + rr) * D + c0 + cc] = (float)acc;
    }
}

hipError_t launch_swd_match(const float* px, const float* py, int B, int L, int power, float* coef, double* loss_l, hipStream_t st) {
    if (B == 0 || L == 0) return hipSuccess;
    int P = 64;
    while (P < B) P <<= 1;
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
