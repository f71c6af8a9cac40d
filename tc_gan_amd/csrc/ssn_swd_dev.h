// Device bodies of the sliced Wasserstein loss kernels, shared by the single-run kernels (ssn_wdist.hip: project_rows_kernel;
// ssn_swd.hip: swd_match_kernel, swd_backproject_kernel) and the grid-over-members kernels of ssn_ens_swd.hip.  A body takes the
// base pointers of ONE problem (one sample, one member) and the part of the grid that works on it; the kernels differ only in how
// they find those from blockIdx, so a member's values are the bits of its single run by construction.  The sort and the ordered
// sum of the match are ssn_sortcol_dev.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ssn_sortcol_dev.h"

namespace ssn {

// the float as an unsigned word whose order is the float order (finite values and the infinities); -0 is taken as +0
__device__ __forceinline__ uint32_t swd_ordered(float v) {
    const uint32_t u = v == 0.f ? 0u : __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float swd_unordered(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

// the term of rank i and the coefficient of its row: d = (double) u_i - (double) v_i
__device__ __forceinline__ void swd_rank_term(double d, int power, double inv, double& term, double& cf) {
#pragma clang fp contract(off)
    if (power == 1) {
        term = fabs(d);
        cf = (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0)) * inv;
    } else {
        term = d * d;                                         // (rounded on its own: no FMA into the sum)
        cf = (2.0 * d) * inv;
    }
}

constexpr int PJ_DIRS = 32;                                   // directions of a workgroup
constexpr int PJ_ROWS = 32;                                   // rows of a tile: 8 row slots x 4 rows per thread
constexpr int PJ_COLS = 128;                                  // columns staged at a time
static_assert(PJ_DIRS == PJ_ROWS, "one staging loop fills both tiles");

// 256 threads = 8 row slots x 32 directions: the directions [l0, l0 + 32) of the row tiles tile0, tile0 + tile_step, ...
// x[rows][ldx] (the first C of a row are used), theta[L][C], out[rows][L]
__device__ __forceinline__ void project_rows_body(const float* __restrict__ x, long rows, int ldx, int C,
                                                  const float* __restrict__ theta, int L, float* __restrict__ out, int l0,
                                                  long tile0, long tile_step) {
    __shared__ float sth[PJ_DIRS][PJ_COLS + 1];
    __shared__ float sxr[PJ_ROWS][PJ_COLS];
    const int ll = threadIdx.x & (PJ_DIRS - 1), slot = threadIdx.x >> 5;
    const long tiles = (rows + PJ_ROWS - 1) / PJ_ROWS;
    for (long tile = tile0; tile < tiles; tile += tile_step) {
        const long r0 = tile * PJ_ROWS;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int c0 = 0; c0 < C; c0 += PJ_COLS) {
            const int cn = min(PJ_COLS, C - c0);
            __syncthreads();                                  // the tile before this one has been read
            for (int e = threadIdx.x; e < PJ_DIRS * PJ_COLS; e += 256) {
                const int row = e / PJ_COLS, col = e - row * PJ_COLS;
                const bool in_cols = col < cn;
                sth[row][col] = (in_cols && l0 + row < L) ? theta[(size_t)(l0 + row) * C + c0 + col] : 0.f;
                sxr[row][col] = (in_cols && r0 + row < rows) ? x[(size_t)(r0 + row) * ldx + c0 + col] : 0.f;
            }
            __syncthreads();
            for (int cc = 0; cc < cn; ++cc) {
                const double th = (double)sth[ll][cc];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = __builtin_fma((double)sxr[slot + 8 * k][cc], th, acc[k]);
            }
        }
        if (l0 + ll < L) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long r = r0 + slot + 8 * k;
                if (r < rows) out[(size_t)r * L + l0 + ll] = (float)acc[k];
            }
        }
    }
}

// one workgroup of 256 threads, direction l; dynamic LDS: P keys of 8 bytes, then P floats.  px[B][L], py[B][L]; coef[B][L];
// loss_l[L]; inv = 1 / (L B)
__device__ __forceinline__ void swd_match_body(const float* __restrict__ px, const float* __restrict__ py, int B, int L, int P,
                                               int power, double inv, float* __restrict__ coef, double* __restrict__ loss_l,
                                               int l) {
    extern __shared__ unsigned long long swd_lds[];
    __shared__ double red[4];
    __shared__ int bad;
    unsigned long long* kx = swd_lds;
    float* sy = reinterpret_cast<float*>(swd_lds + P);
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
    bitonic_sort_lds(P, kx, sy);
    double sum = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) {
        const unsigned long long key = kx[i];
        const int b = (int)(unsigned)key;
        const double d = (double)swd_unordered((uint32_t)(key >> 32)) - (double)sy[i];
        double term, cf;
        swd_rank_term(d, power, inv, term, cf);
        sum += term;
        if (b < B) coef[(size_t)b * L + l] = (float)cf;       // (the first B ranks are rows: the padding sorts behind them)
    }
    sum = block_sum_in_order(sum, red);
    if (threadIdx.x == 0) loss_l[l] = sum / (double)B;
}

constexpr int BP_ROWS = 16;                                   // rows of a workgroup
constexpr int BP_COLS = 16;                                   // columns of a workgroup
constexpr int BP_DIRS = 64;                                   // directions staged at a time

// 256 threads = 16 rows x 16 columns: the columns [c0, c0 + 16) of the row tiles tile0, tile0 + tile_step, ...
// coef[B][L], theta[L][D], gx[B][D]
__device__ __forceinline__ void swd_backproject_body(const float* __restrict__ coef, const float* __restrict__ theta, int B, int L,
                                                     int D, float* __restrict__ gx, int c0, int tile0, int tile_step) {
    __shared__ float sc[BP_ROWS][BP_DIRS + 1];
    __shared__ float sth[BP_DIRS][BP_COLS];
    const int cc = threadIdx.x & (BP_COLS - 1), rr = threadIdx.x >> 4;
    const int tiles = (B + BP_ROWS - 1) / BP_ROWS;
    for (int tile = tile0; tile < tiles; tile += tile_step) {
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

}  // namespace ssn
