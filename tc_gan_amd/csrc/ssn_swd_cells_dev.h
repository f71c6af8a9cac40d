// Device body of the sliced Wasserstein match per condition cell (ssn_swd_cells.hip; the entry point lives in
// libssnode_ext2.so, include/ssnode_mi355x_ext2.h).  One (cell, direction) is the match of two samples of different sizes over a
// SEGMENT of the generated rows: the segment's k-th value is px[rows[k]][l], the key carries the local index k, and the
// coefficient of rank i goes to rows[k_i].  The walk over the quantile cells is restated here from the first companion library's
// match (that library's headers are its own and are not included by any other file); tests/test_swd_cells_gpu.py holds the two
// to the same bits at one cell.  The key transform, the sort and the ordered block sum are ssn_swd_dev.h's and
// ssn_sortcol_dev.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ssn_sortcol_dev.h"
#include "ssn_swd_dev.h"

namespace ssn {

// one workgroup of 256 threads: direction l of one cell.  Dynamic LDS: Pn keys of 8 bytes, then Pm floats, Pn >= sort_slots(n),
// Pm = sort_slots(m).  px[B][L]; rows[n]: the cell's row indices; py[m][L]: the cell's truth block; coef[B][L]; loss: the cell's
// loss_cl[c] + l; inv = 1 / (L B m)
__device__ __forceinline__ void swd_match_cell_body(const float* __restrict__ px, int B, const int* __restrict__ rows, int n,
                                                    const float* __restrict__ py, int m, int L, int Pn, int Pm, int power,
                                                    double inv, float* __restrict__ coef, double* __restrict__ loss, int l) {
    extern __shared__ unsigned long long swd_cells_lds[];
    __shared__ double red[4];
    __shared__ int bad;
    if (n == 0) {                                             // an empty cell: its loss is +0 and no row is its own
        if (threadIdx.x == 0) *loss = 0.0;
        return;
    }
    unsigned long long* kx = swd_cells_lds;
    float* sy = reinterpret_cast<float*>(swd_cells_lds + Pn);
    const float inf = __builtin_huge_valf();
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    bool mine = false;
    for (int k = threadIdx.x; k < Pn; k += 256) {
        unsigned long long key = ~0ull;                       // (above the key of +inf: the padding sorts last)
        if (k < n) {
            const unsigned row = (unsigned)rows[k];
            const float u = row < (unsigned)B ? px[(size_t)row * L + l] : 0.f;
            mine |= !(fabsf(u) < inf);
            key = ((unsigned long long)swd_ordered(u) << 32) | (unsigned)k;
        }
        kx[k] = key;
    }
    for (int j = threadIdx.x; j < Pm; j += 256) {
        float v = inf;
        if (j < m) {
            v = py[(size_t)j * L + l];
            mine |= !(fabsf(v) < inf);
        }
        sy[j] = v;
    }
    if (mine) bad = 1;
    __syncthreads();
    if (bad) {                                                // NaN, +inf or -inf in the segment or the block: nothing is sorted
        const float nan = __builtin_nanf("");
        for (int k = threadIdx.x; k < n; k += 256) {
            const unsigned row = (unsigned)rows[k];
            if (row < (unsigned)B) coef[(size_t)row * L + l] = nan;
        }
        if (threadIdx.x == 0) *loss = __builtin_nan("");
        return;
    }
    bitonic_sort_lds(Pn, kx);
    bitonic_sort_lds(Pm, sy);
    double sum = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const unsigned long long key = kx[i];
        const unsigned k = (unsigned)key;
        const double u = (double)swd_unordered((uint32_t)(key >> 32));
        const long long lo = (long long)i * m, hi = lo + m;   // rank i owns [lo, hi) of the n m quantile cells
        const int j_lo = (int)(lo / n), j_hi = (int)((hi - 1) / n);
        double t = 0.0, cd = 0.0;
        long long ci = 0;
        for (int j = j_lo; j <= j_hi; ++j) {                  // (j_hi < m: hi - 1 < n m)
#pragma clang fp contract(off)
            const long long ylo = (long long)j * n, yhi = ylo + n;
            const double w = (double)((hi < yhi ? hi : yhi) - (lo > ylo ? lo : ylo));
            const double d = u - (double)sy[j];
            if (power == 1) {
                t += w * fabs(d);
                ci += (long long)w * (d > 0.0 ? 1 : (d < 0.0 ? -1 : 0));
            } else {
                const double dd = d * d;                      // (rounded on its own, as the product with w: no FMA into the sum)
                t += w * dd;
                cd += w * (2.0 * d);
            }
        }
        sum += t;
        const double c = power == 1 ? (double)ci : cd;
        if (k < (unsigned)n) {                                // (the first n ranks are the segment: the padding sorts behind)
            const unsigned row = (unsigned)rows[k];
            if (row < (unsigned)B) coef[(size_t)row * L + l] = (float)(c * inv);
        }
    }
    sum = block_sum_in_order(sum, red);
    if (threadIdx.x == 0) *loss = sum / ((double)n * (double)m);
}

}  // namespace ssn
