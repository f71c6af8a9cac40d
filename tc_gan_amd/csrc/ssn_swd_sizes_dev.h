// Device body of the sliced Wasserstein match of two samples of DIFFERENT sizes (ssn_swd_sizes.hip; the entry point lives in
// libssnode_ext.so, include/ssnode_mi355x_ext.h).  The key transform, the sort and the ordered block sum are those of the
// equal-size match (ssn_swd_dev.h, ssn_sortcol_dev.h): what is new is the coupling.  On a quantile axis scaled by n m the rank i
// of the n generated values owns [i m, (i + 1) m) and the rank j of the m truth values owns [j n, (j + 1) n); rank i meets the
// ranks j_lo = floor(i m / n) .. j_hi = floor(((i + 1) m - 1) / n) with the integer overlaps w_ij as weights.  For n == m this
// is the rank coupling with every weight n.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ssn_sortcol_dev.h"
#include "ssn_swd_dev.h"

namespace ssn {

// one workgroup of 256 threads, direction l; dynamic LDS: Pn keys of 8 bytes, then Pm floats.  px[n][L], py[m][L]; coef[n][L];
// loss_l[L]; inv = 1 / (L n m); Pn = sort_slots(n), Pm = sort_slots(m)
__device__ __forceinline__ void swd_match_sizes_body(const float* __restrict__ px, int n, const float* __restrict__ py, int m,
                                                     int L, int Pn, int Pm, int power, double inv, float* __restrict__ coef,
                                                     double* __restrict__ loss_l, int l) {
    extern __shared__ unsigned long long swd_sizes_lds[];
    __shared__ double red[4];
    __shared__ int bad;
    unsigned long long* kx = swd_sizes_lds;
    float* sy = reinterpret_cast<float*>(swd_sizes_lds + Pn);
    const float inf = __builtin_huge_valf();
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    bool mine = false;
    for (int i = threadIdx.x; i < Pn; i += 256) {
        unsigned long long key = ~0ull;                       // (above the key of +inf: the padding sorts last)
        if (i < n) {
            const float u = px[(size_t)i * L + l];
            mine |= !(fabsf(u) < inf);
            key = ((unsigned long long)swd_ordered(u) << 32) | (unsigned)i;
        }
        kx[i] = key;
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
    if (bad) {                                                // NaN, +inf or -inf in either column: nothing is sorted
        const float nan = __builtin_nanf("");
        for (int i = threadIdx.x; i < n; i += 256) coef[(size_t)i * L + l] = nan;
        if (threadIdx.x == 0) loss_l[l] = __builtin_nan("");
        return;
    }
    bitonic_sort_lds(Pn, kx);
    bitonic_sort_lds(Pm, sy);
    double sum = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const unsigned long long key = kx[i];
        const int b = (int)(unsigned)key;
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
        if ((unsigned)b < (unsigned)n) coef[(size_t)b * L + l] = (float)(c * inv);   // (the first n ranks are rows)
    }
    sum = block_sum_in_order(sum, red);
    if (threadIdx.x == 0) loss_l[l] = sum / ((double)n * (double)m);
}

}  // namespace ssn
