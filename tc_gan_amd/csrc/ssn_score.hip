// Scoring the checkpoints of a run (analyzers/distdiff.py): S recorded parameter sets share ONE noise draw z[B] and run as one
// forward batch of S B draws; the result is reduced to two-sample Kolmogorov-Smirnov statistics against the truth on the device.
//
//   W for a table of parameter sets   build_w_table_kernel: W[s][b] = make_W(z[b]; J_s, D_s, S_s).  A thread keeps its 16 bytes
//                                     of z in registers and walks the S sets: z is read once per draw, W is written once per
//                                     (set, draw).  The arithmetic is w_from_z's (ssn_host.h), the constants are formed from the
//                                     device table the way build_w_kernel forms them from device parameters: the same values
//                                     give the bits of ssn_build_w_f32.
//   per-curve features                tc_features_kernel: maxrate, suppression index, preferred bandwidth (first index of the
//                                     maximum) and inverse participation ratio of every curve over its NB bandwidths, fp32, sums
//                                     in bandwidth order.
//   KS statistic per (set, column)    ks_columns_kernel: one workgroup per (s, column).  The B values go to LDS (non-finite ones
//                                     as +inf, the padding up to a power of two as +inf too), a bitonic sort puts the n finite
//                                     values first, and every pooled point v -- the n values and the column's m truth values --
//                                     gets #{x <= v} and #{t <= v} by binary search (x in LDS, the sorted truth column in
//                                     global memory: 4 T bytes that stay in cache for the workgroup).  The statistic is kept as
//                                     the integer num = max |#{x <= v} m - #{t <= v} n| (KSD = num / (n m)): exact whatever the
//                                     ties, and what scipy.stats.ks_2samp(...).statistic computes in floating point.
//
// LDS banks of the sort (MI355X: ds_read_b32 / ds_write_b32 are served per 32-lane half on 32 banks of 4 bytes): a step with
// partner distance j handles pair p as elements i = 2 (p - p % j) + p % j and i + j.  For j >= 32 the 32 lanes of a half read 32
// consecutive dwords: no conflict.  For j < 32 they read j consecutive dwords out of every 2 j: 2-way on the i's, and the i + j's
// fill the other banks' second turn, so a step costs two LDS cycles per half and instruction where a conflict-free one costs
// one; the stores' 2-way costs nothing (a store's time is its register transfer).  The sort is log2(P) (log2(P) + 1) / 2 such
// steps of P / 2 pairs, the walk (n + m) (log2 n + log2 m) search steps; at the sizes the scorer runs (tens to a few thousand
// draws per set against a few thousand truth rows) the walk is the larger part.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ssn_host.h"

namespace ssn {

// grid: blocks of 256 threads over the vectors of z[B][M][M]; dynamic LDS: S JDS<float> records
template <int VEC>
__global__ void __launch_bounds__(256) build_w_table_kernel(const float* __restrict__ z, const float* __restrict__ table,
                                                            float* __restrict__ W, int S, int N, long total_vec) {
    extern __shared__ float score_lds[];
    JDS<float>* sets = reinterpret_cast<JDS<float>*>(score_lds);
    for (int e = threadIdx.x; e < S * 4; e += 256) {
        const int s = e >> 2, q = e & 3;
        const float* p = table + (size_t)s * 12;
        sets[s].J[q] = p[q];
        sets[s].D[q] = p[4 + q];
        const float sg = p[8 + q];
        float two_s2;
        {
#pragma clang fp contract(off)
            two_s2 = 2.f * sg * sg;
        }
        sets[s].inv2s2[q] = 1.f / two_s2;
    }
    __syncthreads();
    const int M = 2 * N;
    const float inv_nm1 = (N > 1) ? 1.f / (float)(N - 1) : 0.f;
    const long per_set = total_vec * VEC;                     // elements of one set's W[B][M][M]
    for (long v = blockIdx.x * 256L + threadIdx.x; v < total_vec; v += (long)gridDim.x * 256L) {
        const long e0 = v * VEC;
        const int col0 = (int)(e0 % M);
        const int row = (int)((e0 / M) % M);
        float zin[VEC];
        if constexpr (VEC == 4) {
            const float4 q = *reinterpret_cast<const float4*>(z + e0);
            zin[0] = q.x; zin[1] = q.y; zin[2] = q.z; zin[3] = q.w;
        } else {
            zin[0] = z[e0];
        }
        for (int s = 0; s < S; ++s) {
            float w[VEC];
#pragma unroll
            for (int t = 0; t < VEC; ++t) w[t] = w_from_z<float>(sets[s], N, inv_nm1, row, col0 + t, zin[t]);
            float* out = W + (size_t)s * per_set + e0;
            if constexpr (VEC == 4) {
                float4 q; q.x = w[0]; q.y = w[1]; q.z = w[2]; q.w = w[3];
                *reinterpret_cast<float4*>(out) = q;
            } else {
                out[0] = w[0];
            }
        }
    }
}

// One thread per (row, curve): tc[R][NC NB Q], column (c NB + b) Q + q (Q = cell types x probes); feat[R][4][NC Q], feature
// f of curve c Q + q in column f NC Q + c Q + q.  A NaN in a curve makes its maxrate NaN and prefbw the NaN's index (numpy's
// max / argmax).
__global__ void __launch_bounds__(256) tc_features_kernel(const float* __restrict__ tc, float* __restrict__ feat, long R, int NC,
                                                          int NB, int Q) {
    const int curves = NC * Q;
    const long total = R * curves;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
        const long r = e / curves;
        const int k = (int)(e - r * curves), c = k / Q, q = k - c * Q;
        const float* x = tc + r * (long)NC * NB * Q + (long)c * NB * Q + q;
        float mx = x[0], s1 = 0.f, s2 = 0.f, last = 0.f;
        int arg = 0;
        for (int b = 0; b < NB; ++b) {
            const float v = x[(long)b * Q];
            if (v > mx || (v != v && mx == mx)) { mx = v; arg = b; }
            s1 += v;
            s2 += v * v;
            last = v;
        }
        float* out = feat + r * 4L * curves + k;
        out[0] = mx;
        out[curves] = 1.f - last / mx;
        out[2 * curves] = (float)arg;
        out[3 * curves] = (s1 * s1) / ((float)NB * s2);
    }
}

// #{a[0 .. n) <= v} of an ascending array
__device__ __forceinline__ int count_le(const float* a, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// grid (C, S); dynamic LDS: P floats, P = the power of two >= max(B, 64).  x[S][B][C]; t[C][T] ascending with the m[c] finite
// values first; n_out[S][C] (int), num_out[S][C] (long long)
__global__ void __launch_bounds__(256) ks_columns_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                         const int* __restrict__ m_of, int B, int C, int T, int P,
                                                         int* __restrict__ n_out, long long* __restrict__ num_out) {
    extern __shared__ float score_lds[];
    float* sx = score_lds;
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
    const int n = count_le(sx, P, 3.4028234663852886e38f);    // the finite values: everything below +inf
    const int m = min(max(m_of[c], 0), T);
    const float* tc = t + (size_t)c * T;
    long long best = 0;
    for (int i = threadIdx.x; i < n + m; i += 256) {
        const float v = i < n ? sx[i] : tc[i - n];
        const long long cx = count_le(sx, n, v), ct = count_le(tc, m, v);
        long long d = cx * m - ct * n;
        if (d < 0) d = -d;
        if (d > best) best = d;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const long long o = __shfl_xor(best, off);
        if (o > best) best = o;
    }
    __syncthreads();                                          // every wave is done with sx: its first words carry the reduction
    long long* red = reinterpret_cast<long long*>(sx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) if (red[w] > best) best = red[w];
        n_out[(size_t)s * C + c] = n;
        num_out[(size_t)s * C + c] = best;
    }
}

hipError_t launch_build_w_table(const float* z, const float* table, float* W, int S, int B, int N, hipStream_t st) {
    const int M = 2 * N;
    const long total = (long)B * M * M;
    if (total == 0 || S == 0) return hipSuccess;
    const bool vec4 = (M % 4 == 0) && (((uintptr_t)z | (uintptr_t)W) % 16 == 0);      // (total % 4 == 0 then: every set's W stays aligned)
    const long nvec = vec4 ? total / 4 : total;
    const int blocks = (int)((nvec + 255) / 256 < 256 * 8 ? (nvec + 255) / 256 : 256 * 8);
    const int slice = 1024;                                   // sets per launch: 48 KiB of constants in LDS
    for (int s0 = 0; s0 < S; s0 += slice) {
        const int ns = S - s0 < slice ? S - s0 : slice;
        const size_t lds = (size_t)ns * sizeof(JDS<float>);
        const float* tb = table + (size_t)s0 * 12;
        float* Ws = W + (size_t)s0 * total;
        if (vec4) hipLaunchKernelGGL((build_w_table_kernel<4>), dim3(blocks), dim3(256), lds, st, z, tb, Ws, ns, N, nvec);
        else      hipLaunchKernelGGL((build_w_table_kernel<1>), dim3(blocks), dim3(256), lds, st, z, tb, Ws, ns, N, nvec);
    }
    return hipGetLastError();
}

hipError_t launch_tc_features(const float* tc, float* feat, long R, int NC, int NB, int Q, hipStream_t st) {
    const long total = R * NC * Q;
    if (total == 0) return hipSuccess;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(tc_features_kernel, dim3(blocks), dim3(256), 0, st, tc, feat, R, NC, NB, Q);
    return hipGetLastError();
}

hipError_t launch_ks_columns(const float* x, const float* t, const int* m, int S, int B, int C, int T, int* n_out,
                             long long* num_out, hipStream_t st) {
    if (S == 0 || C == 0) return hipSuccess;
    int P = 64;
    while (P < B) P <<= 1;
    for (int s0 = 0; s0 < S; s0 += 65535) {                   // (grid.y is a 16-bit count)
        const int ns = S - s0 < 65535 ? S - s0 : 65535;
        hipLaunchKernelGGL(ks_columns_kernel, dim3(C, ns), dim3(256), (size_t)P * sizeof(float), st, x + (size_t)s0 * B * C, t, m,
                           B, C, T, P, n_out + (size_t)s0 * C, num_out + (size_t)s0 * C);
    }
    return hipGetLastError();
}

}  // namespace ssn
