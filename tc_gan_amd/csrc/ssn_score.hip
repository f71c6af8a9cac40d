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
//   KS statistic per (set, column)    ks_columns_kernel: one workgroup per (s, column) sorts the column in LDS and walks the
//                                     pooled sample: ks_column_body (ssn_sortcol_dev.h).  The statistic is kept as the integer
//                                     num = max |#{x <= v} m - #{t <= v} n| (KSD = num / (n m)): exact whatever the ties, and
//                                     what scipy.stats.ks_2samp(...).statistic computes in floating point.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ssn_host.h"
#include "ssn_sortcol_dev.h"

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

// grid (C, S); dynamic LDS: P floats, P = sort_slots(B): ks_column_body (ssn_sortcol_dev.h) without the W1 sum
__global__ void __launch_bounds__(256) ks_columns_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                         const int* __restrict__ m_of, int B, int C, int T, int P,
                                                         int* __restrict__ n_out, long long* __restrict__ num_out) {
    extern __shared__ float score_lds[];
    ks_column_body<false>(x, t, m_of, B, C, T, P, n_out, num_out, nullptr, score_lds);
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
    return launch_ks_kernel(ks_columns_kernel, x, t, m, S, B, C, T, st, n_out, num_out);
}

}  // namespace ssn
