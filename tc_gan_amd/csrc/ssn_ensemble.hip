// Ensembles of moment-matching runs (networks/moment_matching_ensemble.py): K independent runs whose draws share the generator
// launches.  Member k owns the contiguous draws [k B, (k + 1) B) of every batch; what differs between members (data moments,
// moment weights, learning rates, regularisation, clip bounds, J / D / S / V, loss costs) comes in small device arrays indexed by
// the member.  Every kernel here is ONE launch whatever K is, and every sum of a member runs over that member's rows only: a
// NaN in one member reaches no other member's sums, update or record.
//
//   moment sums / loss gradient    moment_sums_kernel / moment_loss_grad_kernel (ssn_aux.hip) per member, the same loops: a
//                                  member's values are the bits its single run gets
//   chain rule through make_W      jds_grad_kernel (ssn_gen.hip) with the member's J, D, 1 / 2S^2, 1 / S^3
//   gradient assembly              per member: dL/dV, the sums of the [B][4][3] partials, the penalty means of the forward's
//                                  per-draw rows, L0 and the loss; one workgroup per member, fp64 in a fixed order
//   optimizer                      optimizer_kernel's update (ssn_critic.hip) for every member's parameter vector, with the
//                                  member's learning rate, regularisation and per-element clip bounds
//   heterogeneous-input stimulus   stimulus_hetero_kernel (ssn_aux.hip) with V of the draw's member
//
// The record: one fp64 row of ssn_ens_record_doubles(D, P) per member -- [L0, m[D], s[D], dynamics_penalty, rate_penalty,
// loss, new parameters[P], gradients[P]] -- is what the host reads back, once per step for the whole ensemble.  An ensemble whose
// loss is not a function of moments (ssn_ens_swd.hip) has D = 0 in its record and hands the gradient assembly its L0 per member.
#include <hip/hip_runtime.h>
#include "ssn_host.h"

namespace ssn {

__device__ __forceinline__ double ens_block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// grid (D, K): sums[k][2][D] of member k's rows x[k B .. (k + 1) B)
__global__ void __launch_bounds__(256) ens_moment_sums_kernel(const float* __restrict__ x, int B, int D, double* __restrict__ sums) {
    const int d = blockIdx.x, k = blockIdx.y;
    const float* xk = x + (size_t)k * B * D;
    double s1 = 0, s2 = 0;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const double v = (double)xk[(size_t)b * D + d];
        s1 += v; s2 += v * v;
    }
    __shared__ double red[2][256];
    red[0][threadIdx.x] = s1; red[1][threadIdx.x] = s2;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (threadIdx.x < off) { red[0][threadIdx.x] += red[0][threadIdx.x + off]; red[1][threadIdx.x] += red[1][threadIdx.x + off]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { sums[(size_t)k * 2 * D + d] = red[0][0]; sums[(size_t)k * 2 * D + D + d] = red[1][0]; }
}

// grid (D, K): gx of member k's rows and m, s of its channels into its record row (rec + k * rstride + 1)
__global__ void __launch_bounds__(256) ens_moment_loss_grad_kernel(const float* __restrict__ x, const double* __restrict__ sums,
                                                                   const double* __restrict__ data_moments,
                                                                   const double* __restrict__ weights, int B, int D,
                                                                   float* __restrict__ gx, double* __restrict__ rec, int rstride) {
    const int d = blockIdx.x, k = blockIdx.y;
    const double Bg = (double)B;
    const double* sk = sums + (size_t)k * 2 * D;
    const double* dm = data_moments + (size_t)k * 2 * D;
    const double* wk = weights + (size_t)k * 2 * D;
    const double m = sk[d] / Bg, s = sk[D + d] / Bg - m * m;
    const double em = m - dm[d], es = s - dm[D + d];
    const double w0 = wk[d], w1 = wk[D + d];
    const double c0 = w0 * em / (Bg * D), c1 = 2.0 * w1 * es / (Bg * D);
    const float* xk = x + (size_t)k * B * D;
    float* gk = gx + (size_t)k * B * D;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const double xv = (double)xk[(size_t)b * D + d];
        gk[(size_t)b * D + d] = (float)(c0 + c1 * (xv - m));
    }
    if (threadIdx.x == 0) { rec[(size_t)k * rstride + 1 + d] = m; rec[(size_t)k * rstride + 1 + D + d] = s; }
}

// grid (K * B * 4): jds_grad_kernel with the member's parameters; p16[k] = J[4], D[4], 1 / (2 S^2)[4], 1 / S^3[4] (fp32, formed
// on the host the way launch_jds_grad forms them)
__global__ void __launch_bounds__(256) ens_jds_grad_kernel(const float* __restrict__ gW, const float* __restrict__ z,
                                                           const float* __restrict__ p16, double* __restrict__ out, int B, int N) {
    const int M = 2 * N;
    const int b = blockIdx.x >> 2, pq = blockIdx.x & 3, pp = pq >> 1, qq = pq & 1;
    const float* p = p16 + (size_t)(b / B) * 16;
    const float Jq = p[pq], Dq = p[4 + pq], inv2s2 = p[8 + pq], inv_s3 = p[12 + pq];
    const float inv_nm1 = (N > 1) ? 1.f / (float)(N - 1) : 0.f;
    const float sgn = qq ? -1.f : 1.f;
    double sj = 0, sd = 0, ss = 0;
    for (int e = threadIdx.x; e < N * N; e += blockDim.x) {
        const int i = e / N, j = e - i * N;
        const size_t o = ((size_t)b * M + pp * N + i) * M + qq * N + j;
        const float dx = (float)(i - j) * inv_nm1;
        const float wnn = exp(-(dx * dx) * inv2s2);
        const float g = gW[o], zz = z[o];
        sj += (double)(g * sgn * wnn);
        sd += (double)(g * sgn * wnn * zz);
        ss += (double)(g * wnn * (sgn * Jq + sgn * Dq * zz) * dx * dx * inv_s3);
    }
    __shared__ double red[3][256];
    red[0][threadIdx.x] = sj; red[1][threadIdx.x] = sd; red[2][threadIdx.x] = ss;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (threadIdx.x < off) {
            red[0][threadIdx.x] += red[0][threadIdx.x + off];
            red[1][threadIdx.x] += red[1][threadIdx.x + off];
            red[2][threadIdx.x] += red[2][threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) out[((size_t)b * 4 + pq) * 3 + threadIdx.x] = red[threadIdx.x][0];
}

// grid (K): member k's flat gradient [dL/dV (nv), dL/dJ (4), dL/dD (4), dL/dS (4)] and its loss.  L0 is
// moment_loss_sum_kernel's tree over the member's channels, or l0[k] where the caller has it; the penalties are the means of the forward's per-draw rows over
// the member's draws, rounded to fp32 as the single run reads them; loss = L0 + dynamics_cost dyn + rate_cost rate.
__global__ void __launch_bounds__(256) ens_gen_grads_kernel(EnsGradsArgs a) {
    __shared__ double red[256];
    const int k = blockIdx.x;
    const int P = a.nv + 12;
    double* rec = a.rec + (size_t)k * a.rstride;
    double L0;
    if (a.l0) {                                       // (the loss kernels formed it: ssn_ens_gen_grads_l0_f32)
        L0 = a.l0[k];
    } else {
        const double* dm = a.data_moments + (size_t)k * 2 * a.D;
        const double* wk = a.weights + (size_t)k * 2 * a.D;
        double t = 0.0;
        for (int d = threadIdx.x; d < a.D; d += 256) {
            const double em = rec[1 + d] - dm[d], es = rec[1 + a.D + d] - dm[a.D + d];
            t += wk[d] * em * em + wk[a.D + d] * es * es;
        }
        L0 = ens_block_sum(t, red) / (2.0 * a.D);
    }
    const long per_member = (long)a.B * a.NB * a.M;
    const size_t row0 = (size_t)k * per_member;
    double sd = 0.0, sr = 0.0;
    for (long e = threadIdx.x; e < per_member; e += 256) { sd += (double)a.dyn_row[row0 + e]; sr += (double)a.rate_row[row0 + e]; }
    const double dyn = ens_block_sum(sd, red) * a.scale_dyn, rate = ens_block_sum(sr, red) * a.scale_rate;
    float* out = a.grads + (size_t)k * P;
    if (a.nv > 0) {
        const int N = a.M / 2;
        const long per_draw = (long)a.NB * a.M;
        double vE = 0.0, vI = 0.0;
        for (long e = threadIdx.x; e < per_member; e += 256) {
            const long b = (long)k * a.B + e / per_draw;
            const int m = (int)(e % a.M);
            const double v = (double)a.g_ext[row0 + e] * (double)a.ext_base[row0 + e] * (double)a.zin[b * a.M + m];
            if (m < N) vE += v; else vI += v;
        }
        const double tE = ens_block_sum(vE, red), tI = ens_block_sum(vI, red);
        if (threadIdx.x == 0) {
            if (a.nv == 1) out[0] = (float)(tE + tI);
            else { out[0] = (float)tE; out[1] = (float)tI; }
        }
    }
    for (int c = 0; c < 12; ++c) {                    // c = 3 q + t of part[b][q][t]; out: J (t = 0), D (1), S (2) blocks of four
        double s = 0.0;
        for (int b = threadIdx.x; b < a.B; b += 256) s += a.part[((size_t)k * a.B + b) * 12 + c];
        const double tot = ens_block_sum(s, red);
        if (threadIdx.x == 0) out[a.nv + (c % 3) * 4 + c / 3] = (float)tot;
    }
    if (threadIdx.x == 0) {
        const float fd = (float)dyn, fr = (float)rate;
        rec[0] = L0;
        rec[1 + 2 * a.D] = (double)fd;
        rec[2 + 2 * a.D] = (double)fr;
        rec[3 + 2 * a.D] = L0 + a.costs[2 * k] * (double)fd + a.costs[2 * k + 1] * (double)fr;
    }
}

// grid over K * P elements: optimizer_kernel's update of every member's parameter vector (kind, betas, epsilon and rho shared;
// learning rate, a_t and the four regularisation weights per member: hyp[k] = lr, a_t, l2_penalty, l1_penalty, l2_decay,
// l1_decay; clip bounds per element).  New values and gradients go to the member's record row.
__global__ void __launch_bounds__(256) ens_apply_kernel(EnsApplyArgs a) {
    const int P = a.P;
    const long n = (long)a.K * P;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += (long)gridDim.x * 256L) {
        const int k = (int)(e / P), i = (int)(e % P);
        const float* h = a.hyp + (size_t)k * 8;
        const float lr = h[0], a_t = h[1], l2_penalty = h[2], l1_penalty = h[3], l2_decay = h[4], l1_decay = h[5];
        const float p0 = a.p[e];
        float g = a.g[e];
        const float g_in = g;
        g += 2.f * l2_penalty * p0 + l1_penalty * ((p0 > 0.f) - (p0 < 0.f));
        float pn;
        if (a.kind == 1) {
            const float m = a.beta1 * a.s1[e] + (1.f - a.beta1) * g;
            const float v = a.beta2 * a.s2[e] + (1.f - a.beta2) * g * g;
            a.s1[e] = m; a.s2[e] = v;
            pn = p0 - a_t * m / (sqrtf(v) + a.eps);
        } else if (a.kind == 2) {
            const float acc = a.rho * a.s1[e] + (1.f - a.rho) * g * g;
            a.s1[e] = acc;
            pn = p0 - lr * g / sqrtf(acc + a.eps);
        } else {
            pn = p0 - lr * g;
        }
        pn -= lr * l2_decay * p0 + lr * l1_decay * ((p0 > 0.f) - (p0 < 0.f));
        if (pn == pn) pn = fminf(fmaxf(pn, a.clip_lo[e]), a.clip_hi[e]);        // (NaN stays NaN, as in optimizer_kernel)
        a.p[e] = pn;
        double* rec = a.rec + (size_t)k * a.rstride + a.rec_off;
        rec[i] = (double)pn;
        rec[P + i] = (double)g_in;
    }
}

// stimulus_hetero_kernel with V of the draw's member: v[k][2] = (V_E, V_I) of member k, draws [k B, (k + 1) B)
__global__ void __launch_bounds__(256) ens_stimulus_hetero_kernel(const float* __restrict__ bw, const float* __restrict__ con,
                                                                  float inv_l, const float* __restrict__ zin,
                                                                  const float* __restrict__ v, int B, int NB,
                                                                  float* __restrict__ ext, int N, long total) {
    const int M = 2 * N;
    const float step = (N > 1) ? 1.f / (float)(N - 1) : 0.f;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
        const int m = (int)(e % M);
        const long bs = e / M;
        const long b = bs / NB;
        const int i = m >= N ? m - N : m;
        const float x = -0.5f + step * (float)i;
        const float hb = bw[bs] * 0.5f;
        const float s1 = 1.f / (1.f + exp(-(x + hb) * inv_l));
        const float s2 = 1.f / (1.f + exp(-(hb - x) * inv_l));
        const float vm = v[(b / B) * 2 + (m >= N ? 1 : 0)];
        float t = vm * zin[b * M + m];
        asm volatile("" : "+v"(t));                      // (the product is rounded before the addition: no contraction into one fma)
        const float gain = 1.f + t;
        ext[e] = gain * con[bs] * s1 * s2;
    }
}

hipError_t launch_ens_moments(const float* x, int K, int B, int D, double* sums, const double* data_moments, const double* weights,
                              float* gx, double* rec, int rstride, hipStream_t st) {
    if (K == 0 || D == 0) return hipSuccess;
    hipLaunchKernelGGL(ens_moment_sums_kernel, dim3(D, K), dim3(256), 0, st, x, B, D, sums);
    hipLaunchKernelGGL(ens_moment_loss_grad_kernel, dim3(D, K), dim3(256), 0, st, x, sums, data_moments, weights, B, D, gx, rec, rstride);
    return hipGetLastError();
}
hipError_t launch_ens_jds_grad(const float* gW, const float* z, const float* p16, double* out, int K, int B, int N, hipStream_t st) {
    if (K == 0 || B == 0) return hipSuccess;
    hipLaunchKernelGGL(ens_jds_grad_kernel, dim3(K * B * 4), dim3(256), 0, st, gW, z, p16, out, B, N);
    return hipGetLastError();
}
hipError_t launch_ens_gen_grads(const EnsGradsArgs& a, hipStream_t st) {
    if (a.K == 0) return hipSuccess;
    hipLaunchKernelGGL(ens_gen_grads_kernel, dim3(a.K), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_ens_apply(const EnsApplyArgs& a, hipStream_t st) {
    const long n = (long)a.K * a.P;
    if (n == 0) return hipSuccess;
    const int blocks = (int)((n + 255) / 256 < 64 ? (n + 255) / 256 : 64);
    hipLaunchKernelGGL(ens_apply_kernel, dim3(blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_ens_stimulus_hetero(const float* bw, const float* con, float smooth, const float* zin, const float* v, float* ext,
                                      int K, int B, int NB, int N, hipStream_t st) {
    const long total = (long)K * B * NB * 2 * N;
    if (total == 0) return hipSuccess;
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(ens_stimulus_hetero_kernel, dim3(blocks), dim3(256), 0, st, bw, con, 1.f / smooth, zin, v, B, NB, ext, N, total);
    return hipGetLastError();
}

}  // namespace ssn
