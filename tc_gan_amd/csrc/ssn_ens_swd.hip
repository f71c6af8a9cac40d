// Ensembles of sliced Wasserstein runs (networks/sliced_wasserstein_ensemble.py): the loss kernels of ssn_swd.hip over K members
// in one launch each.  Member k owns rows [k B, (k + 1) B) of x[K B][D] and y[K B][D], its own directions theta[k][L][D] and its
// own power; L, B and D are shared.  Every kernel body is the single-run kernel's (ssn_swd_dev.h) on the member's base pointers,
// so a member's px, py, coef, loss_l and gx are the bits ssn_project_rows_f32, ssn_swd_match_f32 and ssn_swd_backproject_f32 give
// for that member alone, and a value that is not finite in one member reaches no other member.
//
//   project      ens_swd_project_kernel, grid (direction tiles, row tiles, 2 K): z = 2 k + sample (0: x, 1: y).
//   match        two forms behind one launcher, both followed by ens_swd_l0_kernel:
//                general, any B: ens_swd_match_kernel, grid (L, K), swd_match_body -- the LDS bitonic network.
//                wave, B <= 64:  ens_swd_match_wave_kernel, one wave64 per (member, direction) column, four columns per workgroup.
//                Lane i loads row i: the key (ordered float, row) and the y value stay in registers, lanes >= B carry the padding
//                (key ~0, y = +inf).  The network for 64 elements -- the general form's at P = 64, the same compare-exchange
//                rule on the same pairs -- runs as 21 stages over cross-lane moves: DPP for the distances 1, 2 (quad_perm),
//                4 (quad_perm then row_half_mirror) and 8 (row_ror:8), __shfl_xor for 16 and 32.  No LDS array, no barrier.
//                Lane i < B then holds rank i: one term per lane, added lanes 32 ... 1 apart as the general form's wave
//                reduction does; there, for B <= 64, a thread has at most one term and the waves 1 .. 3 add +0, so order and
//                bits are the same.
//   l0           ens_swd_l0_kernel, one thread per member: l0[k] = (sum_l loss_l[k][l]) / L, sequential in index order.
//   backproject  ens_swd_backproject_kernel, grid (column tiles, row tiles, K): swd_backproject_body.
//
// The members' powers come as one bit each in the kernel arguments (SwdPowerBits): the host checks them, nothing is uploaded.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ssn_host.h"
#include "ssn_swd_dev.h"

namespace ssn {

__device__ __forceinline__ int swd_power_of(const SwdPowerBits& bits, int k) { return ((bits.w[k >> 5] >> (k & 31)) & 1u) ? 2 : 1; }

__global__ void __launch_bounds__(256) ens_swd_project_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                              const float* __restrict__ theta, int B, int L, int D,
                                                              float* __restrict__ px, float* __restrict__ py) {
    const int k = blockIdx.z >> 1;
    const float* src = ((blockIdx.z & 1) ? y : x) + (size_t)k * B * D;
    float* out = ((blockIdx.z & 1) ? py : px) + (size_t)k * B * L;
    project_rows_body(src, B, D, D, theta + (size_t)k * L * D, L, out, blockIdx.x * PJ_DIRS, blockIdx.y, gridDim.y);
}

// grid (L, K); dynamic LDS as swd_match_kernel
__global__ void __launch_bounds__(256) ens_swd_match_kernel(const float* __restrict__ px, const float* __restrict__ py, int B, int L,
                                                            int P, SwdPowerBits powers, double inv, float* __restrict__ coef,
                                                            double* __restrict__ loss_l) {
    const int k = blockIdx.y;
    const size_t o = (size_t)k * B * L;
    swd_match_body(px + o, py + o, B, L, P, swd_power_of(powers, k), inv, coef + o, loss_l + (size_t)k * L, blockIdx.x);
}

template <int CTRL>
__device__ __forceinline__ uint32_t swd_dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, false);
}
// the value of lane (lane ^ J); every lane of the wave is active
template <int J>
__device__ __forceinline__ uint32_t swd_lane_xor(uint32_t v) {
    if constexpr (J == 1) return swd_dpp<0xB1>(v);                       // quad_perm [1, 0, 3, 2]
    else if constexpr (J == 2) return swd_dpp<0x4E>(v);                  // quad_perm [2, 3, 0, 1]
    else if constexpr (J == 4) return swd_dpp<0x141>(swd_dpp<0x1B>(v));  // quad_perm [3, 2, 1, 0] (^3), row_half_mirror (^7)
    else if constexpr (J == 8) return swd_dpp<0x128>(v);                 // row_ror:8
    else return (uint32_t)__shfl_xor((int)v, J);
}

// one compare-exchange stage of the bitonic network (block size K, distance J) on the pair (lane & ~J, lane | J): the rule of
// cmp_exchange (ssn_sortcol_dev.h), a = the value at the lower index, b = at the upper, exchanged where (a > b) == up
template <int K, int J>
__device__ __forceinline__ void swd_wave_stage(uint32_t& hi, uint32_t& lo, float& y, int lane) {
    const uint32_t ohi = swd_lane_xor<J>(hi), olo = swd_lane_xor<J>(lo);
    const float oy = __uint_as_float(swd_lane_xor<J>(__float_as_uint(y)));
    const bool lower = (lane & J) == 0, up = (lane & K) == 0;
    const unsigned long long mine = ((unsigned long long)hi << 32) | lo, other = ((unsigned long long)ohi << 32) | olo;
    const bool key_gt = lower ? (mine > other) : (other > mine);
    if (key_gt == up) { hi = ohi; lo = olo; }
    const bool y_gt = lower ? (y > oy) : (oy > y);
    if (y_gt == up) y = oy;
}
template <int K, int J>
__device__ __forceinline__ void swd_wave_merge(uint32_t& hi, uint32_t& lo, float& y, int lane) {
    swd_wave_stage<K, J>(hi, lo, y, lane);
    if constexpr (J > 1) swd_wave_merge<K, J / 2>(hi, lo, y, lane);
}
template <int K>
__device__ __forceinline__ void swd_wave_sort(uint32_t& hi, uint32_t& lo, float& y, int lane) {
    if constexpr (K > 2) swd_wave_sort<K / 2>(hi, lo, y, lane);
    swd_wave_merge<K, K / 2>(hi, lo, y, lane);
}

// grid (ceil(K L / 4)): wave w of a workgroup owns column 4 blockIdx.x + w = k L + l.  B <= 64
__global__ void __launch_bounds__(256) ens_swd_match_wave_kernel(const float* __restrict__ px, const float* __restrict__ py, int B,
                                                                 int L, int columns, SwdPowerBits powers, double inv,
                                                                 float* __restrict__ coef, double* __restrict__ loss_l) {
    const int lane = threadIdx.x & 63;
    const int col = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= columns) return;                               // (the whole wave)
    const int k = col / L, l = col - k * L;
    const size_t o = (size_t)k * B * L;
    const float inf = __builtin_huge_valf();
    uint32_t hi = ~0u, lo = ~0u;                              // (above the key of +inf: the padding sorts last)
    float y = inf;
    bool mine = false;
    if (lane < B) {
        const float u = px[o + (size_t)lane * L + l];
        y = py[o + (size_t)lane * L + l];
        mine = !(fabsf(u) < inf) || !(fabsf(y) < inf);
        hi = swd_ordered(u);
        lo = (uint32_t)lane;
    }
    if (__any(mine)) {                                        // NaN, +inf or -inf in either column: nothing is sorted
        if (lane < B) coef[o + (size_t)lane * L + l] = __builtin_nanf("");
        if (lane == 0) loss_l[col] = __builtin_nan("");
        return;
    }
    swd_wave_sort<64>(hi, lo, y, lane);
    double sum = 0.0;
    if (lane < B) {
        const double d = (double)swd_unordered(hi) - (double)y;
        double term, cf;
        swd_rank_term(d, swd_power_of(powers, k), inv, term, cf);
        sum += term;
        if ((int)lo < B) coef[o + (size_t)lo * L + l] = (float)cf;       // (the first B ranks are rows)
    }
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);  // (wave_sum_in_order's text: through the call, 23 VGPRs)
    if (lane == 0) loss_l[col] = sum / (double)B;
}

// one thread per member: the sequential sum of its loss_l in index order, divided by L
__global__ void __launch_bounds__(256) ens_swd_l0_kernel(const double* __restrict__ loss_l, int K, int L, double* __restrict__ l0) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    double s = loss_l[(size_t)k * L];
    for (int l = 1; l < L; ++l) s += loss_l[(size_t)k * L + l];
    l0[k] = s / (double)L;
}

// grid (column tiles, row tiles, K)
__global__ void __launch_bounds__(256) ens_swd_backproject_kernel(const float* __restrict__ coef, const float* __restrict__ theta,
                                                                  int B, int L, int D, float* __restrict__ gx) {
    const int k = blockIdx.z;
    swd_backproject_body(coef + (size_t)k * B * L, theta + (size_t)k * L * D, B, L, D, gx + (size_t)k * B * D, blockIdx.x * BP_COLS,
                         blockIdx.y, gridDim.y);
}

hipError_t launch_ens_swd_project(const float* x, const float* y, const float* theta, int K, int B, int L, int D, float* px, float* py,
                                  hipStream_t st) {
    if (K == 0 || B == 0 || L == 0) return hipSuccess;
    const int tiles = (B + PJ_ROWS - 1) / PJ_ROWS;
    hipLaunchKernelGGL(ens_swd_project_kernel, dim3((L + PJ_DIRS - 1) / PJ_DIRS, tiles, 2 * K), dim3(256), 0, st, x, y, theta, B, L, D,
                       px, py);
    return hipGetLastError();
}

hipError_t launch_ens_swd_match(const float* px, const float* py, const SwdPowerBits& powers, int K, int B, int L, int form, float* coef,
                                double* loss_l, double* l0, hipStream_t st) {
    if (K == 0 || B == 0 || L == 0) return hipSuccess;
    const double inv = 1.0 / ((double)L * (double)B);
    if (form == SWD_FORM_WAVE || (form == SWD_FORM_AUTO && B <= SWD_WAVE_MAX_BATCH)) {
        const int columns = K * L;
        hipLaunchKernelGGL(ens_swd_match_wave_kernel, dim3((columns + 3) / 4), dim3(256), 0, st, px, py, B, L, columns, powers, inv, coef,
                           loss_l);
    } else {
        const int P = sort_slots(B);
        hipLaunchKernelGGL(ens_swd_match_kernel, dim3(L, K), dim3(256), (size_t)P * (sizeof(unsigned long long) + sizeof(float)), st, px,
                           py, B, L, P, powers, inv, coef, loss_l);
    }
    hipLaunchKernelGGL(ens_swd_l0_kernel, dim3((K + 255) / 256), dim3(256), 0, st, loss_l, K, L, l0);
    return hipGetLastError();
}

hipError_t launch_ens_swd_backproject(const float* coef, const float* theta, int K, int B, int L, int D, float* gx, hipStream_t st) {
    if (K == 0 || B == 0 || D == 0) return hipSuccess;
    const int tiles = (B + BP_ROWS - 1) / BP_ROWS;
    hipLaunchKernelGGL(ens_swd_backproject_kernel, dim3((D + BP_COLS - 1) / BP_COLS, tiles, K), dim3(256), 0, st, coef, theta, B, L, D,
                       gx);
    return hipGetLastError();
}

}  // namespace ssn
