// Rejection sampling of fixed points on the device (ssnode.sample_tuning_curves_table; analyzers/distdiff.py with
// dynamics='fixed-point'): A parameter sets see the same stream of candidate draws z, every (set, candidate) pair is solved for
// every stimulus by the batched solver, and the first NZ candidates of a set whose solves all succeed are kept -- the rule of
// ssnode.find_fixed_points -- without the states leaving the device.
//
//   W for a table of parameter sets   build_w_table_kernel<T>: the fp64 (and any T) form of ssn_score.hip's kernel of the same
//                                     name.  A thread keeps 4 elements of z in registers and walks the A sets; the constants of a
//                                     set are formed from the device table the way build_w_kernel forms them, the arithmetic is
//                                     w_from_z: the bits of ssn_build_w_f64 called once per set.
//   verdict per (set, candidate)      verdict_kernel: one wave per pair.  It sweeps the pair's NB 2N states once with 16-byte
//                                     loads (a flat walk over the aligned vectors that cover the pair's elements, the elements of
//                                     the neighbours masked off), keeps the largest stimulus index that holds a non-finite value
//                                     and the largest stimulus index whose solver code is not 0, and reduces both over the wave.
//                                     The pair fails at the larger of the two: with that stimulus' code, or with code 1 where the
//                                     code is 0 and the state is not finite ("Converged to non-finite value").  That is the first
//                                     failure in REVERSED stimulus order.  A plain memory sweep: A R NB 2N sizeof(T) bytes.
//   select per set                    select_kernel: one workgroup of 256 threads per set, no atomics.  An ordered exclusive scan
//                                     of (verdict == 0) over the round's candidates in blocks of 256 (64-bit ballot and popcount
//                                     per wave, wave totals through LDS, a running base over the blocks) gives every success
//                                     its rank; rank r is accepted into row have + r while that is below NZ.  The accepted
//                                     candidates' indices go to LDS (that list is what bounds a round: FP_MAX_CANDIDATES), and
//                                     the 256 threads then gather their probed rates, one (row, column) per thread and turn.
//                                     Rejections are counted only in front of the NZ-th success, so the counts do not depend on
//                                     how the candidates were grouped into rounds.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ssn_host.h"

namespace ssn {

constexpr int FP_MAX_CANDIDATES = 8192;        // candidates of one round: 32 KiB of accepted indices in LDS

// grid: blocks of 256 threads over the vectors of z[B][M][M]; dynamic LDS: A JDS<T> records.  table: device T[A][12] (J, D, S)
template <typename T, int VEC>
__global__ void __launch_bounds__(256) build_w_table_kernel(const T* __restrict__ z, const T* __restrict__ table, T* __restrict__ W,
                                                            int A, int N, long total_vec) {
    extern __shared__ double fps_lds[];
    JDS<T>* sets = reinterpret_cast<JDS<T>*>(fps_lds);
    for (int e = threadIdx.x; e < A * 4; e += 256) {
        const int a = e >> 2, q = e & 3;
        const T* p = table + (size_t)a * 12;
        sets[a].J[q] = p[q];
        sets[a].D[q] = p[4 + q];
        const T sg = p[8 + q];
        T two_s2;
        {
#pragma clang fp contract(off)
            two_s2 = (T)2 * sg * sg;
        }
        sets[a].inv2s2[q] = (T)1 / two_s2;
    }
    __syncthreads();
    using V4 = T __attribute__((ext_vector_type(4)));
    const int M = 2 * N;
    const T inv_nm1 = (N > 1) ? (T)1 / (T)(N - 1) : (T)0;
    const long per_set = total_vec * VEC;                     // elements of one set's W[B][M][M]
    for (long v = blockIdx.x * 256L + threadIdx.x; v < total_vec; v += (long)gridDim.x * 256L) {
        const long e0 = v * VEC;
        const int col0 = (int)(e0 % M);
        const int row = (int)((e0 / M) % M);
        T zin[VEC];
        if constexpr (VEC == 4) {
            const V4 q = *reinterpret_cast<const V4*>(z + e0);
            zin[0] = q.x; zin[1] = q.y; zin[2] = q.z; zin[3] = q.w;
        } else {
            zin[0] = z[e0];
        }
        for (int a = 0; a < A; ++a) {
            T w[VEC];
#pragma unroll
            for (int t = 0; t < VEC; ++t) w[t] = w_from_z<T>(sets[a], N, inv_nm1, row, col0 + t, zin[t]);
            T* out = W + (size_t)a * per_set + e0;
            if constexpr (VEC == 4) {
                V4 q; q.x = w[0]; q.y = w[1]; q.z = w[2]; q.w = w[3];
                *reinterpret_cast<V4*>(out) = q;
            } else {
                out[0] = w[0];
            }
        }
    }
}

template <typename T>
__device__ __forceinline__ bool fp_finite(T v) { return fabs(v) < (T)__builtin_huge_val(); }

// grid: blocks of 256 threads = 4 waves, wave g of the grid handles pair g of the `pairs` (set, candidate) pairs.
// codes[pairs][NB], x[pairs][NB][M], verdict[pairs].  VEC = elements of a 16-byte load (x 16-byte aligned), or 1.
template <typename T, int VEC>
__global__ void __launch_bounds__(256) verdict_kernel(const int* __restrict__ codes, const T* __restrict__ x, int* __restrict__ verdict,
                                                      long pairs, int NB, int M) {
    const long g = blockIdx.x * 4L + (threadIdx.x >> 6);
    if (g >= pairs) return;                                   // (wave-uniform; nothing below synchronises the block)
    const int lane = threadIdx.x & 63;
    const long per = (long)NB * M;
    const long e0 = g * per, e1 = e0 + per;                   // the pair's elements of x
    const long total = pairs * per;
    int bad_x = -1;                                           // largest stimulus index with a non-finite value
    using VT = T __attribute__((ext_vector_type(VEC)));
    for (long v = e0 / VEC + lane; v * VEC < e1; v += 64) {
        const long f = v * VEC;                               // first element of this vector; [f, f + VEC) meets [e0, e1)
        T val[VEC];
        if (VEC > 1 && f + VEC <= total) {
            const VT q = *reinterpret_cast<const VT*>(x + f);
#pragma unroll
            for (int t = 0; t < VEC; ++t) val[t] = q[t];
        } else {                                              // the array's last, partial vector (or VEC == 1)
#pragma unroll
            for (int t = 0; t < VEC; ++t) val[t] = f + t < e1 ? x[f + t] : (T)0;
        }
        const long first = f > e0 ? f : e0;
        const int d = (int)(first - e0);                      // (NB M < 2^31: checked by the caller)
        int s = d / M;
        int r = d - s * M;
#pragma unroll
        for (int t = 0; t < VEC; ++t) {
            const long e = f + t;
            if (e >= e0 && e < e1) {
                if (!fp_finite<T>(val[t])) bad_x = s;          // (s only grows along the vector)
                if (++r == M) { r = 0; ++s; }
            }
        }
    }
    int bad_c = -1;                                           // largest stimulus index with a code other than 0
    const int* cg = codes + g * NB;
    for (int s = lane; s < NB; s += 64) if (cg[s] != 0) bad_c = s;
    for (int off = 32; off >= 1; off >>= 1) {
        bad_x = max(bad_x, __shfl_xor(bad_x, off));
        bad_c = max(bad_c, __shfl_xor(bad_c, off));
    }
    if (lane == 0) {
        const int s = max(bad_x, bad_c);
        int out = 0;
        if (s >= 0) {
            const int c = cg[s];
            out = c != 0 ? c : 1;
        }
        verdict[g] = out;
    }
}

// grid (A); 256 threads; static LDS.  verdict[A][R], x[A][R][NB][M]; probes[nprobe]; set_of[A] -> row of the persistent arrays
// out[.][NZ][NB nprobe], accepted[.], used[.], rejections[.][2], draw_index[.][NZ].  cand0: global index of the round's first candidate.
template <typename T>
__global__ void __launch_bounds__(256) select_kernel(const int* __restrict__ verdict, const T* __restrict__ x,
                                                     const int* __restrict__ probes, const int* __restrict__ set_of, int R, int NB,
                                                     int M, int nprobe, int cand0, int NZ, T* __restrict__ out,
                                                     int* __restrict__ accepted, int* __restrict__ used,
                                                     int* __restrict__ rejections, int* __restrict__ draw_index) {
    __shared__ int taken[FP_MAX_CANDIDATES];                  // taken[r]: the round's candidate accepted with rank r
    __shared__ int wtot[4], red[8], last;
    const int a = blockIdx.x, row = set_of[a];
    const int have = accepted[row];
    if (have >= NZ || R <= 0) return;                         // complete before the round (block-uniform)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int room = NZ - have;
    if (tid == 0) last = -1;
    const int* vd = verdict + (size_t)a * R;
    int base = 0, n1 = 0, n2 = 0;
    for (int b0 = 0; b0 < R; b0 += 256) {
        const int b = b0 + tid;
        const int v = b < R ? vd[b] : -1;
        const unsigned long long mask = __ballot(v == 0);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        __syncthreads();                                      // the previous block's wave totals have been read (and `last` is set)
        if (lane == 0) wtot[w] = __popcll(mask);
        __syncthreads();
        int rank = base + before;
        for (int k = 0; k < w; ++k) rank += wtot[k];
        base += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        if (b < R && rank < room) {                           // in front of, or at, the NZ-th success
            if (v == 0) {
                taken[rank] = b;
                draw_index[(size_t)row * NZ + have + rank] = cand0 + b;
                if (rank == room - 1) last = b;
            } else if (v == 1) {
                ++n1;
            } else if (v == 2) {
                ++n2;
            }
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        n1 += __shfl_xor(n1, off);
        n2 += __shfl_xor(n2, off);
    }
    if (lane == 0) { red[w] = n1; red[4 + w] = n2; }
    __syncthreads();                                          // taken, last, red
    const int nacc = base < room ? base : room;
    if (tid == 0) {
        accepted[row] = have + nacc;
        used[row] = last >= 0 ? cand0 + last + 1 : cand0 + R;
        rejections[2 * row] += red[0] + red[1] + red[2] + red[3];
        rejections[2 * row + 1] += red[4] + red[5] + red[6] + red[7];
    }
    const int C = NB * nprobe;
    const T* xa = x + (size_t)a * R * NB * M;
    T* oa = out + ((size_t)row * NZ + have) * C;
    for (int i = tid; i < nacc * C; i += 256) {
        const int r = i / C, c = i - r * C, s = c / nprobe, p = probes[c - s * nprobe];
        if (p >= 0 && p < M) oa[i] = xa[((size_t)taken[r] * NB + s) * M + p];
    }
}

template <typename T>
hipError_t launch_build_w_table_t(const T* z, const T* table, T* W, int A, int B, int N, hipStream_t st) {
    const int M = 2 * N;
    const long total = (long)B * M * M;
    if (total == 0 || A == 0) return hipSuccess;
    const bool vec4 = (M % 4 == 0) && (((uintptr_t)z | (uintptr_t)W) % (4 * sizeof(T)) == 0);   // (every set's W stays aligned)
    const long nvec = vec4 ? total / 4 : total;
    const int blocks = (int)((nvec + 255) / 256 < 256 * 8 ? (nvec + 255) / 256 : 256 * 8);
    const int slice = (int)(49152 / sizeof(JDS<T>));          // sets per launch: 48 KiB of constants in LDS
    for (int a0 = 0; a0 < A; a0 += slice) {
        const int na = A - a0 < slice ? A - a0 : slice;
        const size_t lds = (size_t)na * sizeof(JDS<T>);
        const T* tb = table + (size_t)a0 * 12;
        T* Wa = W + (size_t)a0 * total;
        if (vec4) hipLaunchKernelGGL((build_w_table_kernel<T, 4>), dim3(blocks), dim3(256), lds, st, z, tb, Wa, na, N, nvec);
        else      hipLaunchKernelGGL((build_w_table_kernel<T, 1>), dim3(blocks), dim3(256), lds, st, z, tb, Wa, na, N, nvec);
    }
    return hipGetLastError();
}

hipError_t launch_build_w_table_f64(const double* z, const double* table, double* W, int A, int B, int N, hipStream_t st) {
    return launch_build_w_table_t<double>(z, table, W, A, B, N, st);
}

int fp_select_max_candidates() { return FP_MAX_CANDIDATES; }

template <typename T>
hipError_t launch_fp_select(const FpSelectArgs<T>& a, hipStream_t st) {
    const long pairs = (long)a.A * a.R;
    if (pairs == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((pairs + 3) / 4);
    constexpr int VEC = 16 / sizeof(T);
    if ((uintptr_t)a.x % 16 == 0)
        hipLaunchKernelGGL((verdict_kernel<T, VEC>), dim3(blocks), dim3(256), 0, st, a.codes, a.x, a.verdict, pairs, a.NB, a.M);
    else
        hipLaunchKernelGGL((verdict_kernel<T, 1>), dim3(blocks), dim3(256), 0, st, a.codes, a.x, a.verdict, pairs, a.NB, a.M);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((select_kernel<T>), dim3(a.A), dim3(256), 0, st, a.verdict, a.x, a.probes, a.set_of, a.R, a.NB, a.M, a.nprobe,
                       a.cand0, a.NZ, a.out, a.accepted, a.used, a.rejections, a.draw_index);
    return hipGetLastError();
}
template hipError_t launch_fp_select<float>(const FpSelectArgs<float>&, hipStream_t);
template hipError_t launch_fp_select<double>(const FpSelectArgs<double>&, hipStream_t);

}  // namespace ssn
