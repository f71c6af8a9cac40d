// Two weight draws per workgroup, every wave both roles: the SSN recurrence for NB >= 4 stimuli per draw on the fp16
// matrix cores (exact-product split, see ssn_mfma16.hip) with the chain of one draw hidden behind the serial part of
// the other.
//
// ssn_mfma16.hip's wide form puts all 8 stimuli of a draw into the 16 operand columns of v_mfma_f32_16x16x32_f16 (column s
// = r_h, column 8 + s = r_m of stimulus s), which halves the matrix work of the alternating form but leaves nothing to
// alternate with: a step there is [chain] barrier [serial part] barrier, matrix waves and serial waves take turns and the
// matrix pipe idles two thirds of the time.  Here the second unit of work is a second DRAW:
//
//   workgroup = 8 waves = 2 draws x 4 waves; waves w and w + 4 share a SIMD and belong to different draws;
//   every wave holds its quarter of its draw's W (two fp16 parts, 22-23 tiles of 16 x 32, 184 registers) for the whole
//   launch AND finishes the rows of the row tiles it completes: in even phases the waves of draw 0 run their chains
//   while the waves of draw 1 run their serial parts (nonlinearity, Euler update, reductions, split of the new state),
//   in odd phases the other way round, ONE s_barrier per phase.  Each SIMD therefore always has one wave on the matrix
//   pipe and one on the vector pipe.
//
//   No round trip of the sums through LDS: the wave that ran a row tile's chain keeps the accumulators in registers
//   across the barrier and finishes them itself.  In the accumulator layout lane (lg, li) holds rows 4 lg .. 4 lg + 3 of
//   column li; columns s and 8 + s are the two parts of stimulus s, so one DPP row rotate by 8 adds them and the two
//   lanes share the four rows: lane s finishes rows 4 lg, 4 lg + 1, lane 8 + s rows 4 lg + 2, 4 lg + 3 -- every lane two
//   rows per row tile, 6 or 8 values per step.  Only a row tile whose k range is split between two neighbouring waves
//   (3 of 13 at 2N = 200, the price of an even deal of the 91 tiles) sends one partial sum through LDS, written at the end
//   of the chain phase and read behind the barrier in the serial phase of the same draw.
//   The new state goes to LDS as two fp16 parts by ROUND TO NEAREST (h = rn(s), m = rn(s - h): |s - h - m| <= 2^-23 |s|;
//   v_cvt_pk_f16_f32), where the four waves of the draw read it as their B operand in the next chain phase.
//
// Same arithmetic per step as the other forms (accumulation fp32, W = W_h + W_m by round to nearest, one power-of-two scale
// per draw from max |W|, state scale from the rate bound of the saturating I/O function: asym_tanh only).
#include "ssn_duo_core.h"

namespace ssn {

// Diagnostic build (SSN_DUO_STAMP): the kernel that ran last leaves, for every wave w = 4 draw + wave of workgroup 0, its
// DuoStamp row in duo_stamps[8 w ..].  Segments -- forward (steps before the window): chain, early tile, barrier, rest of the
// serial part, publication, barrier; solver: chain + early tile, verdict, barrier, serial part, barrier; adjoint sweep (steps
// after the window): serial part, barrier, chain (+ early tile), barrier.
using Stamp = DuoStamp<SSN_DUO_STAMP != 0>;
#if SSN_DUO_STAMP
__device__ unsigned long long duo_stamps[64];
__device__ __forceinline__ unsigned long long* duo_stamp_row(int w) { return duo_stamps + 8 * w; }
#else
__device__ __forceinline__ unsigned long long* duo_stamp_row(int) { return nullptr; }
#endif

template <int MK, int WV, bool SAVE, bool FREE, bool HT>
__device__ __forceinline__ void duo_forward_wave(const GenFwdArgs<float>& a, int rshift, int d, int b, int s0, bool valid,
                                                 int lane, char* dlds, unsigned* wmax) {
    using S = Duo16<MK>;
    using WS = DuoWave<MK, WV>;
    constexpr int NT = WS::NT, NTF = WS::NTF, RT0 = WS::RT0;
    constexpr bool HTW = HT && WV == S::WM - 1 && NTF > 1;       // this wave finishes the half-real tail tile one value per lane
    constexpr int NP = HTW ? NTF - 1 : NTF;                      // row tiles finished as row pairs
    constexpr int NE = 2 * NP + (HTW ? 1 : 0);
    const int M = a.M, N = a.M / 2, T_ = a.seqlen;
    const int li = lane & 15, lg = lane >> 4, hi = li >> 3, st = li & 7;
    const int row_tail = 16 * (RT0 + NTF - 1) + 4 * (lg & 1) + 2 * hi + (lg >> 1);
    auto row_of = [&](int i) { return (HTW && i == NE - 1) ? row_tail : 16 * (RT0 + i / 2) + 4 * lg + 2 * hi + (i & 1); };
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.W + (size_t)b * M * M), 0, M * M * 4, 0x00020000);
    // ---- W, read once: max |W| of the draw, then the two fp16 parts of W 2^a (every unit in registers: Duo16)
    using Ops = DuoOperands<MK, WV, 0>;
    typename Ops::Raw raw;
    atomicMax(wmax, __builtin_bit_cast(unsigned, Ops::fetch(rsrc, M, li, lg, raw)));
    __syncthreads();                                                          // (A)
    const int wexp = duo_w_exp(*wmax);
    const float sa = duo_pow2(wexp), usc = duo_pow2(-wexp - rshift), rs = duo_pow2(rshift);
    Ops ops;
    ops.split(raw, sa, nullptr, lane);
    // ---- the values this lane finishes: row tile RT0 + tf, rows 4 lg + 2 hi + e, stimulus s0 + st
    const IoSelect io(a.io);
    const int s = s0 + st;
    const bool live = valid && s < a.NB;
    float rc[NE], ex[NE], eps[NE], ta[NE];
    float dps = 0.f, rps = 0.f;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const int row = row_of(i);
        rc[i] = ta[i] = 0.f;
        ex[i] = (s < a.NB && row < M) ? a.ext[((size_t)b * a.NB + s) * M + row] : 0.f;
        eps[i] = row < N ? a.eps_E : a.eps_I;
    }
    const size_t blk_elems = (size_t)a.NB * T_ * M;
    __amdgpu_buffer_rsrc_t rs_traj, rs_df;
    int toff = -1;                               // byte offset of (my stimulus, step 0, row 4 lg + 2 hi) within this draw's block
    if constexpr (SAVE) {
        rs_traj = __builtin_amdgcn_make_buffer_rsrc(a.traj + (size_t)b * blk_elems, 0, (int)(blk_elems * 4), 0x00020000);
        rs_df = __builtin_amdgcn_make_buffer_rsrc(a.df + (size_t)b * blk_elems, 0, (int)(blk_elems * 4), 0x00020000);
        toff = live ? (int)(((size_t)s * T_ * M + 4 * lg + 2 * hi) * 4) : -1;
    }
    const int toff_tail = (SAVE && live && row_tail < M) ? (int)(((size_t)s * T_ * M + row_tail) * 4) : -1;
    using LdsH8 = const __attribute__((address_space(3))) hv8*;
    using LdsF4 = __attribute__((address_space(3))) mf4*;
    using LdsU = __attribute__((address_space(3))) unsigned*;
    using LdsH = __attribute__((address_space(3))) unsigned short*;
    const unsigned bimg = (unsigned)(size_t)(LdsH8)dlds;
    const unsigned xs = bimg + (unsigned)(2 * S::BB) + (unsigned)(lane * 16);             // + slot * XS
    const unsigned b_rd = bimg + (unsigned)(lg * S::BROW + li * 16);                      // + kt * 4 * BROW
    // new state of rows 16 rt + 4 lg + 2 hi + {0, 1}: k tile rt / 2, k octet 2 (rt & 1) + lg / 2, element 4 (lg & 1) + 2 hi
    const unsigned b_wr = bimg + (unsigned)((lg >> 1) * S::BROW + st * 16 + (lg & 1) * 8 + hi * 4);
    // the tail value (row 16 rt + 4 (lg & 1) + 2 hi + (lg >> 1)): k octet 2 (rt & 1), element 4 (lg & 1) + 2 hi + (lg >> 1)
    const unsigned b_wr_tail = bimg + (unsigned)(st * 16 + (lg & 1) * 8 + hi * 4 + (lg >> 1) * 2);

    const unsigned sync = bimg + (unsigned)S::SYNC;
    bool dead = false;
    mf4 acc[NT];
    auto chain = [&](int it) {
        // free-running form: all four waves of the draw must have stored the state of step it - 1 (image it & 1)
        if (FREE && it > 0) duo_wait_ge(sync, S::WM * it, dead);
        ops.chain(b_rd + (FREE ? (unsigned)((it & 1) * S::BB) : 0u), acc);
        if constexpr (WS::TAIL_SHARED) {
            *(LdsF4)(size_t)(xs + (unsigned)(WV * S::XS)) = acc[NT - 1];
            if (FREE) duo_signal_set(sync + 4u * (1 + WV), (unsigned)(it + 1), lane);
        }
    };
    // The serial part of a step, in two pieces.  `compute(T0, T1, TAIL)` finishes the row tiles [T0, T1) (and the tail value):
    // join of the two parts of every sum, f(u), Euler step, window sums, trajectory stores -- registers and global memory
    // only.  `publish` splits the new state and writes it to the B image.  The wave that has just ended its chain would idle
    // until the partner wave of its SIMD is through a serial part that runs at about half speed beside the MFMA stream, so
    // it computes its last EARLY row tiles right behind its own chain, in the same phase (their sums are complete, nothing
    // they need lives in LDS); what stays for its serial phase is the rest and the publication of all tiles.
    auto compute = [&](auto WIN, int it, auto T0_, auto T1_, auto TAIL_) {
        constexpr bool win_on = decltype(WIN)::value;
        constexpr int T0 = decltype(T0_)::value, T1 = decltype(T1_)::value;
        constexpr bool TAIL = decltype(TAIL_)::value;
        constexpr int NV = 2 * (T1 - T0) + (TAIL ? 1 : 0);
        if constexpr (NV > 0) {
            auto gi = [&](int jv) { return (TAIL && jv == NV - 1) ? NE - 1 : 2 * T0 + jv; };       // local value -> lane value
            float uu[NV], ff[NV], dfn[NV];
#pragma unroll
            for (int tf = T0; tf < T1 + (TAIL ? 1 : 0); ++tf) {
                const bool is_tail = TAIL && tf == T1;
                mf4 sm = acc[is_tail ? NTF - 1 : tf];
                if constexpr (WS::HEAD_SHARED) {
                    if (tf == 0 && !is_tail) {
                        if (FREE) duo_wait_ge(sync + 4u * WV, it + 1, dead);          // wave WV - 1 has stored its partial sum of step it
                        const mf4 xp = *(LdsF4)(size_t)(xs + (unsigned)((WV - 1) * S::XS));
                        sm.x += xp.x; sm.y += xp.y; sm.z += xp.z; sm.w += xp.w;
                    }
                }
                // lane s (hi = 0) finishes rows 0, 1, lane 8 + s rows 2, 3 (duo_join)
                const float j0 = tf == T0 ? duo_join<true>(sm.x, sm.z, hi) : duo_join<false>(sm.x, sm.z, hi);
                const float j1 = duo_join(sm.y, sm.w, hi);
                if (is_tail) {
                    uu[NV - 1] = fmaf(duo_tail_take(j0, j1), usc, ex[NE - 1]);
                } else {
                    uu[2 * (tf - T0)] = fmaf(j0, usc, ex[2 * tf]);
                    uu[2 * (tf - T0) + 1] = fmaf(j1, usc, ex[2 * tf + 1]);
                }
            }
#pragma unroll
            for (int jv = 0; jv < NV; ++jv) dfn[jv] = 0.f;
            duo_eval<SAVE, NV>(io, uu, ff, dfn);
            const float win2 = (it > a.skip) ? 1.f : 0.f;
#pragma unroll
            for (int jv = 0; jv < NV; ++jv) {
                const int i = gi(jv);
                const float r1 = fmaf(eps[i], ff[jv] - rc[i], rc[i]);                 // (1 - eps) r + eps f(u)
                const float dd = r1 - rc[i];
                if constexpr (win_on) {
                    ta[i] += r1;
                    rps += fmaxf(r1 - a.theta, 0.f);
                    dps = fmaf(win2 * dd, dd, dps);
                }
                rc[i] = r1;
            }
            if constexpr (SAVE) {
#pragma unroll
                for (int tf = T0; tf < T1; ++tf) {
                    const int rt = RT0 + tf;
                    // (a layout in which every wave stores 512 contiguous bytes ran at 5.19-5.20 against 5.24-5.46 ms: DESIGN 3.13c)
                    const int off = (toff < 0 || 16 * rt + 4 * lg + 2 * hi >= M) ? -1 : toff + (it * M + 16 * rt) * 4;
                    const fv2 rv = {rc[2 * tf], rc[2 * tf + 1]}, dv = {dfn[2 * (tf - T0)], dfn[2 * (tf - T0) + 1]};
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(unsigned __attribute__((ext_vector_type(2))), rv), rs_traj, off, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(unsigned __attribute__((ext_vector_type(2))), dv), rs_df, off, 0, 0);
                }
                if constexpr (TAIL) {
                    const int off = toff_tail < 0 ? -1 : toff_tail + it * M * 4;
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, rc[NE - 1]), rs_traj, off, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, dfn[NV - 1]), rs_df, off, 0, 0);
                }
            }
        }
    };
    auto publish = [&](int it) {
#pragma unroll
        for (int tf = 0; tf < NP; ++tf) {
            const int rt = RT0 + tf;
            unsigned h, m;
            duo_split2(rc[2 * tf], rc[2 * tf + 1], rs, h, m);
            const unsigned wr = b_wr + (unsigned)(((rt >> 1) * 4 + 2 * (rt & 1)) * S::BROW) + (FREE ? (unsigned)(((it + 1) & 1) * S::BB) : 0u);
            *(LdsU)(size_t)wr = h;
            *(LdsU)(size_t)(wr + 128u) = m;
        }
        if constexpr (HTW) {
            constexpr int rt = RT0 + NTF - 1;
            unsigned h, m;
            duo_split2(rc[NE - 1], 0.f, rs, h, m);
            const unsigned wr = b_wr_tail + (unsigned)(((rt >> 1) * 4 + 2 * (rt & 1)) * S::BROW) + (FREE ? (unsigned)(((it + 1) & 1) * S::BB) : 0u);
            *(LdsH)(size_t)wr = (unsigned short)h;
            *(LdsH)(size_t)(wr + 128u) = (unsigned short)m;
        }
        if (FREE) duo_signal_add(sync, lane);
    };
    // row tiles finished behind the own chain: the last ones (never the first, which may wait for a neighbour's partial sum)
    constexpr int EARLY = FREE ? 0 : (S::EARLY < NP - 1 ? S::EARLY : NP - 1);
    constexpr std::integral_constant<int, 0> TB{};
    constexpr std::integral_constant<int, NP - EARLY> TM{};
    constexpr std::integral_constant<int, NP> TE{};
    constexpr std::integral_constant<bool, HTW> HAS_TAIL{};
    constexpr std::integral_constant<bool, false> NO_TAIL{};
    auto early = [&](auto WIN, int it) { compute(WIN, it, TM, TE, NO_TAIL); };
    auto serial = [&](auto WIN, int it) {
        compute(WIN, it, TB, TM, HAS_TAIL);
        publish(it);
    };
    constexpr std::integral_constant<bool, false> W0{};
    constexpr std::integral_constant<bool, true> W1{};
    const int nskip = a.skip < T_ ? (a.skip > 0 ? a.skip : 0) : T_;
    __syncthreads();                                                          // (B)
    if constexpr (FREE) {
        // no workgroup barrier from here on: the four waves of a draw meet at their own counters, the two draws drift
        for (int it = 0; it < nskip; ++it) { chain(it); serial(W0, it); }
        for (int it = nskip; it < T_; ++it) { chain(it); serial(W1, it); }
    } else {
        if (d) __syncthreads();                        // draw 1 runs one phase behind draw 0
        Stamp ts;                                      // (the steps before the window, the serial part as its two pieces)
        ts.start();
        for (int it = 0; it < nskip; ++it) {
            chain(it);
            ts.lap(0);
            early(W0, it);
            ts.lap(1);
            duo_phase_barrier();
            ts.lap(2);
            compute(W0, it, TB, TM, HAS_TAIL);
            ts.lap(3);
            publish(it);
            ts.lap(4);
            duo_phase_barrier();
            ts.lap(5);
            ts.tick();
        }
        ts.flush(duo_stamp_row(4 * d + WV));
        for (int it = nskip; it < T_; ++it) {
            chain(it);
            early(W1, it);
            duo_phase_barrier();
            serial(W1, it);
            duo_phase_barrier();
        }
        if (!d) __syncthreads();
    }

    if (!live) return;
    const float inv = dead ? __builtin_nanf("") : 1.f / (float)(T_ - a.skip);
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const int row = row_of(i);
        if (row >= M) continue;
        const size_t o = ((size_t)b * a.NB + s) * M + row;
        a.time_avg[o] = ta[i] * inv;
        // window sums of (x_{t+1} - x_t)^2 and relu(x_t - theta): this lane's total over its rows, booked on its first row
        a.dyn_row[o] = i == 0 ? dps : 0.f;
        a.rate_row[o] = i == 0 ? rps : 0.f;
    }
}

// grid: ceil(units / 2) workgroups, unit = (draw, group of 8 stimuli); 512 threads
template <int MK, bool SAVE, bool FREE, bool HT>
__global__ void __launch_bounds__(512, 2) gen_forward_duo_kernel(GenFwdArgs<float> a, int rshift) {
    using S = Duo16<MK>;
    __shared__ __align__(16) char lds[S::LDS + 16];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (uniform: buffer descriptors stay in SGPRs)
    const int d = wave >> 2;
    const int ngroups = (a.NB + 7) / 8;
    const long nunits = (long)a.B * ngroups;
    long unit = 2L * blockIdx.x + d;
    const bool valid = unit < nunits;
    if (!valid) unit = nunits - 1;                  // an odd unit count: the idle half repeats the last unit and stores nothing
    const int b = (int)(unit / ngroups), s0 = (int)(unit % ngroups) * 8;
    for (int c = threadIdx.x; c < S::LDS / 4; c += blockDim.x) reinterpret_cast<unsigned*>(lds)[c] = 0u;
    __syncthreads();                                // (zeroed before any wave records max |W|; state 0 = the B images)
    char* const dlds = lds + d * S::DRAW;
    unsigned* const wmax = reinterpret_cast<unsigned*>(lds + 2 * S::DRAW) + d;
    switch (wave & 3) {
        case 0: duo_forward_wave<MK, 0, SAVE, FREE, HT>(a, rshift, d, b, s0, valid, lane, dlds, wmax); break;
        case 1: duo_forward_wave<MK, 1, SAVE, FREE, HT>(a, rshift, d, b, s0, valid, lane, dlds, wmax); break;
        case 2: duo_forward_wave<MK, 2, SAVE, FREE, HT>(a, rshift, d, b, s0, valid, lane, dlds, wmax); break;
        default: duo_forward_wave<MK, 3, SAVE, FREE, HT>(a, rshift, d, b, s0, valid, lane, dlds, wmax); break;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The fixed-point solver (ext/ssnode.c:64-187 semantics: Euler form r + (-r + f(u)) dt / tau, convergence and rate-bound
// tests per step, every (draw, stimulus) pair stops at its own step) in the two-draw form, lock-step phases.
// Stop protocol as solve_mfma_kernel / solve_split_kernel: per draw three rotating flag words per stimulus in LDS (low
// half: some row not converged; high half: some row at the rate bound), written in the serial phase of step t, read by
// all four waves of the draw at the start of its next chain phase (one barrier later), cleared one step ahead.  A draw
// whose 8 stimuli are all frozen (or that reached max_iter) idles through the phases until the other draw of the
// workgroup is done too: each draw publishes `finished` in a word of the slot of the current phase parity, every wave
// reads both words of the previous phase's slot with its flag read and leaves the loop at the END of the phase in which
// it saw both set -- the same decision in all 8 waves, because nobody writes the slot being read.
// ---------------------------------------------------------------------------------------------------------------
template <int MK, int WV>
__device__ __forceinline__ void duo_solve_wave(const SolveArgs<float>& a, int d, int b, int s0, bool valid, int lane,
                                               char* dlds, char* wlds, char* plds, char* wwlds) {
    using S = Duo16<MK>;
    using WS = DuoWave<MK, WV>;
    constexpr int NT = WS::NT, NTF = WS::NTF, RT0 = WS::RT0;
    constexpr int NE = 2 * NTF;
    const int M = a.M, N = a.N, max_iter = a.st.max_iter;
    const int li = lane & 15, lg = lane >> 4, hi = li >> 3, st = li & 7;
    using LdsW = __attribute__((address_space(3))) unsigned*;
    using LdsI = __attribute__((address_space(3))) int*;
    const LdsW wmax = (LdsW)wlds + 2 * d;                                        // [0] max |W|, [1] max |r0| of this draw
    const LdsW done = (LdsW)wlds + 4;                                           // [phase parity][draw]
    // stop flags of this draw: three rotating words, one per step (bits 0-7: stimulus st has a row that is not converged,
    // bits 8-15: ... a row at the rate bound).  A wave folds its lanes' verdicts with one ballot and ORs ONE word in (round 3
    // had every lane store its own 16-bit flag: up to 8 lanes per address and instruction, 2.2e7 bank-conflict cycles per launch)
    const LdsI flags = (LdsI)(dlds + S::SYNC);
    // previous state of this lane's values (r_prev output): kept in LDS, 32 B per lane, rewritten with every applied step
    using LdsF4s = __attribute__((address_space(3))) mf4*;
    const LdsF4s rp_slot = (LdsF4s)(plds + (size_t)WV * 2048 + (size_t)lane * 16);     // second half 1 KB further: conflict-free 16-byte stores
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.W + (size_t)b * M * M), 0, M * M * 4, 0x00020000);
    using Ops = DuoOperands<MK, WV, S::nl_solve()>;
    // (W in two passes, max_abs here and load behind barrier (A): see DuoOperands)
    __hip_atomic_fetch_max(wmax, __builtin_bit_cast(unsigned, Ops::max_abs(rsrc, M, li, lg)), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
    // ---- the values this lane finishes
    const IoSelect io(a.io);
    const int s = s0 + st;
    const bool live = valid && s < a.NB;
    // (max |r0| comes from a first read of the lane's 6-8 values, the state, input and constants from a second one)
    float rc[NE], ex[NE], eps[NE];
    float r0max = 0.f;
    auto read_values = [&](bool keep) {
        const size_t vec = ((size_t)b * a.NB + (s < a.NB ? s : 0)) * M;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const int row = 16 * (RT0 + i / 2) + 4 * lg + 2 * hi + (i & 1);
            const bool ok = s < a.NB && row < M;
            const float r0 = ok ? a.r[vec + row] : 0.f;
            if (keep) {
                rc[i] = r0;
                ex[i] = ok ? a.ext[(a.ext_per_draw ? vec : (size_t)s * M) + row] : 0.f;
                eps[i] = row < N ? a.st.eps_E : a.st.eps_I;
            } else {
                r0max = fmaxf(r0max, __builtin_fabsf(r0));
            }
        }
    };
    read_values(false);
    read_values(true);
    __hip_atomic_fetch_max(wmax + 1, __builtin_bit_cast(unsigned, r0max), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    auto store_prev = [&]() {
        rp_slot[0] = (mf4){rc[0], rc[1], NE > 2 ? rc[2 % NE] : 0.f, NE > 2 ? rc[3 % NE] : 0.f};
        if constexpr (NE > 4) rp_slot[64] = (mf4){rc[4 % NE], rc[5 % NE], NE > 6 ? rc[6 % NE] : 0.f, NE > 6 ? rc[7 % NE] : 0.f};
    };
    store_prev();                                        // (zero steps: previous = initial state; a slot only its own lane reads)
    __syncthreads();                                                          // (A) max |W|, max |r0| of both draws
    // state scale: bound 2^rshift < 2^14 for bound = max(rate_hard_bound, max |r0|): every later state is a convex
    // combination of values inside that bound
    const float bound = fmaxf(a.io.hard, __builtin_bit_cast(float, wmax[1]));
    int rshift = 13 - ((int)((__builtin_bit_cast(unsigned, bound) >> 23) & 0xffu) - 127);
    rshift = rshift > 100 ? 100 : (rshift < -100 ? -100 : rshift);
    const int wexp = duo_w_exp(wmax[0]);
    const float sa = duo_pow2(wexp), usc = duo_pow2(-wexp - rshift), rs = duo_pow2(rshift);
    Ops ops;
    ops.load(rsrc, M, li, lg, sa, wwlds, lane);
    using LdsH8 = const __attribute__((address_space(3))) hv8*;
    using LdsF4 = __attribute__((address_space(3))) mf4*;
    using LdsU = __attribute__((address_space(3))) unsigned*;
    const unsigned bimg = (unsigned)(size_t)(LdsH8)dlds;
    const unsigned xs = bimg + (unsigned)(2 * S::BB) + (unsigned)(lane * 16);
    const unsigned b_rd = bimg + (unsigned)(lg * S::BROW + li * 16);
    const unsigned b_wr = bimg + (unsigned)((lg >> 1) * S::BROW + st * 16 + (lg & 1) * 8 + hi * 4);
    auto store_state = [&]() {
#pragma unroll
        for (int tf = 0; tf < NTF; ++tf) {
            const int rt = RT0 + tf;
            unsigned h, m;
            duo_split2(rc[2 * tf], rc[2 * tf + 1], rs, h, m);
            const unsigned wr = b_wr + (unsigned)(((rt >> 1) * 4 + 2 * (rt & 1)) * S::BROW);
            *(LdsU)(size_t)wr = h;
            *(LdsU)(size_t)(wr + 128u) = m;
        }
    };
    store_state();                                       // the initial state as the first B operand

    int slot = 0;                                        // step % 3: the flag word of the step being finished
    mf4 acc[NT];
    auto chain = [&]() {
        ops.chain(b_rd, acc);
        if constexpr (WS::TAIL_SHARED) *(LdsF4)(size_t)(xs + (unsigned)(WV * S::XS)) = acc[NT - 1];
    };
    // bookkeeping identical in the four waves of the draw: lane s < 8 holds the verdict of stimulus s0 + s
    // (a form with the stopped set as one scalar and the per-stimulus code / step count touched only when a stimulus stops
    // was built and measured: the register allocation of the 2N = 208 kernel tipped into 87 spills, 4 of them inside the
    // serial part -- 31.9 ms against 27.4; the segment it would shorten is short anyway, see the stamps in DESIGN 3.13c)
    int my_code = 1, my_steps = max_iter;
    bool my_frozen = lane >= 8 || !valid || s0 + lane >= a.NB;
    unsigned frozen = (unsigned)__builtin_amdgcn_ballot_w64(my_frozen) & 0xffu;
    auto verdict = [&](int it, int f) {            // f: flag word of step it (lanes 0-7 judge stimulus `lane`)
        const bool fnc = ((f >> (lane & 7)) & 1) != 0, fhb = ((f >> (8 + (lane & 7))) & 1) != 0;
        const bool stop = lane < 8 && !my_frozen && (!fnc || fhb);
        my_code = stop ? (fnc ? 2 : 0) : my_code;
        my_steps = stop ? it + 1 : my_steps;
        my_frozen = my_frozen || stop;
        frozen = (unsigned)__builtin_amdgcn_ballot_w64(my_frozen) & 0xffu;
    };
    // u of the two values of row tile tf from the chain's sums (join of the two parts, scale, external input)
    auto tile_u = [&](int tf, bool first, float& u0, float& u1) {
        mf4 sm = acc[tf];
        if constexpr (WS::HEAD_SHARED) {
            if (tf == 0) {
                const mf4 xp = *(LdsF4)(size_t)(xs + (unsigned)((WV - 1) * S::XS));
                sm.x += xp.x; sm.y += xp.y; sm.z += xp.z; sm.w += xp.w;
            }
        }
        const float j0 = first ? duo_join<true>(sm.x, sm.z, hi) : duo_join<false>(sm.x, sm.z, hi);
        u0 = fmaf(j0, usc, ex[2 * tf]);
        u1 = fmaf(duo_join(sm.y, sm.w, hi), usc, ex[2 * tf + 1]);
    };
    // One row tile early (as the forward, 3.13c): the wave that has ended its chain computes the candidate state of its LAST
    // row tile right behind the chain, in the chain's phase -- join, f(u), Euler step: registers only; whether the step is
    // applied, the stop flags, the previous state and the publication stay in the serial phase.  Same values bit for bit.
    constexpr int TE = NTF - 1;
    constexpr bool EARLY = S::early_solve(NTF);             // (the four-tile wave only)
    constexpr int NS = EARLY ? NE - 2 : NE;                 // values the serial phase still finishes (row tiles 0 .. TE - 1)
    float r1e[2] = {0.f, 0.f};
    auto early = [&]() {
        if constexpr (EARLY) {
            float uu[2], ff[2], dfn[2] = {0.f, 0.f};
            tile_u(TE, true, uu[0], uu[1]);
            duo_eval<false, 2>(io, uu, ff, dfn);
#pragma unroll
            for (int e = 0; e < 2; ++e) r1e[e] = rc[2 * TE + e] + (-rc[2 * TE + e] + ff[e]) * eps[2 * TE + e];
        }
    };
    auto serial = [&](int it) {
        float uu[NS], ff[NS], dfn[NS];
#pragma unroll
        for (int tf = 0; tf < NS / 2; ++tf) tile_u(tf, tf == 0, uu[2 * tf], uu[2 * tf + 1]);
        duo_eval<false, NS>(io, uu, ff, dfn);
        // Rows that do not exist (the padding of the last row tile) stay at their zero state: rows of zeros in W and no input
        // give u = 0, f(0) = 0 and a step of exactly 0 (or NaN beside a NaN in the state, which fmaxf ignores), so their
        // |r1 - r0| never exceeds that of a real row and needs no select; the state itself keeps its select below.
        float r1[NE], dmax = 0.f;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            r1[i] = i < NS ? rc[i] + (-rc[i] + ff[i % NS]) * eps[i] : r1e[(i - NS) & 1];          // ssnode.c:64-67
            dmax = fmaxf(dmax, fabsf(r1[i] - rc[i]));
        }
        const bool take = live && !((frozen >> st) & 1u);
        const bool ncv = dmax >= a.st.atol;                                      // ssnode.c:84-90 (a NaN difference does not count)
        // (timing builds with the cross-lane part of the stop test only every 4th step, and with the previous state written in
        // every step as a state ring would need, priced what a k-step test with exact replay could save: DESIGN 3.13c, round 5)
        unsigned long long votes = __builtin_amdgcn_ballot_w64(take && ncv);
        unsigned bits;
        if (a.st.check_hard) {                                                   // (uniform; never with the saturating I/O function)
            float rmax = -__builtin_inff();
#pragma unroll
            for (int i = 0; i < NE; ++i) rmax = fmaxf(rmax, r1[i]);          // (rows that do not exist are at 0 <= any bound)
            unsigned long long hb = __builtin_amdgcn_ballot_w64(take && rmax >= a.st.hard_stop);     // ssnode.c:98-102
            hb |= hb >> 32; hb |= hb >> 16; hb |= hb >> 8;
            bits = ((unsigned)hb & 0xffu) << 8;
        } else {
            bits = 0u;
        }
        votes |= votes >> 32; votes |= votes >> 16; votes |= votes >> 8;         // lane = 16 lg + 8 hi + st: bit st of the low byte
        bits |= (unsigned)votes & 0xffu;
        // (slot = it % 3 kept incrementally: three integer divisions by 3 per step are 20 scalar instructions of an in-order
        // wave; the OR as a bare ds_or_b32 of one lane -- the builtin brings the atomic optimiser's lane census with it)
        const unsigned fbase = (unsigned)(size_t)flags;
        if (WV == 0 && lane == 0) *(LdsW)(size_t)(fbase + 4u * (unsigned)(slot == 2 ? 0 : slot + 1)) = 0u;
        if (lane == 0 && bits) asm volatile("ds_or_b32 %0, %1" : : "v"(fbase + 4u * (unsigned)slot), "v"(bits) : "memory");
        if (take) {
            // r_prev = the state before the LAST applied step.  The last applied step of a stimulus is the one at which all of
            // its rows pass the convergence test (or step max_iter - 1), so a lane whose own rows do not pass it knows that this
            // step is not the last and need not save -- unless a rate-bound test (any row of any lane) can end the solve too.
            if (!ncv || it >= max_iter - 1 || a.st.check_hard) store_prev();
#pragma unroll
            for (int i = 0; i < NE; ++i) rc[i] = r1[i];         // (a row that does not exist steps from 0 to 0: see above)
            store_state();
        }
    };
    __syncthreads();                                                          // (B)
    bool finished = !valid;
    int it = 0;
    Stamp ts;
    for (int p = 0;; ++p) {
        // flag word of my draw's last finished step (lanes 0-7) and both `done` words of the previous phase (lanes 8, 9): the
        // read is issued here and first used BEHIND the chain -- nothing in front of the chain waits for LDS
        const bool chain_phase = ((p + d) & 1) == 0;
        int word = 0;
        {
            const LdsI src = lane < 8 ? flags + (slot == 0 ? 2 : slot - 1) : (LdsI)(done + ((p + 1) & 1) * 2 + (lane & 1));
            if (lane < 10) word = *src;
        }
        ts.start();
        if (chain_phase && p >= d) {
            // The chain of step `it` runs before the verdict on step it - 1 is known: it reads the state that step published
            // whatever the verdict says, and if the verdict ends the solve its sums are simply not used.
            const bool run = !finished && it < max_iter;
            if (run) {
                chain();
                early();
            } else {
                // (the sums are not used when the chain did not run: say so, or the compiler carries the old ones around the
                // chain with a dozen register moves in front of every chain that does run)
#pragma unroll
                for (int t = 0; t < NT; ++t) asm volatile("" : "=v"(acc[t]));
                asm volatile("" : "=v"(r1e[0]), "=v"(r1e[1]));
            }
            ts.lap(0, !finished);
            if (!finished && it >= 1) verdict(it - 1, word);
            if (frozen == 0xffu || it >= max_iter) finished = true;
        } else if (p >= d) {
            if (!finished) serial(it);
            ++it;
            slot = slot == 2 ? 0 : slot + 1;
        }
        if (WV == 0 && lane == 0) done[(p & 1) * 2 + d] = finished ? 1u : 0u;
        const bool both = p >= 1 && __builtin_amdgcn_readlane(word, 8) != 0 && __builtin_amdgcn_readlane(word, 9) != 0;
        const bool timed = p >= d && !finished;         // (segments 0 .. 2: a chain phase, 3 and 4: a serial phase)
        ts.lap(chain_phase ? 1 : 3, timed);
        duo_phase_barrier();
        ts.lap(chain_phase ? 2 : 4, timed);
        ts.tick(chain_phase && timed);
        if (both) break;
    }
    ts.flush(duo_stamp_row(4 * d + WV));
    if (valid && s < a.NB) {
        const size_t unit = (size_t)b * a.NB + s;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const int row = 16 * (RT0 + i / 2) + 4 * lg + 2 * hi + (i & 1);
            if (row >= M) continue;
            a.r[unit * M + row] = rc[i];
            if (a.r_prev) a.r_prev[unit * M + row] = ((const __attribute__((address_space(3))) float*)rp_slot)[(i / 4) * 256 + (i % 4)];
        }
    }
    if (WV == 0 && valid && lane < 8 && s0 + lane < a.NB) {
        const size_t unit = (size_t)b * a.NB + s0 + lane;
        a.codes[unit] = my_code;
        if (a.steps) a.steps[unit] = my_steps;
    }
}

template <int MK>
__global__ void __launch_bounds__(512, 2) solve_duo_kernel(SolveArgs<float> a) {
    using S = Duo16<MK>;
    // per draw: images, slots, [3][8] flags, previous states of its 4 waves (32 B per lane); then max words, done words
    constexpr int PER_DRAW = S::DRAW + 128 + 4 * 64 * 32;
    constexpr int WL = S::nl_solve() * 1024;
    __shared__ __align__(16) char lds[2 * PER_DRAW + 64 + 8 * WL];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int d = wave >> 2;
    const int ngroups = (a.NB + 7) / 8;
    const long nunits = (long)a.B * ngroups;
    long unit = 2L * blockIdx.x + d;
    const bool valid = unit < nunits;
    if (!valid) unit = nunits - 1;
    const int b = (int)(unit / ngroups), s0 = (int)(unit % ngroups) * 8;
    for (int c = threadIdx.x; c < (int)sizeof(lds) / 4; c += blockDim.x) reinterpret_cast<unsigned*>(lds)[c] = 0u;
    __syncthreads();
    char* const dlds = lds + d * PER_DRAW;
    char* const plds = dlds + S::DRAW + 128;
    char* const wlds = lds + 2 * PER_DRAW;
    char* const wwlds = lds + 2 * PER_DRAW + 64 + wave * WL;
    switch (wave & 3) {
        case 0: duo_solve_wave<MK, 0>(a, d, b, s0, valid, lane, dlds, wlds, plds, wwlds); break;
        case 1: duo_solve_wave<MK, 1>(a, d, b, s0, valid, lane, dlds, wlds, plds, wwlds); break;
        case 2: duo_solve_wave<MK, 2>(a, d, b, s0, valid, lane, dlds, wlds, plds, wwlds); break;
        default: duo_solve_wave<MK, 3>(a, d, b, s0, valid, lane, dlds, wlds, plds, wwlds); break;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The BPTT adjoint sweep in the two-draw form (lock-step phases; semantics of gen_backward_split_kernel, ssn_mfma16.hip,
// and of gen_backward_kernel, ssn_gen.hip: time runs backwards, the wave that finishes row j keeps a_t[j], forms
// delta_t = eps f'(u_t) a_t, hands it to the chain W^T delta_t and writes it -- shifted by one step, in place over f' --
// to HBM).  Per draw: phase A = serial part of step tau (needs W^T delta_{tau+1} from the accumulators of the previous
// chain), phase B = chain of step tau; the two draws of a workgroup run the two phases in opposition.
// delta goes to the chain as TWO fp16 parts by round to nearest (|d - h - m| <= 2^-23 |d|) under a power-of-two scale that
// follows the data with one step of lag: the scale of step tau puts max |delta_{tau+1}| of the draw at 2^7 (the four
// waves' maxima meet in one of three rotating LDS words per draw); a step whose delta outgrows the fp16 range under that
// scale is poisoned with NaN (see gen_backward_split_kernel).  All 8 stimuli of a draw share the scale.
// The sweep's state (carry, f' with one prefetch, three trajectory rows with one prefetch inside the penalty window,
// the sum of delta for dL/d ext: 9 values per row and stimulus) lives in registers next to W^T, which is why the low parts
// of the last 16 / 20 units of a wave (three / four row tiles finished) stay in LDS through the penalty window and 8 / 12
// after it, when the trajectory rows are gone and the difference is pulled into registers (Duo16::nl_bwd_win, nl_bwd;
// an operand spilled to scratch instead costs its chain 4000 cycles instead of 1400).
// ---------------------------------------------------------------------------------------------------------------
template <int MK, int WV, bool GEXT>
__device__ __forceinline__ void duo_backward_wave(const GenBwdArgs<float>& a, int d, int b, int s0, bool valid, int lane,
                                                  char* dlds, char* wwlds, unsigned* wmax) {
    using S = Duo16<MK>;
    using WS = DuoWave<MK, WV>;
    constexpr int NT = WS::NT, NTF = WS::NTF, RT0 = WS::RT0;
    constexpr int NE = 2 * NTF;
    const int M = a.M, N = a.M / 2, T_ = a.seqlen;
    const int li = lane & 15, lg = lane >> 4, hi = li >> 3, st = li & 7;
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.W + (size_t)b * M * M), 0, M * M * 4, 0x00020000);
    using Ops = DuoOperands<MK, WV, S::nl_bwd_win(WV, WS::NTF), true>;             // window steps
    using OpsN = DuoOperands<MK, WV, S::nl_bwd(WS::NTF, GEXT), true>;            // the steps after the window
    typename Ops::Raw raw;
    atomicMax(wmax, __builtin_bit_cast(unsigned, Ops::fetch(rsrc, M, li, lg, raw)));
    using LdsH8 = const __attribute__((address_space(3))) hv8*;
    using LdsF4 = __attribute__((address_space(3))) mf4*;
    using LdsU = __attribute__((address_space(3))) unsigned*;
    using LdsUC = volatile const __attribute__((address_space(3))) unsigned*;
    const unsigned bimg = (unsigned)(size_t)(LdsH8)dlds;
    // (lock-step only: ONE B image per draw -- the second one of the common layout is LDS this kernel needs for W^T)
    constexpr int SYNCB = S::BB + (S::WM - 1) * S::XS;
    const unsigned xs = bimg + (unsigned)S::BB + (unsigned)(lane * 16);
    const unsigned b_rd = bimg + (unsigned)(lg * S::BROW + li * 16);
    const unsigned b_wr = bimg + (unsigned)((lg >> 1) * S::BROW + st * 16 + (lg & 1) * 8 + hi * 4);
    const unsigned slots = bimg + (unsigned)SYNCB;                              // three rotating words: max |delta| bit patterns
    auto slot = [&](int tau) { return slots + 4u * (unsigned)((tau + 3) % 3); };
    // ---- the values this lane finishes
    const int s = s0 + st;
    const bool live = valid && s < a.NB;
    const float inv = 1.f / (float)(T_ - a.skip);
    const size_t blk_elems = (size_t)a.NB * T_ * M;
    const __amdgpu_buffer_rsrc_t rs_traj =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.traj) + (size_t)b * blk_elems, 0, (int)(blk_elems * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_dlt =
        __builtin_amdgcn_make_buffer_rsrc(a.delta + (size_t)b * blk_elems, 0, (int)(blk_elems * 4), 0x00020000);
    // Addresses of the two streams: byte offset = lane part (stimulus, row 4 lg + 2 hi within a tile: ONE register per
    // finished tile, -1 = this lane has nothing there: out of range for the buffer, loads return zeros and stores are
    // dropped) + uniform part (stream index, row tile) in the instruction's scalar offset.  The hardware's range check sees
    // the lane part only, so a step that has no such index (tau - 3 < 0 ...) goes to a descriptor of zero records instead.
    const int toff = live ? (int)(((size_t)s * T_ * M + 4 * lg + 2 * hi) * 4) : -1;
    int voff[NTF];
#pragma unroll
    for (int tf = 0; tf < NTF; ++tf) voff[tf] = (toff < 0 || 16 * (RT0 + tf) + 4 * lg + 2 * hi >= M) ? -1 : toff;
    const __amdgpu_buffer_rsrc_t rs_none = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.traj), 0, 0, 0x00020000);
    struct At { int tf, t; };
    auto at = [&](int tf, int t) { return At{tf, t}; };
    auto soff = [&](const At& p) { return (p.t * M + 16 * (RT0 + p.tf)) * 4; };
    auto load2 = [&](const __amdgpu_buffer_rsrc_t& rs, bool on, const At& p, float& x0, float& x1) {
        const fv2 q = __builtin_bit_cast(fv2, __builtin_amdgcn_raw_buffer_load_b64(on ? rs : rs_none, voff[p.tf], on ? soff(p) : 0, 0));
        x0 = q.x; x1 = q.y;
    };
    auto store2 = [&](const __amdgpu_buffer_rsrc_t& rs, bool on, const At& p, float x0, float x1) {
        const fv2 q = {x0, x1};
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(unsigned __attribute__((ext_vector_type(2))), q), on ? rs : rs_none,
                                              voff[p.tf], on ? soff(p) : 0, 0);
    };
    // f'(u) of three consecutive steps in a rotating set of registers: the step with phase PH = (T - tau) % 3 uses
    // df3[(PH + 1) % 3] and loads, two steps ahead, into df3[PH] -- no register copies between steps, so the wait for a
    // load sits two steps (four phases) behind its issue instead of at the end of the serial part that issued it
    float eps[NE], gta[NE], carry[NE], dsum[NE], xn[NE], xc[NE], xm[NE], pxm[NE], df3[3][NE];
    bool rowok[NE];
    auto direct = [&](int i, int tau) {            // dL/dx_tau inside the penalty window (time average, rate and dynamics terms)
        float gg = gta[i] + ((xc[i] > a.theta) ? a.c_rate : 0.f);
        if (tau <= T_ - 1) gg -= 2.f * a.c_dyn * (xn[i] - xc[i]);
        if (tau >= a.skip + 2) gg += 2.f * a.c_dyn * (xc[i] - xm[i]);
        return gg;
    };
    __syncthreads();                                                          // (A) max |W|
    const int wexp = duo_w_exp(*wmax);
    Ops ops;
    ops.split(raw, duo_pow2(wexp), wwlds, lane);
    // (the per-value state is set up AFTER the W prologue, the one place where every register is taken: set up before it,
    // two of the window's constants were spilled there and reloaded from scratch -- with s_waitcnt vmcnt(0) -- in every step)
    float m0 = 0.f;
#pragma unroll
    for (int tf = 0; tf < NTF; ++tf) {
        const int row = 16 * (RT0 + tf) + 4 * lg + 2 * hi;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int i = 2 * tf + e;
            rowok[i] = row + e < M;
            // (0 for a row or stimulus that does not exist: its delta = eps f' a is then 0 without a select in the loop;
            // its f', carry and sums are zeros already -- out-of-range loads, zero rows of W^T, zero columns of the B image)
            eps[i] = (row + e < M && live) ? (row + e < N ? a.eps_E : a.eps_I) : 0.f;
            gta[i] = (live && row + e < M) ? a.g_time_avg[((size_t)b * a.NB + s) * M + row + e] * inv : 0.f;
            carry[i] = dsum[i] = xn[i] = 0.f;
        }
        load2(rs_traj, true, at(tf, T_ - 1), xc[2 * tf], xc[2 * tf + 1]);                   // x_T
        load2(rs_traj, T_ >= 2, at(tf, T_ - 2), xm[2 * tf], xm[2 * tf + 1]);
        load2(rs_dlt, true, at(tf, T_ - 1), df3[1][2 * tf], df3[1][2 * tf + 1]);             // f'(u_T): phase 0 uses df3[1]
        store2(rs_dlt, true, at(tf, T_ - 1), 0.f, 0.f);                                      // slot T - 1 of the shifted delta stays zero
        load2(rs_traj, T_ >= 3, at(tf, T_ - 3), pxm[2 * tf], pxm[2 * tf + 1]);
        load2(rs_dlt, T_ >= 2, at(tf, T_ - 2), df3[2][2 * tf], df3[2][2 * tf + 1]);          // f'(u_{T-1}): phase 1 uses df3[2]
        df3[0][2 * tf] = df3[0][2 * tf + 1] = 0.f;
        // the first step's scale: max |delta_T| (carry = 0), or of eps |a_T| 2^-20 if f' vanishes everywhere
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int i = 2 * tf + e;
            if (!rowok[i] || !live) continue;
            const float a_T = (T_ >= a.skip + 1) ? direct(i, T_) : 0.f;
            m0 = fmaxf(m0, fmaxf(__builtin_fabsf(eps[i] * df3[1][i] * a_T), __builtin_fabsf(eps[i] * a_T) * 9.5367431640625e-07f));
        }
    }
    {
        const unsigned wm0 = wave_max_bits(m0);
        if (lane == 0) __hip_atomic_fetch_max((__attribute__((address_space(3))) unsigned*)(dlds + SYNCB) + (T_ + 1 + 3) % 3, wm0,
                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }

    mf4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (mf4){0.f, 0.f, 0.f, 0.f};
    int bused = 0;                                  // the scale exponent the draw's delta in LDS was written with
    unsigned lastref = 0u;
    unsigned runmax = 0u;                           // max over the steps so far of max |delta_tau| (scalar): GenBwdArgs::dmax
    auto chain = [&](const auto& o) {
        o.chain(b_rd, acc);
        if constexpr (WS::TAIL_SHARED) *(LdsF4)(size_t)(xs + (unsigned)(WV * S::XS)) = acc[NT - 1];
    };
    // The last row tile of a step AFTER the window can be finished early: right behind the chain of the step before, in
    // that chain's phase (the wave would idle there while the partner wave of its SIMD is in a serial part 300-500 cycles
    // longer than a chain): join, delta, carry, the f' load two steps ahead and the store of delta need registers and global
    // memory only.  What it leaves for the serial phase: delta of that tile (2 values) and their maximum, for the scale test
    // and the publication to the B image.
    constexpr int TE = NTF - 1;
    float de0 = 0.f, de1 = 0.f, dme = 0.f;
    auto join_tile = [&](int tf, float usc) {
        mf4 sm = acc[tf];
        if constexpr (WS::HEAD_SHARED) {
            if (tf == 0) {
                const mf4 xp = *(LdsF4)(size_t)(xs + (unsigned)((WV - 1) * S::XS));
                sm.x += xp.x; sm.y += xp.y; sm.z += xp.z; sm.w += xp.w;
            }
        }
        carry[2 * tf] = fmaf(duo_join(sm.x, sm.z, hi), usc, carry[2 * tf]);
        carry[2 * tf + 1] = fmaf(duo_join(sm.y, sm.w, hi), usc, carry[2 * tf + 1]);
    };
    auto early = [&](auto PH, int tau) {             // step tau (no window terms), tile TE; runs behind the chain of step tau + 1
        constexpr int ph = decltype(PH)::value;
        float (&dfc)[NE] = df3[(ph + 1) % 3];
        float (&ndf)[NE] = df3[ph];
        if (tau < T_) join_tile(TE, duo_pow2(-wexp - bused));
        float dl[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int i = 2 * TE + e;
            const float a_t = carry[i];
            dl[e] = eps[i] * dfc[i] * a_t;
            carry[i] = fmaf(-eps[i], a_t, a_t);
            if (GEXT) dsum[i] += dl[e];
        }
        de0 = dl[0]; de1 = dl[1];
        dme = fmaxf(__builtin_fabsf(dl[0]), __builtin_fabsf(dl[1]));
        load2(rs_dlt, tau >= 3, at(TE, tau - 3), ndf[2 * TE], ndf[2 * TE + 1]);
        store2(rs_dlt, tau >= 2, at(TE, tau - 2), dl[0], dl[1]);
    };
    auto serial = [&](auto WIN, auto PH, int tau, auto ED_) {
        constexpr bool win_on = decltype(WIN)::value;
        constexpr int ph = decltype(PH)::value;
        constexpr bool ED = decltype(ED_)::value && !win_on && NTF > 1;      // tile TE of this step was finished early
        float (&dfc)[NE] = df3[(ph + 1) % 3];
        float (&ndf)[NE] = df3[ph];
        // loads for two steps ahead (f' into the rotating set; the trajectory row of the window is copied into place at the end)
        float nxm[NE];
#pragma unroll
        for (int tf = 0; tf < NTF; ++tf) {
            nxm[2 * tf] = nxm[2 * tf + 1] = 0.f;
            if constexpr (win_on)         // (no such index: zero-record descriptor, the load returns zeros, no branch)
                load2(rs_traj, tau >= 4 && tau >= a.skip + 3, at(tf, tau - 4), nxm[2 * tf], nxm[2 * tf + 1]);
        }
        // scale of this step's delta from the previous step's maximum (kept when that was exactly zero)
        const unsigned mprev = (unsigned)__builtin_amdgcn_readfirstlane((int)*(LdsUC)(size_t)slot(tau + 1));
        if (WV == 0 && lane == 0) *(LdsU)(size_t)slot(tau + 2) = 0u;             // next step's word (last read two phases ago)
        const unsigned ref = mprev ? mprev : lastref;
        lastref = ref;
        runmax = runmax > mprev ? runmax : mprev;       // (delta_T .. delta_2 are stored; their maxima are read at tau = T - 1 .. 1)
        int bexp = 7 - ((int)((ref >> 23) & 0xffu) - 127);
        bexp = ref == 0u ? 0 : (bexp > 100 ? 100 : (bexp < -100 ? -100 : bexp));
        if (tau < T_) {                             // W^T delta_{tau+1} 2^(a + bused) from the accumulators of the last chain
            const float usc = duo_pow2(-wexp - bused);
#pragma unroll
            for (int tf = 0; tf < NTF; ++tf)
                if (!(ED && tf == TE)) join_tile(tf, usc);
        }
        float delta[NE], dm = 0.f;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            if (ED && i / 2 == TE) { delta[i] = (i & 1) ? de1 : de0; continue; }
            float a_t = carry[i];
            if constexpr (win_on) a_t += direct(i, tau);
            delta[i] = eps[i] * dfc[i] * a_t;
            dm = fmaxf(dm, __builtin_fabsf(delta[i]));
            carry[i] = fmaf(-eps[i], a_t, a_t);                                   // (1 - eps) a_t
            if (GEXT) dsum[i] += delta[i];
            if constexpr (win_on) { xn[i] = xc[i]; xc[i] = xm[i]; xm[i] = pxm[i]; pxm[i] = nxm[i]; }
        }
        // (after the last use of this phase's f': its registers are free for nothing else; the load two steps ahead goes
        // into the set the step before last used)
#pragma unroll
        for (int tf = 0; tf < NTF; ++tf) {
            if (!(ED && tf == TE)) load2(rs_dlt, tau >= 3, at(tf, tau - 3), ndf[2 * tf], ndf[2 * tf + 1]);
        }
        if constexpr (ED) dm = fmaxf(dm, dme);
        const float rs = live ? duo_pow2(bexp) : 0.f;
        if (!(dm * rs < 65504.f)) {                                                // outgrew the lagged scale: poison, do not clamp
            delta[0] = __builtin_nanf("");
            // ... and say so where the host can count it: the draw's hand-over word becomes NaN (as a bit pattern it is above
            // every |delta|, so the atomic maximum keeps it)
            if (a.dmax) atomicMax(a.dmax + b, 0x7fc00000u);
        }
#pragma unroll
        for (int tf = 0; tf < NTF; ++tf) {
            const int rt = RT0 + tf;
            unsigned h, m;
            duo_split2(delta[2 * tf], delta[2 * tf + 1], rs, h, m);
            const unsigned wr = b_wr + (unsigned)(((rt >> 1) * 4 + 2 * (rt & 1)) * S::BROW);
            *(LdsU)(size_t)wr = h;
            *(LdsU)(size_t)(wr + 128u) = m;
            if (!(ED && tf == TE)) store2(rs_dlt, tau >= 2, at(tf, tau - 2), delta[2 * tf], delta[2 * tf + 1]);   // shifted: pairs with x_{tau-1}
        }
        bused = bexp;
        // one LDS atomic per wave (64 lanes on one address serialise: 16.6 -> 9.x ms): wave maximum first, six DPP steps
        const unsigned wm = wave_max_bits(live ? dm : 0.f);
        if (lane == 0) __hip_atomic_fetch_max((__attribute__((address_space(3))) unsigned*)(dlds + SYNCB) + (tau + 3) % 3, wm,
                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    constexpr std::integral_constant<bool, false> W0{};
    constexpr std::integral_constant<bool, true> W1{};
    __syncthreads();                                                          // (B)
    if (d) __syncthreads();                            // draw 1 runs one phase behind draw 0
    Stamp ts;                                          // (the steps after the window)
    constexpr std::integral_constant<bool, false> E0{};
    constexpr std::integral_constant<bool, true> E1{};
    auto step = [&](auto WIN, auto PH, int tau, const auto& o) {
        constexpr bool timed = !decltype(WIN)::value;
        ts.start();
        serial(WIN, PH, tau, E0);
        ts.lap(0, timed);
        duo_phase_barrier();
        ts.lap(1, timed);
        chain(o);
        ts.lap(2, timed);
        duo_phase_barrier();
        ts.lap(3, timed);
        ts.tick(timed);
    };
    // a step after the window whose last tile was finished early, finishing the next step's last tile behind its own chain
    auto step_e = [&](auto PH, auto PHN, int tau, bool more, const auto& o) {
        ts.start();
        serial(W0, PH, tau, E1);
        ts.lap(0);
        duo_phase_barrier();
        ts.lap(1);
        chain(o);
        if (more) early(PHN, tau - 1);
        ts.lap(2);
        duo_phase_barrier();
        ts.lap(3);
        ts.tick();
    };
    constexpr std::integral_constant<int, 0> P0{};
    constexpr std::integral_constant<int, 1> P1{};
    constexpr std::integral_constant<int, 2> P2{};
    // The f' registers rotate through three sets, one per step (the load of step tau - 3 goes into the set step tau - 1
    // used).  The rotation must be STATIC in the code that runs 1200 times: written as one loop over a phase variable the
    // compiler folds the three variants back into one body that rotates the sets with v_mov -- and a copy of a register
    // with a load in flight needs s_waitcnt vmcnt(0), i.e. every step waited for its own stores to be acknowledged
    // (seen in the assembly; 2100 cycles per serial part instead of 1300).  So: three steps per iteration, spelled
    // out; the generic form only for the at most two steps that bring the phase back to 0 at each end.
    int tau = T_, ph = 0;
    auto step_any = [&](auto WIN, const auto& o) {
        if (ph == 0) step(WIN, P0, tau, o); else if (ph == 1) step(WIN, P1, tau, o); else step(WIN, P2, tau, o);
        ph = ph == 2 ? 0 : ph + 1;
        --tau;
    };
    const int tw = a.skip + 1 > 1 ? a.skip + 1 : 1;     // window steps first (time runs backwards): tau = T ... tw
    for (; tau - 2 >= tw; tau -= 3) {
        step(W1, P0, tau, ops);
        step(W1, P1, tau - 1, ops);
        step(W1, P2, tau - 2, ops);
    }
    while (tau >= tw) step_any(W1, ops);
    OpsN opsn;                                         // the window is over: its registers go to W^T (fewer LDS reads per chain)
    opsn.promote_from(ops);
    while (tau >= 1 && ph != 0) step_any(W0, opsn);
    if constexpr (S::EARLY_BWD && NTF > 3) {       // (the four-tile wave only: for the others chain + tile outlasts the serial part it shortens)
        if (tau >= 3) early(P0, tau);                  // (primes the pipeline: once, outside a chain phase)
        for (; tau >= 3; tau -= 3) {
            step_e(P0, P1, tau, true, opsn);
            step_e(P1, P2, tau - 1, true, opsn);
            step_e(P2, P0, tau - 2, tau - 3 >= 3, opsn);
        }
    } else {
        for (; tau >= 3; tau -= 3) {
            step(W0, P0, tau, opsn);
            step(W0, P1, tau - 1, opsn);
            step(W0, P2, tau - 2, opsn);
        }
    }
    while (tau >= 1) step_any(W0, opsn);
    ts.flush(duo_stamp_row(4 * d + WV));
    if (!d) __syncthreads();
    // the bound ssn_gw.hip scales the draw's delta with (the prologue's estimate of max |delta_T| in the first word read
    // only makes it larger; a poisoned step stores NaN and the products are NaN whatever the scale)
    if (a.dmax && valid && WV == 0 && lane == 0) atomicMax(a.dmax + b, runmax);
    if (GEXT && live) {
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const int row = 16 * (RT0 + i / 2) + 4 * lg + 2 * hi + (i & 1);
            if (row < M) a.g_ext[((size_t)b * a.NB + s) * M + row] = dsum[i];
        }
    }
}

template <int MK, bool GEXT>
__global__ void __launch_bounds__(512, 2) gen_backward_duo_kernel(GenBwdArgs<float> a) {
    using S = Duo16<MK>;
    // LDS-resident part of W^T per wave of a draw (by the row tiles the wave finishes), and its prefix sums
    constexpr int WL0 = S::nl_bwd_win(0, DuoWave<MK, 0>::NTF) * 1024, WL1 = S::nl_bwd_win(1, DuoWave<MK, 1>::NTF) * 1024,
                  WL2 = S::nl_bwd_win(2, DuoWave<MK, 2>::NTF) * 1024, WL3 = S::nl_bwd_win(3, DuoWave<MK, 3>::NTF) * 1024;
    constexpr int WLD = WL0 + WL1 + WL2 + WL3;                        // per draw
    constexpr int DRAWB = S::BB + (S::WM - 1) * S::XS + 32;          // per draw: one B image, partial-sum slots, scale words
    constexpr int LDSB = 2 * DRAWB + 16;
    __shared__ __align__(16) char lds[LDSB + 2 * WLD + 16];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int d = wave >> 2;
    const int ngroups = (a.NB + 7) / 8;
    const long nunits = (long)a.B * ngroups;
    long unit = 2L * blockIdx.x + d;
    const bool valid = unit < nunits;
    if (!valid) unit = nunits - 1;
    const int b = (int)(unit / ngroups), s0 = (int)(unit % ngroups) * 8;
    for (int c = threadIdx.x; c < LDSB / 4; c += blockDim.x) reinterpret_cast<unsigned*>(lds)[c] = 0u;
    __syncthreads();
    char* const dlds = lds + d * DRAWB;
    const int wq = wave & 3;
    char* const wwlds = lds + LDSB + d * WLD + (wq > 0 ? WL0 : 0) + (wq > 1 ? WL1 : 0) + (wq > 2 ? WL2 : 0);
    unsigned* const wmax = reinterpret_cast<unsigned*>(lds + 2 * DRAWB) + d;
    switch (wave & 3) {
        case 0: duo_backward_wave<MK, 0, GEXT>(a, d, b, s0, valid, lane, dlds, wwlds, wmax); break;
        case 1: duo_backward_wave<MK, 1, GEXT>(a, d, b, s0, valid, lane, dlds, wwlds, wmax); break;
        case 2: duo_backward_wave<MK, 2, GEXT>(a, d, b, s0, valid, lane, dlds, wwlds, wmax); break;
        default: duo_backward_wave<MK, 3, GEXT>(a, d, b, s0, valid, lane, dlds, wwlds, wmax); break;
    }
}

// SSN_DUO_FREE=1: the free-running form (per-draw LDS counters, no workgroup barrier in the time loop) instead of the
// lock-step one (one workgroup barrier per phase).  Same results bit for bit; measured 3.50 against 3.38 ms at C3, so the
// lock-step form is the default and this one stays for A/B timing.
static bool duo_free_running() {
    static const bool on = [] { const char* e = getenv("SSN_DUO_FREE"); return e && e[0] == '1'; }();
    return on;
}
// SSN_DUO_HT=0: the half-real tail tile as row pairs like every other tile (A/B runs; results are bit-identical)
static bool duo_half_tail_on() {
    static const bool on = [] { const char* e = getenv("SSN_DUO_HT"); return !(e && e[0] == '0'); }();
    return on;
}

template <int MK, bool HT>
static hipError_t launch_duo_fwd_ht(const GenFwdArgs<float>& a, int rshift, hipStream_t st) {
    const long nunits = (long)a.B * ((a.NB + 7) / 8);
    const dim3 grid((unsigned)((nunits + 1) / 2));
    if (duo_free_running()) {
        if (a.traj) hipLaunchKernelGGL((gen_forward_duo_kernel<MK, true, true, HT>), grid, dim3(512), 0, st, a, rshift);
        else hipLaunchKernelGGL((gen_forward_duo_kernel<MK, false, true, HT>), grid, dim3(512), 0, st, a, rshift);
    } else {
        if (a.traj) hipLaunchKernelGGL((gen_forward_duo_kernel<MK, true, false, HT>), grid, dim3(512), 0, st, a, rshift);
        else hipLaunchKernelGGL((gen_forward_duo_kernel<MK, false, false, HT>), grid, dim3(512), 0, st, a, rshift);
    }
    return hipGetLastError();
}
// rshift from gen_split_rshift (ssn_mfma16.hip): the same applicability rules as the other fp16-split forms
hipError_t launch_gen_forward_duo(const GenFwdArgs<float>& a, hipStream_t st) {
    const int rshift = gen_split_rshift(a);
    if (rshift < 0) return hipErrorInvalidValue;
    return Fp16Ladder::with(a.M, [&](auto MKC) {
        constexpr int MK = decltype(MKC)::value;
        if constexpr (MK == 208) {
            if (duo_half_tail(MK, a.M) && duo_half_tail_on()) return launch_duo_fwd_ht<MK, true>(a, rshift, st);
        }
        return launch_duo_fwd_ht<MK, false>(a, rshift, st);
    });
}

// applicability: solve_split_supported (ssn_mfma16.hip)
hipError_t launch_solve_duo(const SolveArgs<float>& a, hipStream_t st) {
    if (!solve_split_supported(a)) return hipErrorInvalidValue;
    return Fp16Ladder::with(a.M, [&](auto MKC) {
        const long nunits = (long)a.B * ((a.NB + 7) / 8);
        hipLaunchKernelGGL((solve_duo_kernel<decltype(MKC)::value>), dim3((unsigned)((nunits + 1) / 2)), dim3(512), 0, st, a);
        return hipGetLastError();
    });
}

// applicability: gen_mfma_supported (any I/O function: the scale follows the data)
hipError_t launch_gen_backward_duo(const GenBwdArgs<float>& a, hipStream_t st) {
    return Fp16Ladder::with(a.M, [&](auto MKC) {
        constexpr int MK = decltype(MKC)::value;
        const long nunits = (long)a.B * ((a.NB + 7) / 8);
        const dim3 grid((unsigned)((nunits + 1) / 2));
        if (a.g_ext) hipLaunchKernelGGL((gen_backward_duo_kernel<MK, true>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((gen_backward_duo_kernel<MK, false>), grid, dim3(512), 0, st, a);
        return hipGetLastError();
    });
}

}  // namespace ssn

#if SSN_DUO_STAMP
extern "C" int ssn_debug_duo_stamps(unsigned long long* out64) {
    return (int)hipMemcpyFromSymbol(out64, HIP_SYMBOL(ssn::duo_stamps), 64 * sizeof(unsigned long long));
}
#endif
