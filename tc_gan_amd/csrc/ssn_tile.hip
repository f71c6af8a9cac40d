// "Tile" register-stationary SSN solver (variant 2) for MI355X (gfx950).
//
// Same contract as solve_regw_kernel (ssn_solver.hip) -- the Euler loop of
// tc_gan/ext/ssnode.c:69-187 over B draws x NB stimuli -- with a different
// mapping of W onto the register file, chosen from measurements on the chip
// (tools/microbench): a v_fmac_f32 whose r operand is DPP-broadcast issues at
// ~2/3 of the rate of a plain VGPR-operand v_fmac_f32, and with one matrix row
// per lane a 200-neuron solve keeps only 200 of 256 lanes busy.
//
// Layout: a wave is an 8 x 8 grid of lanes, lane = 8*rg + cg.
//   * row group rg owns RA consecutive rows:  row = (8*wave + rg)*RA + a
//   * column group cg owns C consecutive columns:  col = cg*C + c
//   * each lane holds the RA x C tile W[rows(rg)][cols(cg)] in VGPRs for the
//     whole solve (W is read from HBM once);
//   * per Euler step the lane reads ITS C values of r from LDS with 16-byte
//     reads (the 8 lanes of a column group read the same address -> broadcast;
//     slabs are padded so the 8 column groups hit disjoint banks) and issues
//     RA*C plain FMAs: every loaded r value feeds RA FMAs;
//   * the 8 partial sums of a row sit in 8 ADJACENT lanes; a transpose-reduce
//     (reduce8_to_lane, ssn_tile_core.h: 7 DPP adds + selects, the first stage as
//     masked v_add_f32_dpp) leaves lane cg with the complete sum of row a = cg;
//   * lane cg < RA then finishes row a = cg: + ext, I/O nonlinearity, Euler
//     update, stop tests, and writes r' back to LDS.  ONE barrier per step.
// For 2N = 200: C = 25, RA = 7, 4 waves (224 row slots, 200 used; all 200
// columns exact).  Default shape: split residency (RL = 2: five rows of every
// lane's tile in VGPRs as packed pairs, two in LDS), 167 VGPRs, three workgroups
// per CU; the all-register shape (175 W registers per lane, two workgroups per
// CU) is variant 4.  fp32 with one stimulus per draw at 2N = 170..200: rows 56/48/48/48, one 7-row and three 6-row
// waves (solve_tile_mixed6_kernel), whose lane grid puts the column-group bits on lane bits 2, 3 and 0 so that two of the three
// exchanges of the transpose-reduce choose with DPP bank masks (reduce_bank_f32, ssn_tile_core.h).  fp64: 7 rows x C <= 13 up
// to 2N = 104, 4 rows x C = 19 / 26 (one workgroup of 5-7 waves per CU) up to 2N = 208.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "ssn_device.h"
#include "ssn_host.h"
#include "ssn_tile_core.h"

// diagnostic switch: 0 = the uniform 7-row kernel also at 2N = 170..200 (A/B builds)
#ifndef SSN_TILE_MIXED
#define SSN_TILE_MIXED 1
#endif
// diagnostic switch: columns of a 6-row wave's third row pair that stay in VGPRs (0 = the whole pair in LDS; A/B builds)
#ifndef SSN_TILE_KV
#define SSN_TILE_KV 12
#endif

namespace ssn {

// LDS words of the stop protocol per stimulus: three rotating slots, or the two verdict words of the fp32 NB = 1 loop
template <typename T, int NB> constexpr int tile_flag_words() { return (NB == 1 && sizeof(T) == 4) ? 2 : 3; }

// The fp32 NB = 1 loop exists twice in its kernels, with and without the test of the rate bound, which is uniform per launch:
// the kernel picks the whole wave body once, so that the loop of a launch without the test holds no compare against hard_stop.
// (Two loops behind one prologue do not fit the mixed kernels' 168 VGPRs.)  The mixed kernels do this.  TIGHT:
// solve_tile_mixed_kernel at C = 25 spills a register with two bodies and keeps the one with the test, as solve_tile_kernel does
// in all its shapes: several of them sit right at a register step (128 VGPRs at C = 13: a fourth wave per SIMD; 168 at C = 19
// and C = 25), which the second body crosses.
template <typename T, int NB, bool TIGHT = false> constexpr bool tile_hard_split() { return NB == 1 && sizeof(T) == 4 && !TIGHT; }

// One wave of a tile kernel: its RA x C tile of W (rows rowbase + a of row group rg), and the forms of its step loop that
// follow from it.  Every wave of a workgroup has the same C, NB and barrier sequence; RA / RL / PK (row pairs packed for
// v_pk_fma_f32) may differ between waves (mixed kernels below).  KV, WSO: see SplitTile.
// BANK (the fp32 NB = 1 waves of solve_tile_mixed6_kernel): the column-group bits on lane bits 2, 3 and 0, so that two of the three
// exchanges of the transpose-reduce choose with DPP bank masks (reduce_bank_f32): the lane owns the columns of group
// bank_col_group(lane) and finishes row bank_row(lane) of its row group; rowbase is that of row group bank_row_group(lane).
template <typename T_, int RA_, int C_, int RL_, int NB_, bool PK, int KV = 0, int WSO = 0, bool BANK_ = false>
struct TileWave {
    using T = T_;
    static constexpr int RA = RA_, C = C_, RL = RL_, NB = NB_;
    static constexpr bool BANK = BANK_;
    static constexpr int CP = SlabPad<C>::value;
    static constexpr bool SPLIT = RL > 0 || PK;        // SplitTile: packed row pairs in VGPRs (+ RL rows in LDS); else all in VGPRs
    // OPAIR: the waves of the fp32 NB = 1 split kernels at C = 25 whose tile is two packed row pairs, an odd row and two
    // LDS-resident rows.  They have one form: the odd row in column pairs inside the one-statement FMA block, and a
    // transpose-reduce of their 7 rows that forms no zero row 7.
    static constexpr bool OPAIR = sizeof(T) == 4 && NB == 1 && !PK && RA == 7 && RL == 2 && C % 4 == 1;
    // SIXROW: the 6-row waves of solve_tile_mixed6_kernel: two packed row pairs and a third pair split between VGPRs and LDS,
    // one-statement forms throughout and a transpose-reduce that forms no zero rows 6 and 7
    static constexpr bool SIXROW = KV > 0;
    // the FMA block of the solver (SplitTile::matvec's MODE): the first product of every chain is a multiply, and the light
    // wave of the mixed kernel (all rows packed, none in LDS) runs the one-statement form as well
    static constexpr int FMA_MODE = 2 | ((OPAIR || SIXROW || (PK && RL == 0)) ? 1 : 0);
    // fp32, NB = 1: the step loop without the NB-generic bookkeeping (tile_loop_fp32_one: rotated by half a step so that one
    // test of the verdict word ends it, one scalar verdict byte per wave, unrolled by the parity of the state buffer) and
    // without an exec-mask region around the state store (FLAT)
    static constexpr bool FAST1 = NB == 1 && sizeof(T) == 4;
    static constexpr bool FLAT = FAST1 && CP > C;      // (C = 4 has no pad float to absorb a dummy store)
    using Tile = SplitTile<T, RA, C, RL, OPAIR, KV, WSO>;
    static_assert(RA <= 8, "a row group has 8 lanes to finish its rows");
    static_assert(!SIXROW || (sizeof(T) == 4 && NB == 1 && !PK && RA == 6 && RL == 2), "the 6-row wave is an fp32 NB = 1 form");
    static_assert(!BANK || OPAIR || SIXROW, "the bank-mask reduce is the 7- and 6-row fp32 NB = 1 waves'");
};

// The step loop of the fp32 NB = 1 waves (W::FAST1): rotated by half a step so that one test of the verdict word ends it, one
// scalar verdict byte per wave, unrolled by the parity of the state buffer; ONE workgroup barrier per step.
// Stop protocol: one verdict WORD per parity of the state buffer, one BYTE of it per wave.  In step t
// every wave ANDs its two compare masks with the mask of its finishing lanes and forms one scalar byte -- bit 0:
// some row of this wave is still moving, bit 1: some row hit the rate bound -- which all its lanes store, same
// address, same value, to byte `wave` of word t % 2.  Only the wave itself ever writes that byte, so it keeps the
// value it stored last per parity in a scalar register (0 behind the prologue's clear) and stores under a scalar
// branch, only when the byte changes: there is no clear, no sink word and no address select, and a step whose
// verdict is that of two steps before costs the vector port and the LDS nothing for it.  The bytes of waves that
// do not exist are zeroed once in the prologue.
// Two words are enough: the word of step t is written before barrier t, read after barrier t (the load issued
// before the FMA block of step t + 1, consumed behind it, before barrier t + 1), and its next write, for step
// t + 2, comes after barrier t + 1.  Step t reads state buffer t % 2 and writes the other, so the word follows the
// parity of the buffer, and the loop below holds one body per parity: buffer, word and read address are immediate
// offsets on VGPRs that are computed here, once.
// HARD: the launch tests the rate bound (without it the body holds no compare against hard_stop, and bit 1 of the byte is
// never set).  sw / w, wlds, wtid: the wave's tile (tile_wave_body); lane, cg, fin, myslot, ex, eps: the row this lane
// finishes.  In: rc = x_0.  Out: rc, rp = x_k, x_{k-1}, read back from the two state buffers; code and nsteps if the solve
// stopped; outrow (BANK).
template <typename W, bool HARD, typename T>
__device__ __forceinline__ void tile_loop_fp32_one(const SolveArgs<T>& a, const typename W::Tile& sw, const T (&w)[W::SPLIT ? 1 : W::RA][W::SPLIT ? 1 : W::C],
                                                   T* wlds, const int wtid, T (*rbuf)[1][8 * W::CP], int (*flags)[1], const int lane,
                                                   const int cg, const bool fin, const int myslot, const T ex, const T eps, T& rc, T& rp,
                                                   int& code, int& nsteps, int& outrow) {
    constexpr int RA = W::RA, C = W::C, CP = W::CP;
    constexpr bool BANK = W::BANK;
    int cur = 0, step = 0;
    using LdsI = __attribute__((address_space(3))) int*;
    using LdsB = __attribute__((address_space(3))) unsigned char*;
    using LdsF = __attribute__((address_space(3))) T*;
    using LdsV = const __attribute__((address_space(3))) void*;
    T* const rb0 = &rbuf[0][0][0];
    constexpr unsigned BUF = 8 * CP;                          // elements per state buffer
    unsigned frd = (unsigned)(size_t)(LdsV)&flags[0][0];      // verdict word of parity 0 (parity 1: + 4)
    unsigned fwr = frd + (threadIdx.x >> 6);                  // my wave's byte of it
    asm volatile("" : "+v"(frd), "+v"(fwr));                  // (constants otherwise, moved into a VGPR every step)
    const unsigned sst = (unsigned)(size_t)(LdsV)(rb0 + myslot);            // my state slot in buffer 0
    unsigned xav = (unsigned)(size_t)(LdsV)(rb0 + cg * CP);                 // my column group's slab of buffer 0
    unsigned wav = (unsigned)(size_t)(LdsV)(wlds + wtid * 4);               // my first LDS-resident W unit
    // the lanes that finish a row, as a wave mask, and the same for the rate-bound test (none if it is off: a kernel that
    // holds one wave body runs the one with the test for every launch)
    const unsigned long long finmask = __builtin_amdgcn_ballot_w64(fin);
    const unsigned long long hardmask = (HARD && a.st.check_hard) ? finmask : 0ull;
    // log2 k of the power law in a VGPR for the whole loop (v_fma takes one SGPR operand, and that is n)
    IoConsts<T> io = a.io;
    asm volatile("" : "+v"(io.log2k));
    // partial sums of one step from state buffer PB
    auto partial_sums = [&](auto pb, T (&acc)[1][8]) {
        constexpr unsigned boff = decltype(pb)::value * BUF;
        if constexpr (W::SPLIT) sw.template matvec_at<1, W::FMA_MODE, (int)boff>(xav, wav, acc);
        else tile_matvec<T, RA, C, 1>(w, rb0 + boff, cg, acc);
        // BANK: the transpose-reduce stands right behind the FMA block, in front of the verdict and the loop's branch, so
        // that the loop carries the lane's row total (in acc[0][0]) and not the accumulators; the one of a step that is
        // never taken is discarded with its FMA block
        if constexpr (BANK) acc[0][0] = reduce_bank_f32<RA>(acc[0], lane);
    };
    // keeps the consumption of the verdict word BELOW the FMA block (see the general loop)
    auto verdict = [&](int fl, T (&acc)[1][8]) {
        asm volatile("" : "+v"(fl));
#pragma unroll
        for (int r = 0; r < (BANK ? 1 : RA); ++r) asm volatile("" : "+v"(acc[0][r]));
        return __builtin_amdgcn_readfirstlane(fl);
    };
    // go on <=> some wave has a row that is still moving and no wave has a row at the rate bound
    auto stops = [](int fu) { return !(fu & 0x01010101) || (fu & 0x02020202); };
    int stopword = 1;
    unsigned last0 = 0, last1 = 0;          // the verdict byte this wave stored last, per parity
    // One step of the loop rotated by half a step, for the parity PAR of the buffer that holds x_k = xc: [reduce, Euler
    // update and stop tests of step k: the new state xn goes to the OTHER buffer, the wave's verdict to its byte of word
    // PAR; barrier; verdict word of step k; FMA block of step k + 1; verdict].  Returns "the loop ends here": on the
    // verdict of the step just taken or at max_iter, where the FMA block of a step that is never taken is discarded
    // just as after a stop.  HARD: the launch tests the rate bound (without it the body holds no compare against hard_stop,
    // and bit 1 of the byte is never set).
    auto half_step = [&](auto par, const T xc, T& xn, T (&acc)[1][8]) {
        constexpr unsigned PAR = decltype(par)::value;
        T u;
        if constexpr (BANK) u = acc[0][0];
        else u = reduce_rows_to_lane<RA, T, W::OPAIR || W::SIXROW>(acc[0], cg);
        const T r1 = xc + (-xc + io_eval(u + ex, io)) * eps;
        // the two compares as wave masks (a NaN row counts as not moving), ANDed with the masks of the lanes that report
        const unsigned long long moving = __builtin_amdgcn_ballot_w64(abs_t(r1 - xc) >= a.st.atol);
        // (Lane counts, 0 .. 64, carried into bit 6: integer arithmetic on uniform values stays on the scalar unit, and
        // the byte then costs the vector port the one v_mov that the store needs.  Written as two tests of the masks, the
        // compiler forms it with a vector select and a vector or.)
        const unsigned nm = __builtin_popcountll(moving & finmask);
        unsigned mine = (nm + 63u) >> 6;
        if constexpr (HARD) {
            const unsigned long long beyond = __builtin_amdgcn_ballot_w64(r1 >= a.st.hard_stop);
            const unsigned nb = __builtin_popcountll(beyond & hardmask);
            mine |= ((nb + 63u) >> 5) & 2u;
        }
        unsigned& last = PAR ? last1 : last0;
        if (__builtin_expect(mine != last, 0)) {
            *(LdsB)(size_t)(fwr + 4 * PAR) = (unsigned char)mine;
            last = mine;
        }
        if (W::FLAT || fin) *(LdsF)(size_t)(sst + (unsigned)sizeof(T) * ((PAR ^ 1) * BUF)) = r1;
        xn = r1;
        __syncthreads();
        ++step;
        const int fl = *(LdsI)(size_t)(frd + 4 * PAR);
        partial_sums(std::integral_constant<unsigned, (PAR ^ 1)>{}, acc);
        stopword = verdict(fl, acc);
        return stops(stopword) || step >= a.st.max_iter;
    };
    // Unrolled by two, one body per parity; x_k alternates between two registers (no copy at the loop tail), and which
    // body ended the loop says which buffer holds the newest state.  x_k and x_{k-1} are read back from the two buffers
    // behind the loop (every lane reads what it stored itself), so neither body has to leave them in a common register.
    if (a.st.max_iter > 0) {
        T acc[1][8];
        T xe = rc, xo;
        partial_sums(std::integral_constant<unsigned, 0>{}, acc);
        for (;;) {
            if (half_step(std::integral_constant<unsigned, 0>{}, xe, xo, acc)) { cur = 1; break; }
            if (half_step(std::integral_constant<unsigned, 1>{}, xo, xe, acc)) { cur = 0; break; }
        }
    }
    // BANK: the final stores take their row from the LDS address of the lane's state slot, which the loop keeps anyway
    // (slot = (row / C) CP + row % C in the lanes that finish a row, the only ones that store): the 64-bit element index
    // of the prologue's load is then not kept across the loop, which has no register for it.
    if constexpr (BANK) {
        unsigned slot = (sst - (unsigned)(size_t)(LdsV)rb0) / (unsigned)sizeof(T);
        asm volatile("" : "+v"(slot));
        outrow = (int)((slot / CP) * C + slot % CP);
    }
    // code and step count once, from the word that ended the loop
    if (stops(stopword)) { code = (stopword & 0x01010101) ? 2 : 0; nsteps = step; }
    // nothing runs after the stop: the buffer that was read in the last update still holds x_{k-1}, the other one x_k
    if (step > 0 && fin) rp = rbuf[cur ^ 1][0][myslot];
    if (step > 0 && fin) rc = rbuf[cur][0][myslot];
}

// The Euler loop of one wave W: the tile load, the step loop of its kind (ONE workgroup barrier per step, with its stop
// protocol) and the final stores.
// wlds, wtid: the LDS image of the tile's LDS-resident rows and this thread's index in it (the workgroup's image and
// threadIdx.x; with WSO = 64 the wave's own image and the lane).
template <typename W, bool HARD = true, typename T = typename W::T>
__device__ __forceinline__ void tile_wave_body(const SolveArgs<T>& a, T* wlds, T (*rbuf)[W::NB][8 * W::CP],
                                               int (*flags)[W::NB], const int rowbase, const int wtid) {
    constexpr int RA = W::RA, C = W::C, NB = W::NB, CP = W::CP;
    constexpr bool BANK = W::BANK, SPLIT = W::SPLIT, FAST1 = W::FAST1;
    const int M = a.M, N = a.N;
    const int ngroups = (a.NB + NB - 1) / NB;
    const int b = blockIdx.x / ngroups;
    const int s0 = (blockIdx.x % ngroups) * NB;
    const int lane = threadIdx.x & 63;
    // cg: the column group whose columns this lane owns; fr: the row of its row group that it finishes (>= RA: none)
    const int cg = BANK ? bank_col_group(lane) : lane & 7;
    const int fr = BANK ? bank_row(lane) : cg;
    const int colbase = cg * C;

    // ---- prologue: my RA x C tile of W -> registers (and LDS for the last RL rows) -----------------
    T w[!SPLIT ? RA : 1][!SPLIT ? C : 1];       // plain all-register shape
    typename W::Tile sw;
    if constexpr (SPLIT) sw.template load<false>(a.W + (size_t)b * M * M, M, rowbase, colbase, wlds, wtid);
    else tile_load<T, RA, C, false>(a.W + (size_t)b * M * M, M, rowbase, colbase, w);
    // the row this lane finishes each step (a = fr: cg, or with BANK bank_row(lane)), its LDS slot, input and state
    const int myrow = rowbase + fr;
    const bool fin = (fr < RA) && (myrow < M);
    // FLAT: a lane that finishes no row stores its (meaningless) state every step all the same, to the last pad float of
    // its column group's slab: column CP - 1 >= C, which no FMA consumes -- never to a column c < C of a ragged last
    // group: those meet masked-zero W, and 0 * Inf = NaN
    const int myslot = (W::FLAT && !fin) ? cg * CP + CP - 1 : (myrow / C) * CP + (myrow % C);
    T rc[NB], rp[NB], ex[NB];            // x_k, x_{k-1} of my row; input of my row
    bool live[NB];
#pragma unroll
    for (int s = 0; s < NB; ++s) {
        live[s] = (s0 + s) < a.NB;
        const size_t vec = ((size_t)b * a.NB + (live[s] ? s0 + s : 0)) * M;
        rc[s] = (fin && live[s]) ? a.r[vec + myrow] : (T)0;
        rp[s] = rc[s];
        ex[s] = (fin && live[s]) ? a.ext[(a.ext_per_draw ? vec : (size_t)(s0 + s) * M) + myrow] : (T)0;
    }
    for (int c = threadIdx.x; c < 2 * NB * 8 * CP; c += blockDim.x) (&rbuf[0][0][0])[c] = (T)0;
    // (FAST1: two verdict words; this is also what zeroes the bytes of waves that the workgroup does not have)
    if (threadIdx.x < (FAST1 ? 2 : 3 * NB)) (&flags[0][0])[threadIdx.x] = 0;
    __syncthreads();
    if (fin) {
#pragma unroll
        for (int s = 0; s < NB; ++s) rbuf[0][s][myslot] = rc[s];
    }
    __syncthreads();

    const T eps = (myrow < N) ? a.st.eps_E : a.st.eps_I;
    int code[NB], nsteps[NB];
#pragma unroll
    for (int s = 0; s < NB; ++s) { code[s] = 1; nsteps[s] = a.st.max_iter; }
    int outrow = myrow;                  // the row of the final stores
    if constexpr (FAST1) {
        tile_loop_fp32_one<W, HARD>(a, sw, w, wlds, wtid, rbuf, flags, lane, cg, fin, myslot, ex[0], eps, rc[0], rp[0], code[0],
                                    nsteps[0], outrow);
    } else {
        // The general step loop (fp64, and more than one stimulus per workgroup).
        // Stop protocol (no vote, no second barrier, no exposed LDS latency): in iteration i every lane
        // whose row fails the convergence test (or hits the rate bound) stores 1 to flags[i%3]; the
        // verdict of iteration i is READ in iteration i+1 (the loads are issued before the FMA block and
        // consumed after it, BEFORE that iteration's state update, so rc/rp still hold x_{i+1}/x_i) and
        // slot (i+1)%3 is cleared for iteration i+1.  The FMAs of the extra iteration are discarded.
        constexpr int NQ = (C + 3) / 4;              // 16-B reads per lane per stimulus
        using V4 = T __attribute__((ext_vector_type(4)));
        bool frozen[NB];
#pragma unroll
        for (int s = 0; s < NB; ++s) frozen[s] = !live[s];
        int cur = 0;
        int step = 0;
        for (; step < a.st.max_iter; ++step) {
            int fl[NB];
            if (step > 0) {
#pragma unroll
                for (int s = 0; s < NB; ++s) fl[s] = flags[(step + 2) % 3][s];
            }
            // ---- partial sums over my C columns for my RA rows ---------------------------
            T acc[NB][8];
#pragma unroll
            for (int s = 0; s < NB; ++s)
#pragma unroll
                for (int r = 0; r < 8; ++r) acc[s][r] = (T)0;
            if constexpr (SPLIT) {
                sw.template matvec<NB, W::FMA_MODE>(wlds, wtid, &rbuf[cur][0][0], cg, acc);
            } else {
                // (tile_matvec's block, in place: through the call the fp64 kernel at C = 19 takes 255 VGPRs and not 234)
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    V4 rv[NB];
#pragma unroll
                    for (int s = 0; s < NB; ++s) {
                        rv[s] = *reinterpret_cast<const V4*>(&rbuf[cur][s][cg * CP + 4 * q]);
                    }
#pragma unroll
                    for (int s = 0; s < NB; ++s) {
                        const T rr[4] = {rv[s].x, rv[s].y, rv[s].z, rv[s].w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            if (4 * q + e < C) {
#pragma unroll
                                for (int r = 0; r < RA; ++r) acc[s][r] = fma(w[r][4 * q + e], rr[e], acc[s][r]);
                            }
                        }
                    }
                }
            }
            // ---- verdict of the previous iteration (uniform over the workgroup) -----------
            if (step > 0) {
                // keep the consumption of the flag loads BELOW the FMA block: without this tie the compiler
                // hoists the branch to the loop head and waits for the flag read before issuing the r reads
                // (two exposed LDS latencies per step instead of one)
#pragma unroll
                for (int s = 0; s < NB; ++s) {
                    asm volatile("" : "+v"(fl[s]));
#pragma unroll
                    for (int r = 0; r < RA; ++r) asm volatile("" : "+v"(acc[s][r]));
                }
                int nfrozen = 0;
#pragma unroll
                for (int s = 0; s < NB; ++s) {
                    // every lane read the same word: make the verdict (and with it frozen/code/nsteps/cur and the loop
                    // control) scalar
                    const int fu = __builtin_amdgcn_readfirstlane(fl[s]);
                    const bool fnc = fu & 0xffff, fhb = fu >> 16;
                    if (!frozen[s] && (!fnc || fhb)) {
                        code[s] = fnc ? 2 : 0;
                        nsteps[s] = step;                 // it stopped in iteration step-1
                        frozen[s] = true;
                    }
                    nfrozen += frozen[s];
                }
                if (nfrozen == NB) break;
            }
            // ---- combine the 8 column groups; lane cg ends with the total of row a = cg ----
            const int slot = step % 3;
#pragma unroll
            for (int s = 0; s < NB; ++s) {
                const T u = reduce_rows_to_lane<RA>(acc[s], cg);
                // ---- Euler update + stop tests for my row ---------------------------------
                const T fu = io_eval(u + ex[s], a.io);
                const T r1 = rc[s] + (-rc[s] + fu) * eps;
                if (fin && !frozen[s]) {
                    short* fw = reinterpret_cast<short*>(&flags[slot][s]);
                    if (abs_t(r1 - rc[s]) >= a.st.atol) fw[0] = 1;
                    if (a.st.check_hard && r1 >= a.st.hard_stop) fw[1] = 1;
                    if constexpr (NB > 1) rp[s] = rc[s];     // NB == 1: x_{k-1} is read back from LDS at the end
                    rc[s] = r1;
                }
                if (fin) rbuf[cur ^ 1][s][myslot] = rc[s];
            }
            if (threadIdx.x < NB) flags[(step + 1) % 3][threadIdx.x] = 0;
            __syncthreads();
            cur ^= 1;
        }
        // NB == 1: nothing runs after the stop, so the buffer that was read in the last update still holds x_{k-1}
        if constexpr (NB == 1) { if (step > 0 && fin) rp[0] = rbuf[cur ^ 1][0][myslot]; }
        // verdict of the last executed iteration (no extra step was taken, so no roll-back)
        if (step == a.st.max_iter && step > 0) {
#pragma unroll
            for (int s = 0; s < NB; ++s) {
                if (!frozen[s]) {
                    const int f = flags[(step + 2) % 3][s];
                    const int nc = f & 0xffff, hb = f >> 16;
                    if (!nc) { code[s] = 0; nsteps[s] = step; }
                    else if (hb) { code[s] = 2; nsteps[s] = step; }
                }
            }
        }
    }

    // ---- final stores ------------------------------------------------------------------------------
#pragma unroll
    for (int s = 0; s < NB; ++s) {
        if (!live[s]) continue;
        const size_t vec = ((size_t)b * a.NB + s0 + s) * M;
        if (fin) {
            a.r[vec + outrow] = rc[s];
            if (a.r_prev) a.r_prev[vec + outrow] = rp[s];
        }
        if (threadIdx.x == 0) {
            a.codes[(size_t)b * a.NB + s0 + s] = code[s];
            if (a.steps) a.steps[(size_t)b * a.NB + s0 + s] = nsteps[s];
        }
    }
}

template <typename T, int RA, int C, int RL, int NB, int MAXTHREADS, int MINWAVES>
__global__ void __launch_bounds__(MAXTHREADS, MINWAVES) solve_tile_kernel(SolveArgs<T> a) {
    constexpr int CP = SlabPad<C>::value;
    using Split = TileSplit<RA, C, RL>;       // RL > 0: last RL rows of every lane's tile live in LDS
    __shared__ __align__(16) T wlds[Split::lds_elems(MAXTHREADS)];
    __shared__ __align__(16) T rbuf[2][NB][8 * CP];
    // per slot and stimulus one 32-bit word: low half = "some row has not converged", high half = "some row hit
    // the rate bound"; written with 16-bit stores (no race between the two kinds), read and cleared as one word
    // (the fp32 NB = 1 loop: two words of one verdict byte per wave, see tile_wave_body)
    __shared__ int flags[tile_flag_words<T, NB>()][NB];
    if constexpr (RL > 0) set_rank_priority((blockIdx.x >> 8) % 3);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    tile_wave_body<TileWave<T, RA, C, RL, NB, false>>(a, wlds, rbuf, flags, (8 * wave + (lane >> 3)) * RA, threadIdx.x);
}

// Split shapes whose LAST wave is left with at most 40 rows (2N = 170..200 at C = 25: waves 0-2 own 56 rows each, 32 remain;
// 2N = 114..152 at C = 19: 40 remain): that wave runs an LRA-row tile (LRA = 4 or 5), all in VGPRs as packed row pairs --
// 50 (or 57) FMA instructions per step instead of 100 (76) on a 7-row tile that is mostly padding, and no LDS-resident
// rows to re-read.  Same barriers, same stop protocol, same results.
// (One stimulus per draw at C = 25 runs solve_tile_mixed6_kernel below; this kernel at C = 25 is left with NB > 1.)
template <typename T, int C, int RL, int NW, int LRA, int NB, int MINWAVES>
__global__ void __launch_bounds__(64 * NW, MINWAVES) solve_tile_mixed_kernel(SolveArgs<T> a) {
    constexpr int CP = SlabPad<C>::value;
    using Split = TileSplit<7, C, RL>;
    __shared__ __align__(16) T wlds[Split::lds_elems(64 * (NW - 1))];      // heavy waves only
    __shared__ __align__(16) T rbuf[2][NB][8 * CP];
    __shared__ int flags[tile_flag_words<T, NB>()][NB];
    set_rank_priority((blockIdx.x >> 8) % 3);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    auto body = [&](auto hard) {
        constexpr bool HARD = decltype(hard)::value;
        if (wave < NW - 1)
            tile_wave_body<TileWave<T, 7, C, RL, NB, false>, HARD>(a, wlds, rbuf, flags, (8 * wave + (lane >> 3)) * 7, threadIdx.x);
        else
            tile_wave_body<TileWave<T, LRA, C, 0, NB, true>, HARD>(a, wlds, rbuf, flags, 56 * (NW - 1) + (lane >> 3) * LRA, threadIdx.x);
    };
    if (tile_hard_split<T, NB, C == 25 && RL == 2>() && !a.st.check_hard) body(std::false_type{});
    else body(std::true_type{});
}

// 2N = 170..200 (C = 25, four waves): rows split 56/48/48/48.  Wave 0 runs the 7-row tile of the heavy waves above, waves 1-3 a
// 6-row tile of three packed row pairs and no odd row; the third pair's columns 0 .. KV - 1 stay in VGPRs (a 6-row wave has the
// registers: 100 + 2 KV against the 7-row wave's 125), the rest in LDS, so a 6-row wave re-reads 7 W units per step and not 13.
// Every wave has an LDS image of its own (64 lanes per unit).  The hardware places a workgroup's waves on the SIMDs in the cyclic
// order 0, 2, 1, 3 from a start that advances with every workgroup of the CU (tools/microbench/wave_placement.hip), so the
// 7-row waves of the three workgroups that share a CU sit on three different SIMDs: the fullest SIMD carries one 7-row and two
// 6-row waves, where 56/56/56/32 always leaves one SIMD with three 7-row waves.
template <typename T, int C, int KV, int NB, int MINWAVES>
__global__ void __launch_bounds__(256, MINWAVES) solve_tile_mixed6_kernel(SolveArgs<T> a) {
    constexpr int CP = SlabPad<C>::value;
    constexpr bool BANK = NB == 1 && sizeof(T) == 4;      // (the general loop keeps lane = 8*rg + cg)
    using Heavy = TileWave<T, 7, C, 2, NB, false, 0, 64, BANK>;
    using Six = TileWave<T, 6, C, 2, NB, false, KV, 64, BANK>;
    constexpr int HEAVY_ELEMS = Heavy::Tile::lds_elems(64), SIX_ELEMS = Six::Tile::lds_elems(64);
    static_assert(HEAVY_ELEMS % 4 == 0 && SIX_ELEMS % 4 == 0, "16-byte units");
    __shared__ __align__(16) T wlds[HEAVY_ELEMS + 3 * SIX_ELEMS];
    __shared__ __align__(16) T rbuf[2][NB][8 * CP];
    __shared__ int flags[tile_flag_words<T, NB>()][NB];
    set_rank_priority((blockIdx.x >> 8) % 3);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rg = BANK ? bank_row_group(lane) : lane >> 3;
    auto body = [&](auto hard) {
        constexpr bool HARD = decltype(hard)::value;
        if (wave == 0) tile_wave_body<Heavy, HARD>(a, wlds, rbuf, flags, rg * 7, lane);
        else tile_wave_body<Six, HARD>(a, wlds + HEAVY_ELEMS + (wave - 1) * SIX_ELEMS, rbuf, flags,
                                                                     56 + 48 * (wave - 1) + rg * 6, lane);
    };
    if (tile_hard_split<T, NB>() && !a.st.check_hard) body(std::false_type{});
    else body(std::true_type{});
}

// ---------------------------------------------------------------------------------
// dispatch: C = columns per column group (8*C >= M), RA = 7 rows per lane, waves = ceil(M / 56) <= 4.
// Shapes (fp32): "split" = RL rows of every lane's tile in LDS so that the kernel fits 168 VGPRs and
// three workgroups share a CU (C = 19: RL = 1, C = 25: RL = 2; C = 26 would need 3 x 55 KB of LDS);
// "reg" = whole tile in VGPRs (2 waves/SIMD at C >= 19).  fp64: all-register only.
// ---------------------------------------------------------------------------------
static constexpr int TILE_RA = 7;
// fp32, NB = 1, C = 25: the smallest 2N that runs rows 56/48/48/48 (solve_tile_mixed6_kernel): every size with four waves
static constexpr int TILE_MIXED6_MIN_M = 170;

static int tile_pick_c(int M, int elem_bytes) {
    const int need = (M + 7) / 8;
    const int ladder32[] = {4, 8, 13, 19, 25, 26};
    const int ladder64[] = {4, 8, 13, 19, 26};         // fp64: 2 VGPRs per value; C >= 19 runs with 4 rows per lane
    if (elem_bytes == 4) { for (int c : ladder32) if (need <= c) return c; }
    else                 { for (int c : ladder64) if (need <= c) return c; }
    return 0;
}

template <typename T>
bool tile_supported(int M, int NB) { (void)NB; return (M % 2 == 0) && tile_pick_c(M, (int)sizeof(T)) != 0; }
template bool tile_supported<float>(int, int);
template bool tile_supported<double>(int, int);

template <typename T, int RA, int C, int RL, int NB, int MINW>
static hipError_t launch_tile_k(const SolveArgs<T>& a, hipStream_t st) {
    constexpr int MAXW = (8 * C + 8 * RA - 1) / (8 * RA);
    const int waves = (a.M + 8 * RA - 1) / (8 * RA);
    const int ngroups = (a.NB + NB - 1) / NB;
    hipLaunchKernelGGL((solve_tile_kernel<T, RA, C, RL, NB, 64 * MAXW, MINW>), dim3(a.B * ngroups),
                       dim3(64 * waves), 0, st, a);
    return hipGetLastError();
}

template <typename K>
static hipError_t launch_tile_mixed(K kernel, const SolveArgs<float>& a, hipStream_t st, int blocks, int threads) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, st, a);
    return hipGetLastError();
}

// The launch rule: per element type one list of (condition -> kernel), first match wins.
// fp32, split (the default; shapes 0 and 1 are the same choice): RL rows of the tile in LDS where that is instantiated
// (C = 19, C = 25; C = 26 spills in the loop), and a lighter last wave where the uniform 7-row tile would be mostly padding.
// All-register: NB stimuli per workgroup; 7*C W registers + 8*NB accumulators + 4*NB states must stay under 256 VGPRs (no spills).
template <typename T, int C>
static hipError_t launch_tile_nb(const SolveArgs<T>& a, hipStream_t st, bool split) {
    if constexpr (sizeof(T) == 4) {
        const int waves = (a.M + 55) / 56, last_rows = a.M - 56 * (waves - 1);
        const bool mixed = SSN_TILE_MIXED && split;
        if constexpr (C == 25) {
            if (mixed && a.NB == 1 && a.M >= TILE_MIXED6_MIN_M)
                return launch_tile_mixed(solve_tile_mixed6_kernel<T, C, SSN_TILE_KV, 1, 3>, a, st, a.B, 256);
            if (mixed && waves == 4 && last_rows <= 32)
                return launch_tile_mixed(solve_tile_mixed_kernel<T, C, 2, 4, 4, 1, 3>, a, st, a.B * a.NB, 256);
            if (split) return launch_tile_k<T, TILE_RA, C, 2, 1, 3>(a, st);
        } else if constexpr (C == 19) {
            if (mixed && waves == 3 && last_rows <= 32)
                return launch_tile_mixed(solve_tile_mixed_kernel<T, C, 1, 3, 4, 1, 3>, a, st, a.B * a.NB, 192);
            if (mixed && waves == 3 && last_rows <= 40)
                return launch_tile_mixed(solve_tile_mixed_kernel<T, C, 1, 3, 5, 1, 3>, a, st, a.B * a.NB, 192);
            if (split) return launch_tile_k<T, TILE_RA, C, 1, 1, 3>(a, st);
            if (a.NB >= 4) return launch_tile_k<T, TILE_RA, C, 0, 4, 2>(a, st);
        } else if constexpr (C <= 13) {
            if (a.NB >= 4) return launch_tile_k<T, TILE_RA, C, 0, 4, 2>(a, st);
        }
        if (a.NB >= 2) return launch_tile_k<T, TILE_RA, C, 0, 2, 2>(a, st);
        return launch_tile_k<T, TILE_RA, C, 0, 1, 2>(a, st);
    } else {
        // fp64 (2 VGPRs per value).  Up to 2N = 104: 7 rows x C <= 13 columns per lane, whole tile in VGPRs.  Beyond
        // (the reference's default N = 102 gives 2N = 204, tc_gan/ssnode.py:28): 4 rows per lane and ceil(2N / 32)
        // waves -- one workgroup of up to 7 waves owns the CU, W (333 KB at 2N = 204) sits in its VGPRs and, at C = 26,
        // one row of every lane's tile in LDS (94 KB) so that the kernel stays under 256 VGPRs (two waves per SIMD).
        if constexpr (C == 26) return launch_tile_k<T, 4, C, 1, 1, 2>(a, st);
        else if constexpr (C == 19) return launch_tile_k<T, 4, C, 0, 1, 2>(a, st);
        else return launch_tile_k<T, TILE_RA, C, 0, 1, 1>(a, st);
    }
}

// shape: 0 = library default and 1 = split residency where instantiated (the same choice), 2 = all-register
template <typename T> hipError_t launch_tile(const SolveArgs<T>& a, hipStream_t st, int shape);
template <> hipError_t launch_tile<float>(const SolveArgs<float>& a, hipStream_t st, int shape) {
    const bool split = shape != 2;
    switch (tile_pick_c(a.M, 4)) {
        case 4: return launch_tile_nb<float, 4>(a, st, split);
        case 8: return launch_tile_nb<float, 8>(a, st, split);
        case 13: return launch_tile_nb<float, 13>(a, st, split);
        case 19: return launch_tile_nb<float, 19>(a, st, split);
        case 25: return launch_tile_nb<float, 25>(a, st, split);
        case 26: return launch_tile_nb<float, 26>(a, st, split);
        default: return hipErrorInvalidValue;
    }
}
template <> hipError_t launch_tile<double>(const SolveArgs<double>& a, hipStream_t st, int shape) {
    (void)shape;
    switch (tile_pick_c(a.M, 8)) {
        case 4: return launch_tile_nb<double, 4>(a, st, false);
        case 8: return launch_tile_nb<double, 8>(a, st, false);
        case 13: return launch_tile_nb<double, 13>(a, st, false);
        case 19: return launch_tile_nb<double, 19>(a, st, false);
        case 26: return launch_tile_nb<double, 26>(a, st, false);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ssn
