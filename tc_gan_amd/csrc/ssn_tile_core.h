// Shared device pieces of the "tile" register-stationary layout (see ssn_tile.hip):
// 8x8 lane grid per wave, RA x C tile of the matrix per lane, in-wave transpose-reduce.
#pragma once
#include <hip/hip_runtime.h>
#include "ssn_device.h"

// diagnostic switch: 0 no wave priorities, 2 static priority per workgroup rank (product setting)
#ifndef SSN_PRIO_MODE
#define SSN_PRIO_MODE 2
#endif
#ifndef SSN_REDUCE4
#define SSN_REDUCE4 1            // diagnostic: 0 = 8-row transpose-reduce also for tiles of <= 4 rows
#endif

namespace ssn {

// x from the lane selected by a DPP control
template <int CTRL>
__device__ __forceinline__ float dpp_get_f(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ double dpp_get_f(double x) {
    const long long b = __builtin_bit_cast(long long, x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, true);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

// Transpose-reduce over the 8 adjacent lanes of a row group: in: 8 per-lane partial sums
// acc[0..7] (row a of the group, this lane's columns); out: lane cg holds the TOTAL of row cg.
// Each stage halves the rows a lane still carries (keep the half selected by one bit of cg, send
// the other half to the partner that keeps it): 4+2+1 = 7 DPP adds and 14 selects, instead of
// 3 DPP adds per row for all 8 rows.
template <typename T>
__device__ __forceinline__ T reduce8_to_lane(const T (&acc)[8], int cg) {
    const bool bA = cg & 4, bB = cg & 2, bC = cg & 1;
    T n4[4], n2[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const T keep = bA ? acc[k + 4] : acc[k];
        const T send = bA ? acc[k] : acc[k + 4];
        n4[k] = keep + dpp_get_f<0x141>(send);          // row_half_mirror: lane i <-> 7-i
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const T keep = bB ? n4[k + 2] : n4[k];
        const T send = bB ? n4[k] : n4[k + 2];
        n2[k] = keep + dpp_get_f<0x4E>(send);           // quad_perm:[2,3,0,1]: lane i <-> i^2
    }
    const T keep = bC ? n2[1] : n2[0];
    const T send = bC ? n2[0] : n2[1];
    return keep + dpp_get_f<0xB1>(send);                // quad_perm:[1,0,3,2]: lane i <-> i^1
}

// fp32: the first exchange without selects.  Bit 2 of the lane index (= bit 2 of cg) is a DPP bank boundary, so the
// two halves are formed by two v_add_f32_dpp, the second one writing only the lanes that keep rows 4..7
// (bank_mask 0xa = lanes 4-7 and 12-15 of every row of 16): 8 instructions instead of 12 for this stage.
// ROWS = 7: the tile has 7 rows and acc[7] is not read.  Lanes 4-7 then keep, in n4[3], the sum of their own and
// their mirror lane's partial sums of row 3 where row 7 would stand.  The second exchange sends it from lanes 4, 5 to
// lanes 6, 7, which add it to their own as n2[1], and the third leaves lane 6 with n2[0] (row 6, from both) and lane 7
// with n2[1]: lane cg = 7 of every row group is the only lane whose result has that value in it, and with 7 rows per
// row group it finishes no row (fin = cg < RA).  Lanes 0-6 hold the same bits as with a zero row.
// ROWS = 6: the same with two masked adds (rows 4 and 5).  Lanes 4-7 then keep sums of rows 2 and 3 where rows 6 and 7 would
// stand; the second exchange leaves them in lanes 6 and 7 only, which finish no row: lanes 0-5 hold the bits of two zero rows.
template <int ROWS>
__device__ __forceinline__ float reduce8_f32(const float (&acc)[8], int cg) {
    static_assert(ROWS >= 6 && ROWS <= 8, "8 rows, or 7 or 6 rows without zero rows");
    const bool bB = cg & 2, bC = cg & 1;
    float n4[4], n2[2];
    // A DPP read of a VGPR needs two wait states after the VALU write of that VGPR and the hardware does not
    // interlock; the compiler inserts them for its own DPP instructions but cannot see into inline asm.  One s_nop
    // that "redefines" all eight inputs puts every producing FMA in front of it, and with it two wait states in front
    // of every DPP read below.
    if constexpr (ROWS == 8) {
        float a0 = acc[0], a1 = acc[1], a2 = acc[2], a3 = acc[3], a4 = acc[4], a5 = acc[5], a6 = acc[6], a7 = acc[7];
        asm volatile("s_nop 1" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7));
        const float lo[4] = {a0, a1, a2, a3}, hi[4] = {a4, a5, a6, a7};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float r;
            asm("v_add_f32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=v"(r) : "v"(lo[k]));
            asm("v_add_f32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xa" : "+v"(r) : "v"(hi[k]));
            n4[k] = r;
        }
    } else {
        // The whole exchange as one statement: its inputs put every producing FMA in front of it, the s_nop gives the DPP
        // reads their two wait states, and the masked adds follow the full ones without the wait state the compiler would
        // put between two statements (they read rows 4-6, written long before, and only write n4).
#define SSN_DPP_FULL(r, a) "v_add_f32_dpp %[" r "], %[" a "], %[" a "] row_half_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
#define SSN_DPP_HIGH(r, a) "v_add_f32_dpp %[" r "], %[" a "], %[" a "] row_half_mirror row_mask:0xf bank_mask:0xa\n"
        if constexpr (ROWS == 7)
        asm("s_nop 1\n" SSN_DPP_FULL("r0", "a0") SSN_DPP_FULL("r1", "a1") SSN_DPP_FULL("r2", "a2") SSN_DPP_FULL("r3", "a3")
            SSN_DPP_HIGH("r0", "a4") SSN_DPP_HIGH("r1", "a5") SSN_DPP_HIGH("r2", "a6")
            : [r0] "=&v"(n4[0]), [r1] "=&v"(n4[1]), [r2] "=&v"(n4[2]), [r3] "=&v"(n4[3])
            : [a0] "v"(acc[0]), [a1] "v"(acc[1]), [a2] "v"(acc[2]), [a3] "v"(acc[3]), [a4] "v"(acc[4]), [a5] "v"(acc[5]), [a6] "v"(acc[6]));
        else
        asm("s_nop 1\n" SSN_DPP_FULL("r0", "a0") SSN_DPP_FULL("r1", "a1") SSN_DPP_FULL("r2", "a2") SSN_DPP_FULL("r3", "a3")
            SSN_DPP_HIGH("r0", "a4") SSN_DPP_HIGH("r1", "a5")
            : [r0] "=&v"(n4[0]), [r1] "=&v"(n4[1]), [r2] "=&v"(n4[2]), [r3] "=&v"(n4[3])
            : [a0] "v"(acc[0]), [a1] "v"(acc[1]), [a2] "v"(acc[2]), [a3] "v"(acc[3]), [a4] "v"(acc[4]), [a5] "v"(acc[5]));
#undef SSN_DPP_FULL
#undef SSN_DPP_HIGH
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float keep = bB ? n4[k + 2] : n4[k];
        const float send = bB ? n4[k] : n4[k + 2];
        n2[k] = keep + dpp_get_f<0x4E>(send);           // quad_perm:[2,3,0,1]: lane i <-> i^2
    }
    const float keep = bC ? n2[1] : n2[0];
    const float send = bC ? n2[0] : n2[1];
    return keep + dpp_get_f<0xB1>(send);                // quad_perm:[1,0,3,2]: lane i <-> i^1
}
template <>
__device__ __forceinline__ float reduce8_to_lane<float>(const float (&acc)[8], int cg) { return reduce8_f32<8>(acc, cg); }

// fp32 tiles of 7 or 6 rows with the column-group bits on lane bits 2, 3 and 0 (the waves of solve_tile_mixed6_kernel): lane l
// with bits b5 .. b0 is row group b1 | b4 << 1 | b5 << 2 and owns the columns of group bank_col_group(l) =
// ((b3 << 1) | b0) ^ (b2 ? 7 : 0).  Bits 2 and 3 of the lane index are both DPP bank bits (a bank is four lanes of a row of 16),
// so the first two exchanges make their keep / send choice with bank masks and need no selects:
//   over bit 2, per pair of rows (k, k + 4), v_add_f32_dpp row_shl:4 under bank_mask 0x5 (lanes with b2 = 0 keep row k: own +
//   lane l + 4) and row_shr:4 under bank_mask 0xa (lanes with b2 = 1 keep row k + 4: own + lane l - 4).  (row_half_mirror would
//   flip bit 1 as well, which belongs to the row group now.)
//   over bit 3, row_ror:8: one full add (row k) and one under bank_mask 0xc (lanes with b3 = 1: row k + 2).
// The third, over bit 0, keeps its two selects.  7 + 4 + 3 = 14 instructions for 7 rows and 6 + 4 + 3 = 13 for 6, where
// reduce8_f32 has 16 and 15.  The bit-2 partner owns group 7 - c, the bit-3 partner c ^ 2, the bit-0 partner c ^ 1: every row
// total is the tree of the same fp32 pairs as in reduce8_f32, ((c, 7 - c), then ^ 2, then ^ 1), bit for bit.
// Lane l ends with the total of row bank_row(l) = 4 b2 + 2 b3 + b0 of its row group; with a value nobody may use where the
// tile has no such row (the rows that are not formed: 7, or 6 and 7, and in the lanes with b2 = 1 what stands in for them).
// The first two exchanges are one statement: its s_nop gives the first DPP reads their two wait states behind the producing
// FMAs, and the order of the adds puts two instructions between every write and the DPP read of it.
__device__ __forceinline__ int bank_col_group(int l) { return (((l >> 2) & 2) | (l & 1)) ^ ((l & 4) ? 7 : 0); }
__device__ __forceinline__ int bank_row_group(int l) { return ((l >> 1) & 1) | ((l >> 3) & 6); }
__device__ __forceinline__ int bank_row(int l) { return (l & 4) | ((l >> 2) & 2) | (l & 1); }
template <int ROWS>
__device__ __forceinline__ float reduce_bank_f32(const float (&acc)[8], int lane) {
    static_assert(ROWS == 7 || ROWS == 6, "the 7- and 6-row waves");
    // In place: a masked add leaves the lanes it does not write as they are, and those are the lanes its partner add reads.
    float a0 = acc[0], a1 = acc[1], a2 = acc[2], a3 = acc[3];
#define SSN_DPP_LO(a) "v_add_f32_dpp %[" a "], %[" a "], %[" a "] row_shl:4 row_mask:0xf bank_mask:0x5\n"
#define SSN_DPP_HI(r, a) "v_add_f32_dpp %[" r "], %[" a "], %[" a "] row_shr:4 row_mask:0xf bank_mask:0xa\n"
#define SSN_DPP_ALL(a) "v_add_f32_dpp %[" a "], %[" a "], %[" a "] row_ror:8 row_mask:0xf bank_mask:0xf\n"
#define SSN_DPP_UP(r, a) "v_add_f32_dpp %[" r "], %[" a "], %[" a "] row_ror:8 row_mask:0xf bank_mask:0xc\n"
#define SSN_DPP_BIT3 SSN_DPP_ALL("a0") SSN_DPP_ALL("a1") SSN_DPP_UP("a0", "a2") SSN_DPP_UP("a1", "a3")
    if constexpr (ROWS == 7)
    asm("s_nop 1\n" SSN_DPP_LO("a3") SSN_DPP_LO("a2") SSN_DPP_LO("a0") SSN_DPP_LO("a1")
        SSN_DPP_HI("a0", "a4") SSN_DPP_HI("a1", "a5") SSN_DPP_HI("a2", "a6") SSN_DPP_BIT3
        : [a0] "+v"(a0), [a1] "+v"(a1), [a2] "+v"(a2), [a3] "+v"(a3) : [a4] "v"(acc[4]), [a5] "v"(acc[5]), [a6] "v"(acc[6]));
    else
    asm("s_nop 1\n" SSN_DPP_LO("a0") SSN_DPP_LO("a1") SSN_DPP_HI("a0", "a4") SSN_DPP_HI("a1", "a5")
        SSN_DPP_LO("a2") SSN_DPP_LO("a3") SSN_DPP_BIT3
        : [a0] "+v"(a0), [a1] "+v"(a1), [a2] "+v"(a2), [a3] "+v"(a3) : [a4] "v"(acc[4]), [a5] "v"(acc[5]));
#undef SSN_DPP_BIT3
#undef SSN_DPP_UP
#undef SSN_DPP_ALL
#undef SSN_DPP_HI
#undef SSN_DPP_LO
    const float n2[2] = {a0, a1};
    const bool b0 = lane & 1;
    const float keep = b0 ? n2[1] : n2[0];
    const float send = b0 ? n2[0] : n2[1];
    return keep + dpp_get_f<0xB1>(send);                // quad_perm:[1,0,3,2]: lane i <-> i^1
}

// Tiles of at most 4 rows (acc[4..7] == 0): the first exchange only has to fold the two halves of the lane group
// together -- four DPP adds, no second masked add, no zero inputs to materialise; lanes 0-3 end with rows 0-3.
// TRIM (fp32 tiles of 7 or 6 rows): no zero rows are formed and folded in; lanes cg >= ROWS end with values nobody may use.
template <int ROWS, typename T, bool TRIM = false>
__device__ __forceinline__ T reduce_rows_to_lane(const T (&acc)[8], int cg) {
    if constexpr (TRIM && (ROWS == 7 || ROWS == 6) && sizeof(T) == 4) return reduce8_f32<ROWS>(acc, cg);
    if constexpr (ROWS > 4 || sizeof(T) != 4 || !SSN_REDUCE4) {
        return reduce8_to_lane(acc, cg);
    } else {
        const bool bB = cg & 2, bC = cg & 1;
        T n4[4], n2[2];
#pragma unroll
        for (int k = 0; k < 4; ++k) n4[k] = acc[k] + dpp_get_f<0x141>(acc[k]);      // row_half_mirror: lane i <-> 7-i
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const T keep = bB ? n4[k + 2] : n4[k];
            const T send = bB ? n4[k] : n4[k + 2];
            n2[k] = keep + dpp_get_f<0x4E>(send);           // quad_perm:[2,3,0,1]: lane i <-> i^2
        }
        const T keep = bC ? n2[1] : n2[0];
        const T send = bC ? n2[0] : n2[1];
        return keep + dpp_get_f<0xB1>(send);                // quad_perm:[1,0,3,2]: lane i <-> i^1
    }
}

template <int C> struct SlabPad {
    // floats per column-group slab in LDS: multiple of 4 (16-B reads) with an ODD number of
    // 16-B units, so the 8 slabs start on distinct 4-bank groups (conflict-free ds_read_b128).
    static constexpr int q = (C + 3) / 4;
    static constexpr int value = 4 * ((q & 1) ? q : q + 1);
};


// acc[s][a] = sum_c w[a][c] * x_s[col(cg, c)] for the lane's RA rows: x is read from an LDS
// image laid out as 8 column-group slabs of SlabPad<C> floats per stimulus.
template <typename T, int RA, int C, int NB>
__device__ __forceinline__ void tile_matvec(const T (&w)[RA][C], const T* xs /* [NB][8*CP] */, int cg,
                                            T (&acc)[NB][8]) {
    constexpr int CP = SlabPad<C>::value;
    constexpr int NQ = (C + 3) / 4;
    using V4 = T __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int s = 0; s < NB; ++s)
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[s][r] = (T)0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        V4 rv[NB];
#pragma unroll
        for (int s = 0; s < NB; ++s) rv[s] = *reinterpret_cast<const V4*>(&xs[s * 8 * CP + cg * CP + 4 * q]);
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

// One element of a raw buffer (byte offset = voff + soff); out-of-range offsets return 0 instead of faulting.
__device__ __forceinline__ float buffer_load_elem(__amdgpu_buffer_rsrc_t rsrc, int voff, int soff, float) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, soff, 0));
}
__device__ __forceinline__ double buffer_load_elem(__amdgpu_buffer_rsrc_t rsrc, int voff, int soff, double) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rsrc, voff, soff, 0));
}

// Load the lane's RA x C tile of a row-major M x M matrix A (TRANSPOSED = false) or of its transpose
// (TRANSPOSED = true: tile element (row, col) = A[col][row]); entries outside M x M are zero.
// Buffer loads: one address VGPR per tile row (clamped row), the column as an immediate / scalar offset;
// out-of-tile columns may read the next row (or past the matrix: the buffer returns 0) and are masked.
// No per-element 64-bit addresses, no per-element branches.
template <typename T, int RA, int C, bool TRANSPOSED>
__device__ __forceinline__ void tile_load(const T* A, int M, int rowbase, int colbase, T (&w)[RA][C]) {
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(A), 0, M * M * (int)sizeof(T), 0x00020000);
    const int ncol = M - colbase;                       // columns c < ncol are inside the matrix
#pragma unroll
    for (int r = 0; r < RA; ++r) {
        const int row = rowbase + r;
        const int rowc = row < M ? row : M - 1;
        const int voff = (TRANSPOSED ? colbase * M + rowc : rowc * M + colbase) * (int)sizeof(T);
        if constexpr (!TRANSPOSED && sizeof(T) == 4) {
            // the row is contiguous in memory: 16-byte loads (a row group's 8 lanes read one matrix row back to back)
            // (bit_cast of the WHOLE vector: extracting the integer elements first is folded to a splat of one dword
            // load by this compiler)
            using V4 = float __attribute__((ext_vector_type(4)));
#pragma unroll
            for (int c4 = 0; c4 + 4 <= C; c4 += 4) {
                const V4 v = __builtin_bit_cast(V4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, c4 * 4, 0));
                w[r][c4] = v.x; w[r][c4 + 1] = v.y; w[r][c4 + 2] = v.z; w[r][c4 + 3] = v.w;
            }
#pragma unroll
            for (int c = C & ~3; c < C; ++c) w[r][c] = buffer_load_elem(rsrc, voff, c * 4, (T)0);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c)
                w[r][c] = buffer_load_elem(rsrc, voff, (TRANSPOSED ? __builtin_amdgcn_readfirstlane(c * M) : c) * (int)sizeof(T), (T)0);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) w[r][c] = (row < M && c < ncol) ? w[r][c] : (T)0;
    }
}

// ---------------------------------------------------------------------------------------------
// Split residency: the first RA-RL rows of a lane's RA x C tile stay in VGPRs, the last RL rows live in
// LDS.  At 2N = 200 (RA = 7, C = 25) the all-register tile needs 175 + ~70 VGPRs -> 2 waves/SIMD, and a
// single wave issues only one VALU instruction per ~5 cycles; with RL = 2 the kernel fits 168 VGPRs ->
// 3 waves/SIMD, three workgroups per CU (3 x 50 KB of LDS), which is what fills the VALU.
// LDS image per lane: values j = c*RL + rl (column-major over the RL rows), zero-padded to NF4 16-byte
// units; unit k of lane tid sits at base[(k*WS + tid)*4] (conflict-free, one address VGPR + immediate
// offsets).  WS = number of lanes whose row group can hold a real row (8*ceil(8C/RA), 232 of 256 at
// C = 25): the idle lanes of the last wave alias the next unit -- they never write, and what they read
// only reaches accumulators of row groups that have no rows.
// ---------------------------------------------------------------------------------------------
template <int RA, int C, int RL> struct TileSplit {
    static_assert(RL >= 0 && RL <= 2 && RL < RA, "0, 1 or 2 LDS-resident rows");
    static constexpr int RR = RA - RL;
    static constexpr int NL = RL * C;
    static constexpr int NF4 = (NL + 3) / 4;
    static constexpr int WS = 8 * ((8 * C + RA - 1) / RA);
    static constexpr int lds_elems(int wg) { return NF4 > 0 ? ((NF4 - 1) * WS + wg) * 4 : 4; }
};

// The split tile of one lane.  Register rows are stored as PAIRS of rows per column so that one
// v_pk_fma_f32 (r value broadcast to both halves through op_sel) updates two rows: a lone wave issues a
// VALU instruction only every ~4 cycles, and the packed form does twice the work per issue slot, so the
// FMA block keeps the pipe full even while the other waves of the SIMD sit at the barrier.
// At RA = 7, RL = 2: rows (0,1), (2,3) packed, row 4 plain, LDS rows (5,6) packed -> 4 instead of 7
// instructions per column.  (fp64 has no packed form; the same code compiles to scalar v_fma_f64.)
// OP (fp32 solver, C = 4k + 1): the odd row is held as PAIRS of columns, (o[c], o[c+1]) for even c, which is how the
// 16-byte read leaves r: one plain v_pk_fma_f32 per two columns into a two-float accumulator (even columns in one half,
// odd columns in the other), column C - 1 with one FMA into the low half, the row's partial sum = low + high.
// KV > 0 (fp32 solver, tiles of two register row pairs and one LDS-resident pair, 6 rows): the one-statement forms for a tile
// without an odd row, and columns [0, KV) of the LDS-resident pair held in VGPRs as well (KV a multiple of 4: whole quads).
// The LDS image then holds columns KV .. C - 1 only.
// WSO: lanes per unit of the LDS image when it is not the TileSplit's (an image of one wave: 64, tid = the lane).
// The solver's waves take OP and KV from their TileWave (ssn_tile.hip); the generator kernels use the plain form.
template <typename T, int RA, int C, int RL, bool OP = false, int KV = 0, int WSO = 0> struct SplitTile {
    using S = TileSplit<RA, C, RL>;
    static constexpr int RR = S::RR, NP = RR / 2, ODD = RR % 2;
    static_assert(!OP || (sizeof(T) == 4 && ODD && NP == 2 && RL == 2 && C % 4 == 1 && C >= 5),
                  "odd row in column pairs: 5 register rows and 2 in LDS, whole quads + one column");
    static_assert(KV >= 0 && KV % 4 == 0, "whole quads of the LDS-resident pair in VGPRs, or none");
    static constexpr bool SIX = KV > 0;
    static_assert(!SIX || (sizeof(T) == 4 && !OP && !ODD && NP == 2 && RL == 2 && C % 4 == 1 && KV + 4 <= C),
                  "two register row pairs + one split pair: whole quads and one last column, behind at least one quad from LDS");
    static constexpr int WS = WSO ? WSO : S::WS;
    static constexpr int NLV = RL * (C - KV), NU = (NLV + 3) / 4; // values and units of the LDS image per lane
    static constexpr int lds_elems(int wg) { return NU == 0 ? 4 : ((NU - 1) * WS + wg) * 4; }
    using V2 = T __attribute__((ext_vector_type(2)));
    using V4 = T __attribute__((ext_vector_type(4)));
    V2 p[NP > 0 ? NP : 1][C];      // p[k][c] = (W[row 2k][c], W[row 2k+1][c])
    T o[ODD && !OP ? C : 1];       // last register row when RR is odd (OP: its last column only)
    V2 oc[OP ? C / 2 : 1];         // OP: oc[j] = (W[odd row][2j], W[odd row][2j+1])
    V2 pv[SIX ? KV : 1];           // KV: pv[c] = (W[row RR][c], W[row RR+1][c]), c < KV

    template <bool TRANSPOSED>
    __device__ __forceinline__ void load(const T* A, int M, int rowbase, int colbase, T* wl, int tid) {
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(A), 0, M * M * (int)sizeof(T), 0x00020000);
        const int ncol = M - colbase;                       // columns c < ncol are inside the matrix
        auto row_voff = [&](int row) {
            const int rowc = row < M ? row : M - 1;
            return (TRANSPOSED ? colbase * M + rowc : rowc * M + colbase) * (int)sizeof(T);
        };
        // one tile row -> t[0..C): 16-byte buffer loads where the row is contiguous in memory (a row group's 8
        // lanes then read one whole matrix row back to back), single elements for the transposed tile / fp64
        auto fetch_row = [&](int row, T (&t)[C]) {
            const int voff = row_voff(row);
            if constexpr (!TRANSPOSED && sizeof(T) == 4) {
                // (bit_cast of the WHOLE vector: extracting the integer elements first is folded to a splat of one
                // dword load by this compiler)
#pragma unroll
                for (int c4 = 0; c4 + 4 <= C; c4 += 4) {
                    const V4 v = __builtin_bit_cast(V4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, c4 * 4, 0));
                    t[c4] = v.x; t[c4 + 1] = v.y; t[c4 + 2] = v.z; t[c4 + 3] = v.w;
                }
#pragma unroll
                for (int c = C & ~3; c < C; ++c) t[c] = buffer_load_elem(rsrc, voff, c * 4, (T)0);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c)
                    t[c] = buffer_load_elem(rsrc, voff, (TRANSPOSED ? __builtin_amdgcn_readfirstlane(c * M) : c) * (int)sizeof(T), (T)0);
            }
#pragma unroll
            for (int c = 0; c < C; ++c) t[c] = (row < M && c < ncol) ? t[c] : (T)0;
        };
        // LDS rows first, fenced off from the register rows (fewer values in flight at once)
        if (RL > 0 && tid < WS) {
            T t[RL > 0 ? RL : 1][C];
#pragma unroll
            for (int rl = 0; rl < RL; ++rl) fetch_row(rowbase + RR + rl, t[rl]);
#pragma unroll
            for (int k = 0; k < NU; ++k) {
                T v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = 4 * k + e, c = KV + j / (RL > 0 ? RL : 1), rl = j % (RL > 0 ? RL : 1);
                    v[e] = (j < NLV) ? t[rl][c] : (T)0;
                }
                V4 q; q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
                *reinterpret_cast<V4*>(&wl[((size_t)k * WS + tid) * 4]) = q;
            }
            if constexpr (SIX) {           // (tid < WS holds for every lane of an image with columns in VGPRs)
#pragma unroll
                for (int c = 0; c < KV; ++c) { pv[c].x = t[0][c]; pv[c].y = t[1][c]; }
            }
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int r = 0; r < RR; ++r) {
            T t[C];
            fetch_row(rowbase + r, t);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if constexpr (OP) {
                    if (r == RR - 1) {
                        if (c == C - 1) o[0] = t[c];
                        else if (c & 1) oc[c / 2].y = t[c];
                        else oc[c / 2].x = t[c];
                        continue;
                    }
                } else if (ODD && r == RR - 1) {
                    o[c] = t[c];
                    continue;
                }
                if (r & 1) p[r / 2][c].y = t[c];
                else p[r / 2][c].x = t[c];
            }
        }
    }

    // The packed FMAs of the two register row pairs for NC columns of one quad, as ONE asm statement.  The compiler
    // counts an asm statement as zero wait states and assumes that it may write its result through dst_sel, so between
    // two single-instruction statements of one accumulator chain it puts an s_nop unless an instruction of its own
    // happens to stand there: one per pair of FMAs in a wave that runs two chains only.  v_pk_fma_f32 writes whole
    // registers (op_sel picks SOURCE halves), dependent VALU instructions interlock, and statements a whole stage apart
    // have the LDS reads between them.  MUL: column 0 is a multiply (the accumulators are outputs only).
    // TIE: `tie` rides along as an in-out operand that no instruction touches.  It is the accumulator of the LDS-resident
    // rows, whose FMAs wait for their W units and therefore have to stay BEHIND the block that covers that wait.
    // ODDP (whole quads only): the odd row's two column pairs of the quad join the statement as a third chain, plain
    // v_pk_fma_f32 on the pairs (r0, r1) and (r2, r3); no two consecutive instructions share an accumulator.
#define SSN_PK_LO(a, w, r) "v_pk_fma_f32 %[" a "], %[" w "], %[" r "], %[" a "] op_sel_hi:[1,0,1]\n"
#define SSN_PK_HI(a, w, r) "v_pk_fma_f32 %[" a "], %[" w "], %[" r "], %[" a "] op_sel:[0,1,0] op_sel_hi:[1,1,1]\n"
#define SSN_PK_MUL(a, w, r) "v_pk_mul_f32 %[" a "], %[" w "], %[" r "] op_sel_hi:[1,0]\n"
#define SSN_PK_COL0 SSN_PK_LO("a0", "u0", "rl") SSN_PK_LO("a1", "v0", "rl")
#define SSN_PK_COL0M SSN_PK_MUL("a0", "u0", "rl") SSN_PK_MUL("a1", "v0", "rl")
#define SSN_PK_COL1 SSN_PK_HI("a0", "u1", "rl") SSN_PK_HI("a1", "v1", "rl")
#define SSN_PK_COL2 SSN_PK_LO("a0", "u2", "rh") SSN_PK_LO("a1", "v2", "rh")
#define SSN_PK_COL3 SSN_PK_HI("a0", "u3", "rh") SSN_PK_HI("a1", "v3", "rh")
#define SSN_PK_ODD01 "v_pk_fma_f32 %[ao], %[o0], %[rl], %[ao]\n"
#define SSN_PK_ODD01M "v_pk_mul_f32 %[ao], %[o0], %[rl]\n"
#define SSN_PK_ODD23 "v_pk_fma_f32 %[ao], %[o1], %[rh], %[ao]\n"
#define SSN_PK_QUAD_ODD SSN_PK_COL0 SSN_PK_ODD01 SSN_PK_COL1 SSN_PK_COL2 SSN_PK_ODD23 SSN_PK_COL3
#define SSN_PK_QUAD_ODDM SSN_PK_COL0M SSN_PK_ODD01M SSN_PK_COL1 SSN_PK_COL2 SSN_PK_ODD23 SSN_PK_COL3
#define SSN_PK_IN [rl] "v"(rlo), [rh] "v"(rhi), [u0] "v"(w0[0]), [u1] "v"(w0[NC > 1 ? 1 : 0]), [u2] "v"(w0[NC > 2 ? 2 : 0]), \
                  [u3] "v"(w0[NC > 3 ? 3 : 0]), [v0] "v"(w1[0]), [v1] "v"(w1[NC > 1 ? 1 : 0]), [v2] "v"(w1[NC > 2 ? 2 : 0]), \
                  [v3] "v"(w1[NC > 3 ? 3 : 0])
#define SSN_PK_STMT(text, how)                                                                      \
    do {                                                                                            \
        if constexpr (TIE) asm(text : [a0] how(a0), [a1] how(a1), [t] "+v"(tie) : SSN_PK_IN);       \
        else asm(text : [a0] how(a0), [a1] how(a1) : SSN_PK_IN);                                    \
    } while (0)
#define SSN_PK_STMT_ODD(text, how)                                                                                  \
    do {                                                                                                            \
        if constexpr (TIE) asm(text : [a0] how(a0), [a1] how(a1), [ao] how(ao), [t] "+v"(tie) : SSN_PK_IN, [o0] "v"(wo[0]), [o1] "v"(wo[1])); \
        else asm(text : [a0] how(a0), [a1] how(a1), [ao] how(ao) : SSN_PK_IN, [o0] "v"(wo[0]), [o1] "v"(wo[1]));    \
    } while (0)
    template <int NC, bool MUL, bool TIE, bool ODDP = false>
    static __device__ __forceinline__ void pk_block(V2& a0, V2& a1, V2& ao, V2& tie, const V2* w0, const V2* w1, const V2* wo,
                                                    const V2& rlo, const V2& rhi) {
        static_assert(NC >= 1 && NC <= 4, "columns of one 16-byte read");
        static_assert(!ODDP || NC == 4, "the odd row joins whole quads only");
        if constexpr (ODDP) {
            if constexpr (MUL) SSN_PK_STMT_ODD(SSN_PK_QUAD_ODDM, "=&v");
            else SSN_PK_STMT_ODD(SSN_PK_QUAD_ODD, "+v");
        } else if constexpr (MUL) {
            if constexpr (NC == 1) SSN_PK_STMT(SSN_PK_COL0M, "=&v");
            else if constexpr (NC == 2) SSN_PK_STMT(SSN_PK_COL0M SSN_PK_COL1, "=&v");
            else if constexpr (NC == 3) SSN_PK_STMT(SSN_PK_COL0M SSN_PK_COL1 SSN_PK_COL2, "=&v");
            else SSN_PK_STMT(SSN_PK_COL0M SSN_PK_COL1 SSN_PK_COL2 SSN_PK_COL3, "=&v");
        } else {
            if constexpr (NC == 1) SSN_PK_STMT(SSN_PK_COL0, "+v");
            else if constexpr (NC == 2) SSN_PK_STMT(SSN_PK_COL0 SSN_PK_COL1, "+v");
            else if constexpr (NC == 3) SSN_PK_STMT(SSN_PK_COL0 SSN_PK_COL1 SSN_PK_COL2, "+v");
            else SSN_PK_STMT(SSN_PK_COL0 SSN_PK_COL1 SSN_PK_COL2 SSN_PK_COL3, "+v");
        }
    }
    // The four packed FMAs of the two LDS-resident rows for one whole quad of columns, as one statement behind pk_block:
    // with the odd row inside the block the compiler has no instruction of its own left to put between them.
    // (x, y): the quad's two 16-byte W units = (row 5, row 6) of columns 0, 1 and of columns 2, 3.
    template <bool MUL>
    static __device__ __forceinline__ void lds_block(V2& al, const V4& x, const V4& y, const V2& rlo, const V2& rhi) {
        const V2 u0 = {x.x, x.y}, u1 = {x.z, x.w}, u2 = {y.x, y.y}, u3 = {y.z, y.w};
        if constexpr (MUL)
            asm(SSN_PK_MUL("a0", "u0", "rl") SSN_PK_HI("a0", "u1", "rl") SSN_PK_LO("a0", "u2", "rh") SSN_PK_HI("a0", "u3", "rh")
                : [a0] "=&v"(al) : [rl] "v"(rlo), [rh] "v"(rhi), [u0] "v"(u0), [u1] "v"(u1), [u2] "v"(u2), [u3] "v"(u3));
        else
            asm(SSN_PK_LO("a0", "u0", "rl") SSN_PK_HI("a0", "u1", "rl") SSN_PK_LO("a0", "u2", "rh") SSN_PK_HI("a0", "u3", "rh")
                : [a0] "+v"(al) : [rl] "v"(rlo), [rh] "v"(rhi), [u0] "v"(u0), [u1] "v"(u1), [u2] "v"(u2), [u3] "v"(u3));
    }
    // KV: one whole quad of columns of all three row pairs from VGPRs, as one statement: three chains, no two consecutive
    // instructions on one accumulator.
    template <bool MUL>
    static __device__ __forceinline__ void pk3_block(V2& a0, V2& a1, V2& a2, const V2* w0, const V2* w1, const V2* w2,
                                                     const V2& rlo, const V2& rhi) {
#define SSN_PK3_TAIL SSN_PK_COL1 SSN_PK_HI("a2", "x1", "rl") SSN_PK_COL2 SSN_PK_LO("a2", "x2", "rh") SSN_PK_COL3 SSN_PK_HI("a2", "x3", "rh")
#define SSN_PK3_IN [rl] "v"(rlo), [rh] "v"(rhi), [u0] "v"(w0[0]), [u1] "v"(w0[1]), [u2] "v"(w0[2]), [u3] "v"(w0[3]), [v0] "v"(w1[0]), \
                   [v1] "v"(w1[1]), [v2] "v"(w1[2]), [v3] "v"(w1[3]), [x0] "v"(w2[0]), [x1] "v"(w2[1]), [x2] "v"(w2[2]), [x3] "v"(w2[3])
        if constexpr (MUL) asm(SSN_PK_COL0M SSN_PK_MUL("a2", "x0", "rl") SSN_PK3_TAIL : [a0] "=&v"(a0), [a1] "=&v"(a1), [a2] "=&v"(a2) : SSN_PK3_IN);
        else asm(SSN_PK_COL0 SSN_PK_LO("a2", "x0", "rl") SSN_PK3_TAIL : [a0] "+v"(a0), [a1] "+v"(a1), [a2] "+v"(a2) : SSN_PK3_IN);
#undef SSN_PK3_IN
#undef SSN_PK3_TAIL
    }
#undef SSN_PK_STMT_ODD
#undef SSN_PK_STMT
#undef SSN_PK_IN

    // Per-stimulus partial sums of one matvec: the register row pairs, the odd row (ao2 with OP: even columns in .x, odd
    // columns in .y) and the LDS-resident rows (two: al2, one: al1).
    struct Sums { V2 a2[NP > 0 ? NP : 1], al2, ao2; T ao, al1; };
    // acc (op)= w2 * (r, r), r = element e of the 16-byte read (rlo, rhi).  fp32: r is taken from ONE half of the aligned
    // register pair the read left it in (op_sel broadcasts the low or the high half to both lanes of v_pk_fma_f32).  Written
    // as asm because the compiler, short of registers, copies every fourth r into a fresh pair first (one v_mov per quad and
    // accumulator group: ~15 of ~190 instructions per step).  fp64 has no packed form.
    // first (MUL0): acc = w2 * (r, r), the chain's first product (column 0 is the low half of the low pair)
    template <bool MUL0>
    static __device__ __forceinline__ void pk_bcast(V2& acc, const V2& w2, const V2& rlo, const V2& rhi, int e, bool first = false) {
        if constexpr (MUL0) {
            if (first) { asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(acc) : "v"(w2), "v"(rlo)); return; }
        }
        if constexpr (sizeof(T) == 4) {
            if (e == 0) asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(w2), "v"(rlo));
            else if (e == 1) asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(w2), "v"(rlo));
            else if (e == 2) asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(w2), "v"(rhi));
            else asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(w2), "v"(rhi));
        } else {
            const T r = e == 0 ? rlo.x : e == 1 ? rlo.y : e == 2 ? rhi.x : rhi.y;
            acc = __builtin_elementwise_fma(w2, (V2){r, r}, acc);
        }
    }

    // Quad q of columns for one stimulus in the two one-statement forms (matvec_at chooses once per instantiation between
    // them and the generic chains); rr = (rlo, rhi): the quad's x values, wu: the W units of the LDS image.
    // The one-statement block of a tile with two register row pairs: with OP the odd row's column pairs inside it and the
    // LDS-resident pair in lds_block behind it (the last column: single instructions); without OP (the light wave of the
    // mixed kernels, no LDS-resident rows) an odd row as its own chain.
    // (q is a constant once the loop is unrolled; the other branches fold away.  In the first quad under MUL0 the
    // accumulator of the LDS-resident rows does not exist yet: no tie there.)
    template <bool MUL0>
    __device__ __forceinline__ void quad_block(Sums& a, int q, const T (&rr)[4], const V2& rlo, const V2& rhi, const V4* wu) const {
        static_assert(NP == 2 && (OP || RL == 0), "two register row pairs; LDS-resident rows only behind the odd row in column pairs");
        const int nc = C - 4 * q < 4 ? C - 4 * q : 4;
        const V2 *w0 = &p[0][4 * q], *w1 = &p[1][4 * q], *wo = &oc[OP ? 2 * q : 0];
        V2 &x0 = a.a2[0], &x1 = a.a2[1], &xo = a.ao2, &t = a.al2;
        if (MUL0 && q == 0) {
            if (nc == 1) pk_block<1, true, false>(x0, x1, xo, t, w0, w1, wo, rlo, rhi);
            else if (nc == 2) pk_block<2, true, false>(x0, x1, xo, t, w0, w1, wo, rlo, rhi);
            else if (nc == 3) pk_block<3, true, false>(x0, x1, xo, t, w0, w1, wo, rlo, rhi);
            else pk_block<4, true, false, OP>(x0, x1, xo, t, w0, w1, wo, rlo, rhi);
        } else {
            if (nc == 1) pk_block<1, false, RL == 2>(x0, x1, xo, t, w0, w1, wo, rlo, rhi);
            else if (nc == 2) pk_block<2, false, RL == 2>(x0, x1, xo, t, w0, w1, wo, rlo, rhi);
            else if (nc == 3) pk_block<3, false, RL == 2>(x0, x1, xo, t, w0, w1, wo, rlo, rhi);
            else pk_block<4, false, RL == 2, OP>(x0, x1, xo, t, w0, w1, wo, rlo, rhi);
        }
        if constexpr (OP) {
            if (nc == 4) {
                if (MUL0 && q == 0) lds_block<true>(t, wu[2 * q], wu[2 * q + 1], rlo, rhi);
                else lds_block<false>(t, wu[2 * q], wu[2 * q + 1], rlo, rhi);
            } else {
                // column C - 1 into the low half, then the two halves: the odd row's partial sum
                a.ao = fma(o[0], rr[0], a.ao2.x) + a.ao2.y;
                const int j = (C - 1) * 2;
                pk_bcast<MUL0>(t, (V2){wu[j / 4][j % 4], wu[j / 4][j % 4 + 1]}, rlo, rhi, 0);
            }
        } else if (ODD) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = 4 * q + e;
                if (c < C) a.ao = (MUL0 && c == 0) ? o[c] * rr[e] : fma(o[c], rr[e], a.ao);
            }
        }
    }
    // The 6-row form.  Whole quads below KV: three register chains; then the two register pairs with the split pair's
    // accumulator tied behind them, and the split pair from its two W units (the last column: from the half-filled one).
    template <bool MUL0>
    __device__ __forceinline__ void quad_six(Sums& a, int q, const T (&rr)[4], const V2& rlo, const V2& rhi, const V4* wu) const {
        constexpr int QV = KV / 4;                            // quads of the split pair that come from VGPRs
        const int nc = C - 4 * q < 4 ? C - 4 * q : 4;
        const V2 *w0 = &p[0][4 * q], *w1 = &p[1][4 * q];
        V2 &x0 = a.a2[0], &x1 = a.a2[1], &xo = a.ao2, &t = a.al2;
        const bool first = MUL0 && q == 0;
        if (q < QV) {
            if (first) pk3_block<true>(x0, x1, t, w0, w1, &pv[SIX ? 4 * q : 0], rlo, rhi);
            else pk3_block<false>(x0, x1, t, w0, w1, &pv[SIX ? 4 * q : 0], rlo, rhi);
        } else {
            const int k = (q - QV) * 2;
            if (nc == 4) {
                if (first) { pk_block<4, true, false>(x0, x1, xo, t, w0, w1, w0, rlo, rhi); lds_block<true>(t, wu[k], wu[k + 1], rlo, rhi); }
                else { pk_block<4, false, true>(x0, x1, xo, t, w0, w1, w0, rlo, rhi); lds_block<false>(t, wu[k], wu[k + 1], rlo, rhi); }
            } else {
                pk_block<1, false, true>(x0, x1, xo, t, w0, w1, w0, rlo, rhi);
                pk_bcast<MUL0>(t, (V2){wu[k].x, wu[k].y}, rlo, rhi, 0);
            }
        }
    }

    // acc[s][a] = sum_c W[a][c] * x_s[col(cg, c)], rows a < RR from VGPRs, rows a >= RR from the LDS image.
    // Software pipeline per quad q of columns: issue the x reads of quad q+1 and the W units of quad q, run the
    // register FMAs of quad q (which cover the LDS latency), then the LDS-row FMAs.
    // MODE (fp32 only; 0 = the generator kernels' block): bit 0 = pk_block for a tile with two register row
    // pairs (a tile with OP or KV always asks for it: its odd row and, in lds_block, its LDS-resident rows are part of that
    // form); bit 1 = the first product of every chain is a multiply, so no accumulator is zeroed first.  fma(w, r, +0) and
    // w * r are the same bits unless the product is an exact zero of negative sign (+0 from the FMA, -0 from the
    // multiply); a chain can then end in -0 instead of +0 only if every one of its products is a zero, the
    // transpose-reduce adds it to the other partial sums (x + -0 = x, and -0 + +0 = +0), and a row whose partial sums are
    // all -0 meets `+ ext` before the I/O function, which maps +0 and -0 to the same rate: the state never sees the sign.
    template <int NB, int MODE = 0>
    __device__ __forceinline__ void matvec(const T* wl, int tid, const T* xs /* [NB][8*CP] */, int cg,
                                           T (&acc)[NB][8]) const {
        constexpr int CP = SlabPad<C>::value;
        using LdsT = const __attribute__((address_space(3))) T*;
        unsigned xa = (unsigned)(size_t)(LdsT)(xs + cg * CP);
        unsigned wa = (unsigned)(size_t)(LdsT)(wl + tid * 4);
        matvec_at<NB, MODE, 0>(xa, wa, acc);
    }
    // The same on the two LDS byte addresses themselves: xa = the lane's column-group slab of an x image, wa = the lane's
    // first W unit; x is read at element offset XOFF from xa.  The stage boundaries below "redefine" both addresses, and
    // they come back as redefined: a caller that keeps them as the state of a loop (the fp32 NB = 1 solver) pays no copy of
    // a loop-invariant base per call, and selects one of several x images by XOFF, an immediate of the reads.
    template <int NB, int MODE, int XOFF>
    __device__ __forceinline__ void matvec_at(unsigned& xa, unsigned& wa, T (&acc)[NB][8]) const {
        constexpr int CP = SlabPad<C>::value;
        constexpr int NQ = (C + 3) / 4;
        constexpr bool BLK = sizeof(T) == 4 && (MODE & 1) && NP == 2;
        constexpr bool MUL0 = sizeof(T) == 4 && (MODE & 2);
        static_assert(!OP || BLK, "the odd row in column pairs lives in the one-statement block");
        static_assert(!SIX || (BLK && NB == 1), "the 6-row forms are the fp32 NB = 1 solver's");
        constexpr int QV = KV / 4;                            // quads of the split pair that come from VGPRs
        // Stage boundaries are enforced with data dependencies (an empty asm that "redefines" the LDS
        // addresses and the accumulators): the reads of stage q+1 cannot be hoisted above it, the FMAs of
        // stage q cannot sink below it.  __builtin_amdgcn_sched_barrier alone is not enough -- instruction
        // selection already reorders the (side-effect free) FMAs across it and every read ends up at the top
        // (~80 staging VGPRs).  The tied values are 32-bit LDS byte addresses: tying a generic pointer would
        // lose its address space and turn every ds_read into a flat_load.
        using LdsV4 = const __attribute__((address_space(3))) V4*;
        Sums a[NB];
        if constexpr (!MUL0) {
#pragma unroll
            for (int s = 0; s < NB; ++s) {
#pragma unroll
                for (int k = 0; k < NP; ++k) a[s].a2[k] = (V2){(T)0, (T)0};
                a[s].al2 = a[s].ao2 = (V2){(T)0, (T)0};
                a[s].ao = a[s].al1 = (T)0;
            }
        }
        V4 rv[NQ][NB];
        V4 wu[NU > 0 ? NU : 1];
        auto load_quad = [&](int q) {
#pragma unroll
            for (int s = 0; s < NB; ++s) rv[q][s] = *(LdsV4)(size_t)(xa + (unsigned)sizeof(T) * (XOFF + s * 8 * CP + 4 * q));
        };
        load_quad(0);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            if (q + 1 < NQ) load_quad(q + 1);
#pragma unroll
            for (int uu = 0; uu < RL; ++uu) {                         // values 4*q*RL .. 4*(q+1)*RL - 1 (KV: of the image)
                const int k = (q - QV) * RL + uu;
                if (k >= 0 && k < NU) wu[k] = *(LdsV4)(size_t)(wa + (unsigned)sizeof(T) * (k * WS * 4));
            }
#pragma unroll
            for (int s = 0; s < NB; ++s) {
                // (r is used from the aligned register pairs the 16-byte read left it in)
                const T rr[4] = {rv[q][s].x, rv[q][s].y, rv[q][s].z, rv[q][s].w};
                const V2 rlo = {rv[q][s].x, rv[q][s].y}, rhi = {rv[q][s].z, rv[q][s].w};
                if constexpr (SIX) quad_six<MUL0>(a[s], q, rr, rlo, rhi, wu);
                else if constexpr (BLK) quad_block<MUL0>(a[s], q, rr, rlo, rhi, wu);
                else {
                    // the generic chains, one instruction per statement: the generator kernels' block (MODE = 0) and the
                    // solver shapes without two register row pairs.  (In place: as a function of its own the same
                    // statements are scheduled differently, and solve_tile_mixed_kernel at C = 19 takes two more VGPRs.)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int c = 4 * q + e;
                        if (c < C) {
#pragma unroll
                            for (int k = 0; k < NP; ++k) pk_bcast<MUL0>(a[s].a2[k], p[k][c], rlo, rhi, e, c == 0);
                            if (ODD) a[s].ao = (MUL0 && c == 0) ? o[c] * rr[e] : fma(o[c], rr[e], a[s].ao);
                        }
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int c = 4 * q + e;
                        if (c < C) {
                            if constexpr (RL == 2) {
                                const int j = c * 2;
                                const V2 wp = {wu[j / 4][j % 4], wu[j / 4][j % 4 + 1]};
                                pk_bcast<MUL0>(a[s].al2, wp, rlo, rhi, e, c == 0);
                            } else if constexpr (RL == 1) {
                                a[s].al1 = (MUL0 && c == 0) ? wu[c / 4][c % 4] * rr[e] : fma(wu[c / 4][c % 4], rr[e], a[s].al1);
                            }
                        }
                    }
                }
            }
            if (q + 1 < NQ) {
#pragma unroll
                for (int s = 0; s < NB; ++s) {
#pragma unroll
                    for (int k = 0; k < NP; ++k) asm volatile("" : "+v"(a[s].a2[k]));
                    if (OP) asm volatile("" : "+v"(a[s].ao2));
                    else if (ODD) asm volatile("" : "+v"(a[s].ao));
                    if (RL == 2) asm volatile("" : "+v"(a[s].al2));
                    if (RL == 1) asm volatile("" : "+v"(a[s].al1));
                }
                asm volatile("" : "+v"(xa), "+v"(wa));
            }
        }
#pragma unroll
        for (int s = 0; s < NB; ++s) {
#pragma unroll
            for (int r = 0; r < 8; ++r) acc[s][r] = (T)0;
#pragma unroll
            for (int k = 0; k < NP; ++k) { acc[s][2 * k] = a[s].a2[k].x; acc[s][2 * k + 1] = a[s].a2[k].y; }
            if (ODD) acc[s][RR - 1] = a[s].ao;
            if (RL == 2) { acc[s][RR] = a[s].al2.x; acc[s][RR + 1] = a[s].al2.y; }
            if (RL == 1) acc[s][RR] = a[s].al1;
        }
    }
};


// Static wave priority by the workgroup's (guessed) rank among the three workgroups sharing its CU, so that the
// arbiter prefers one workgroup's waves on all four SIMDs instead of round-robining (which keeps the co-resident
// workgroups in phase: all in their FMA block, then all in their serial part).  Worth ~2 % at the C2 shape.
__device__ __forceinline__ void set_rank_priority(int rank) {
    if (SSN_PRIO_MODE != 2) return;
    if (rank == 0) __builtin_amdgcn_s_setprio(3);
    else if (rank == 1) __builtin_amdgcn_s_setprio(2);
    else __builtin_amdgcn_s_setprio(1);
}   // all-register kernels use tile_load / tile_matvec

}  // namespace ssn
