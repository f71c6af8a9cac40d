// Sliced Wasserstein match per condition cell (libssnode_ext2.so: ssnx2_swd_match_cells_f32).  The generated rows of a
// conditional step carry their condition; the rows of one condition -- a cell -- are few and random in number, the truth rows of
// the cell are the whole truth.  One launch matches every cell's segment of the projections with the cell's truth block by the
// quantile coupling of two samples of different sizes.  The projections come from ssn_project_rows_f32 and the coefficients go to
// ssn_swd_backproject_f32, both of libssnode.so and both indifferent to cells.
//
//   match   swd_match_cells_kernel: grid (L, C), one workgroup per (direction l, cell c).  The cell's n_c values
//           px[cell_rows[start_c + k]][l] become 64-bit keys (ordered float, local index k) padded to P(n_c); the cell's m truth
//           values stay floats padded to P(m); each array is sorted by its own call of bitonic_sort_lds.  Rank i walks the truth
//           ranks its quantile cells meet (ssn_swd_cells_dev.h); the coefficient is scaled by 1 / (L B m) -- the whole step's B --
//           and scattered to the rank's row; the n_c terms go through the ordered block sum and are divided by n_c m.
//           The cells' starts are C + 1 ints in the kernel arguments: nothing is uploaded for them, and a workgroup reads its two
//           with scalar loads.  An empty cell's workgroups write its zero loss and leave.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "ssn_host.h"
#include "ssn_ext2_host.h"
#include "ssn_swd_cells_dev.h"
#include "../../include/ssnode_mi355x_ext2.h"

namespace ssn {

static_assert(SWD_CELLS_MAX == SSNX2_SWD_MAX_CELLS, "the struct of the kernel arguments holds the header's limit");
// the largest request: 8 sort_slots(SSN_SWD_MAX_BATCH) + 4 sort_slots(SSNX2_SWD_MAX_TRUTH) bytes = 96 KiB of the CU's 160 KiB
constexpr size_t SWD_CELLS_MAX_LDS = (size_t)SSN_SWD_MAX_BATCH * sizeof(unsigned long long) + (size_t)SSNX2_SWD_MAX_TRUTH * sizeof(float);
static_assert((SSN_SWD_MAX_BATCH & (SSN_SWD_MAX_BATCH - 1)) == 0 && (SSNX2_SWD_MAX_TRUTH & (SSNX2_SWD_MAX_TRUTH - 1)) == 0 &&
              SWD_CELLS_MAX_LDS <= 160 * 1024 - 64, "the limits are their own sort_slots; the request fits a CU beside the static part");

// grid (L, C); dynamic LDS: sort_slots(largest cell) keys of 8 bytes, then Pm floats: swd_match_cell_body on direction blockIdx.x
// of cell blockIdx.y
__global__ void __launch_bounds__(256) swd_match_cells_kernel(const float* __restrict__ px, int B, const int* __restrict__ cell_rows,
                                                              SwdCellStarts starts, const float* __restrict__ py, int m, int L,
                                                              int Pm, int power, double inv, float* __restrict__ coef,
                                                              double* __restrict__ loss_cl) {
    const int c = blockIdx.y, l = blockIdx.x;
    const int s0 = starts.v[c], n = starts.v[c + 1] - s0;
    int Pn = 64;                                              // sort_slots(n): a small cell does not sort the largest one's slots
    while (Pn < n) Pn <<= 1;
    swd_match_cell_body(px, B, cell_rows + s0, n, py + (size_t)c * m * L, m, L, Pn, Pm, power, inv, coef,
                        loss_cl + (size_t)c * L + l, l);
}

hipError_t launch_swd_match_cells(const float* px, int B, const int* cell_rows, const SwdCellStarts& starts, int C, int n_max,
                                  const float* py, int m, int L, int power, float* coef, double* loss_cl, hipStream_t st) {
    if (B == 0 || L == 0 || C == 0) return hipSuccess;
    const int Pn = sort_slots(n_max), Pm = sort_slots(m);
    const size_t lds = (size_t)Pn * sizeof(unsigned long long) + (size_t)Pm * sizeof(float);
    if (lds > 64 * 1024) {
        // Above 64 KiB the kernel's dynamic LDS limit is raised once per device, to the largest request (as ssn_gw.hip does)
        static std::atomic<bool> done[64];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0) return hipErrorInvalidDevice;
        if (dev >= 64 || !done[dev].load(std::memory_order_acquire)) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(swd_match_cells_kernel),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)SWD_CELLS_MAX_LDS);
            if (e != hipSuccess) return e;
            if (dev < 64) done[dev].store(true, std::memory_order_release);
        }
    }
    const double inv = 1.0 / ((double)L * (double)B * (double)m);
    hipLaunchKernelGGL(swd_match_cells_kernel, dim3(L, C), dim3(256), lds, st, px, B, cell_rows, starts, py, m, L, Pm, power, inv,
                       coef, loss_cl);
    return hipGetLastError();
}

}  // namespace ssn
