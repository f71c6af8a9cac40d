// Host-side declarations shared between the kernel translation units of libssnode_ext2.so and its C surface
// (ssn_ext2_capi.hip).  The second companion library's own: no object of the other two libraries depends on this file.
#pragma once
#include <hip/hip_runtime.h>

namespace ssn {

// most condition cells of one match (SSNX2_SWD_MAX_CELLS of the header): their starts travel in the kernel arguments
constexpr int SWD_CELLS_MAX = 256;
// cell c owns cell_rows[v[c] .. v[c + 1]); the entries behind v[C] are not read
struct SwdCellStarts {
    int v[SWD_CELLS_MAX + 1];
};

// ssn_swd_cells.hip (the quantile coupling of every cell's generated rows with the cell's truth rows, one launch).  `n_max` is
// the largest cell, max_c (v[c + 1] - v[c])
hipError_t launch_swd_match_cells(const float* px, int B, const int* cell_rows, const SwdCellStarts& starts, int C, int n_max,
                                  const float* py, int m, int L, int power, float* coef, double* loss_cl, hipStream_t st);

}  // namespace ssn
