// Sliced Wasserstein match of n generated rows against m truth rows, n != m allowed (libssnode_ext.so: ssnx_swd_match_sizes_f32).
// The projections come from ssn_project_rows_f32 and the coefficients go to ssn_swd_backproject_f32, both of libssnode.so and
// both indifferent to the number of truth rows; only the match had to learn it.
//
//   match   swd_match_sizes_kernel: one workgroup per direction l.  px[.][l] becomes the 64-bit keys of the equal-size match
//           (ssn_swd_dev.h: ordered float, row index), padded to Pn = sort_slots(n); py[.][l] stays floats, padded to
//           Pm = sort_slots(m); each array is sorted by its own call of bitonic_sort_lds.  Rank i of x then walks the truth ranks
//           its quantile cells [i m, (i + 1) m) meet -- ceil(m / n) or one more of them, one or two where m < n -- and adds
//           fl(w |d|) or fl(w fl(d d)) in j order; its coefficient is the sum of w sign(d) (an integer) or of fl(w (2 d)),
//           times inv, scattered to its row.  The n terms go through the ordered block sum and are divided by n m.
//           The walk of one rank is serial: with n >= 256 every thread has work and the m / n terms per rank are few; at n = 1
//           one thread reads all m values (16384 LDS reads: 0.1 ms), which is the price of one body for every size pair.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "ssn_host.h"
#include "ssn_ext_host.h"
#include "ssn_swd_sizes_dev.h"
#include "../../include/ssnode_mi355x_ext.h"

namespace ssn {

// the largest request: 8 sort_slots(SSN_SWD_MAX_BATCH) + 4 sort_slots(SSNX_SWD_MAX_TRUTH) bytes = 96 KiB of the CU's 160 KiB
constexpr size_t SWD_SIZES_MAX_LDS = (size_t)SSN_SWD_MAX_BATCH * sizeof(unsigned long long) + (size_t)SSNX_SWD_MAX_TRUTH * sizeof(float);
static_assert((SSN_SWD_MAX_BATCH & (SSN_SWD_MAX_BATCH - 1)) == 0 && (SSNX_SWD_MAX_TRUTH & (SSNX_SWD_MAX_TRUTH - 1)) == 0 &&
              SWD_SIZES_MAX_LDS <= 160 * 1024 - 64, "the limits are their own sort_slots; the request fits a CU beside the static part");

// grid (L); dynamic LDS: Pn keys of 8 bytes, then Pm floats: swd_match_sizes_body (ssn_swd_sizes_dev.h) on direction blockIdx.x
__global__ void __launch_bounds__(256) swd_match_sizes_kernel(const float* __restrict__ px, int n, const float* __restrict__ py,
                                                              int m, int L, int Pn, int Pm, int power, double inv,
                                                              float* __restrict__ coef, double* __restrict__ loss_l) {
    swd_match_sizes_body(px, n, py, m, L, Pn, Pm, power, inv, coef, loss_l, blockIdx.x);
}

hipError_t launch_swd_match_sizes(const float* px, int n, const float* py, int m, int L, int power, float* coef, double* loss_l,
                                  hipStream_t st) {
    if (n == 0 || L == 0) return hipSuccess;
    const int Pn = sort_slots(n), Pm = sort_slots(m);
    const size_t lds = (size_t)Pn * sizeof(unsigned long long) + (size_t)Pm * sizeof(float);
    if (lds > 64 * 1024) {
        // Above 64 KiB the kernel's dynamic LDS limit is raised once per device, to the largest request (as ssn_gw.hip does)
        static std::atomic<bool> done[64];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0) return hipErrorInvalidDevice;
        if (dev >= 64 || !done[dev].load(std::memory_order_acquire)) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(swd_match_sizes_kernel),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)SWD_SIZES_MAX_LDS);
            if (e != hipSuccess) return e;
            if (dev < 64) done[dev].store(true, std::memory_order_release);
        }
    }
    const double inv = 1.0 / ((double)L * (double)n * (double)m);
    hipLaunchKernelGGL(swd_match_sizes_kernel, dim3(L), dim3(256), lds, st, px, n, py, m, L, Pn, Pm, power, inv, coef, loss_l);
    return hipGetLastError();
}

}  // namespace ssn
