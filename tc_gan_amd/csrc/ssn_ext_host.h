// Host-side declarations shared between the kernel translation units of libssnode_ext.so and its C surface (ssn_ext_capi.hip).
// The companion library's own: ssn_host.h, which every object of libssnode.so depends on, does not know these.
#pragma once
#include <hip/hip_runtime.h>

namespace ssn {

// ssn_swd_sizes.hip (the match of n generated rows against m truth rows by the quantile coupling)
hipError_t launch_swd_match_sizes(const float* px, int n, const float* py, int m, int L, int power, float* coef, double* loss_l,
                                  hipStream_t st);

}  // namespace ssn
