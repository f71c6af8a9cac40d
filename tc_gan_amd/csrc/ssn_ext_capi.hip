// extern "C" surface of libssnode_ext.so (see include/ssnode_mi355x_ext.h): the entry points added after the surface of
// libssnode.so was pinned.  No kernels here.  Written as ssn_capi.hip writes its own: check the arguments, refuse(entry, why)
// what fails, SSN_TRY(launch), return 0.  The error string is this library's own (ssnx_last_error).
#include <hip/hip_runtime.h>
#include <string>
#include "ssn_ext_host.h"
#include "../../include/ssnode_mi355x_ext.h"

namespace {

// ssnx_last_error() of the calling thread.  Written by fail (the runtime said no) and by refuse (the entry point said no).
thread_local std::string g_last_error;

int fail(hipError_t e, const char* where) {
    g_last_error = std::string(where) + ": " + hipGetErrorString(e);
    return SSN_ERR_BASE + (int)e;
}
// the entry point `fn` refuses its arguments: "fn: why" is the error string, SSN_ERR_BASE + hipErrorInvalidValue the status
int refuse(const char* fn, const std::string& why) {
    g_last_error = std::string(fn) + ": " + why;
    return SSN_ERR_BASE + (int)hipErrorInvalidValue;
}
#define SSN_TRY(expr)                                     \
    do {                                                  \
        hipError_t e__ = (expr);                          \
        if (e__ != hipSuccess) return fail(e__, #expr);   \
    } while (0)

}  // namespace

extern "C" {

int ssnx_abi_version(void) { return 1; }
const char* ssnx_last_error(void) { return g_last_error.c_str(); }

int ssnx_swd_match_sizes_f32(const float* px, int n, const float* py, int m, int L, int power, float* coef, double* loss_l,
                             void* stream) {
    const char* const fn = "ssnx_swd_match_sizes_f32";
    if (n > SSN_SWD_MAX_BATCH) return refuse(fn, "more than 4096 generated rows (their keys are sorted in 32 KiB of LDS)");
    if (m > SSNX_SWD_MAX_TRUTH) return refuse(fn, "more than 16384 truth rows (their values are sorted in 64 KiB of LDS)");
    if (L > SSN_W1_MAX_DIRECTIONS) return refuse(fn, "more than 4096 directions");
    if (n < 0 || m < 0 || L < 0) return refuse(fn, "a negative size");
    if (power != 1 && power != 2) return refuse(fn, "a power other than 1 or 2");
    if ((long)n * L > 0) {
        if (m == 0) return refuse(fn, "no truth rows (m == 0) to match the generated rows with");
        if (!px || !py || !coef || !loss_l) return refuse(fn, "invalid argument (null pointer)");
    }
    SSN_TRY(ssn::launch_swd_match_sizes(px, n, py, m, L, power, coef, loss_l, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
