// extern "C" surface of libssnode_ext2.so (see include/ssnode_mi355x_ext2.h): the library whose surface may grow.  No kernels
// here.  Written as ssn_capi.hip writes its own: check the arguments, refuse(entry, why) what fails, SSN_TRY(launch), return 0.
// The error string is this library's own (ssnx2_last_error).
#include <hip/hip_runtime.h>
#include <string>
#include "ssn_ext2_host.h"
#include "../../include/ssnode_mi355x_ext2.h"

namespace {

// ssnx2_last_error() of the calling thread.  Written by fail (the runtime said no) and by refuse (the entry point said no).
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

int ssnx2_abi_version(void) { return 1; }
const char* ssnx2_last_error(void) { return g_last_error.c_str(); }

int ssnx2_swd_match_cells_f32(const float* px, int B, const int* cell_rows, const int* cell_start, int C, const float* py, int m,
                              int L, int power, float* coef, double* loss_cl, void* stream) {
    const char* const fn = "ssnx2_swd_match_cells_f32";
    if (B < 0 || C < 0 || m < 0 || L < 0) return refuse(fn, "a negative size");
    if (C > SSNX2_SWD_MAX_CELLS) return refuse(fn, "more than 256 cells (their starts travel in the kernel arguments)");
    if (m > SSNX2_SWD_MAX_TRUTH) return refuse(fn, "more than 16384 truth rows per cell (their values are sorted in 64 KiB of LDS)");
    if (L > SSN_W1_MAX_DIRECTIONS) return refuse(fn, "more than 4096 directions");
    if (power != 1 && power != 2) return refuse(fn, "a power other than 1 or 2");
    if (B == 0 || L == 0 || C == 0) return 0;
    if (!cell_start) return refuse(fn, "invalid argument (null cell_start)");
    ssn::SwdCellStarts starts = {};
    int n_max = 0;
    if (cell_start[0] != 0) return refuse(fn, "cell_start does not start at 0");
    for (int c = 0; c < C; ++c) {
        const long n = (long)cell_start[c + 1] - (long)cell_start[c];
        if (n < 0) return refuse(fn, "cell_start decreases");
        if (n > SSN_SWD_MAX_BATCH) return refuse(fn, "a cell of more than 4096 generated rows (their keys are sorted in 32 KiB of LDS)");
        if (n > n_max) n_max = (int)n;
        starts.v[c] = cell_start[c];
    }
    starts.v[C] = cell_start[C];
    if (cell_start[C] != B) return refuse(fn, "cell_start does not end at B");
    if (m == 0) return refuse(fn, "no truth rows (m == 0) to match the generated rows with");
    if (!px || !cell_rows || !py || !coef || !loss_cl) return refuse(fn, "invalid argument (null pointer)");
    SSN_TRY(ssn::launch_swd_match_cells(px, B, cell_rows, starts, C, n_max, py, m, L, power, coef, loss_cl, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
