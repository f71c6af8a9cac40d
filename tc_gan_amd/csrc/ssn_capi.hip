// extern "C" surface of libssnode.so (see include/ssnode_mi355x.h).  No kernels here.  An entry point is written as: check the
// arguments, refuse(entry, why) what fails, fill the launcher's argument struct, SSN_TRY(launch), return 0 -- and an _f32 / _f64
// pair is ONE template body with two one-line exports.  The bodies come first, the exports after them, both
// under the banners of the header's sections.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <condition_variable>
#include <mutex>
#include <utility>
#include <string>
#include <vector>
#include "ssn_host.h"

namespace ssn {
// (the fp64 table builder lives in another kernel file under another name: one name for the pair's template)
inline hipError_t launch_build_w_table(const double* z, const double* table, double* W, int S, int B, int N, hipStream_t st) {
    return launch_build_w_table_f64(z, table, W, S, B, N, st);
}
}  // namespace ssn

namespace {

// ---- errors ---------------------------------------------------------------------------------------------------------------------
// ssn_last_error() of the calling thread.  Written by fail (the runtime said no), by refuse (the entry point said no), and by the
// two places of the drop-in solver that pass a batch's message on (SolveCombiner::submit, legacy_solve).
thread_local std::string g_last_error;

int fail(hipError_t e, const char* where) {
    g_last_error = std::string(where) + ": " + hipGetErrorString(e);
    return SSN_ERR_BASE + (int)e;
}
// the entry point `fn` refuses its arguments: "fn: why" is the error string, SSN_ERR_BASE + code the status
int refuse_as(hipError_t code, const char* fn, const std::string& why) {
    g_last_error = std::string(fn) + ": " + why;
    return SSN_ERR_BASE + (int)code;
}
int refuse(const char* fn, const std::string& why) { return refuse_as(hipErrorInvalidValue, fn, why); }
const char* const kInvalid = "invalid argument";
#define SSN_TRY(expr)                                     \
    do {                                                  \
        hipError_t e__ = (expr);                          \
        if (e__ != hipSuccess) return fail(e__, #expr);   \
    } while (0)

// J, D, S of the C surface (four values each) as the launchers take them: jds[12]
template <typename T>
void pack_jds(const T* J, const T* D, const T* S, T* jds) {
    for (int q = 0; q < 4; ++q) { jds[q] = J[q]; jds[4 + q] = D[q]; jds[8 + q] = S[q]; }
}

// ---- solver: device buffers -------------------------------------------------------------------------------------------------
// Operand precision of the AUTOMATIC kernel choice (kernel = 0, variant < 0): process-wide state behind
// ssn_set_operand_precision / ssn_get_operand_precision (include/ssnode_mi355x.h).  1 = the fp16-split matrix-core kernels
// where they apply (W and state as two fp16 parts each), 0 = fp32 operands only.  The environment variable SSN_FWD_SPLIT=0
// only sets the INITIAL value; callers change it at run time through the API and explicit kernel codes ignore it.
std::atomic<int>& operand_precision_state() {
    static std::atomic<int> st{[] { const char* e = getenv("SSN_FWD_SPLIT"); return (e && e[0] == '0') ? 0 : 1; }()};
    return st;
}
bool forward_split_default() { return operand_precision_state().load(std::memory_order_relaxed) != 0; }
long units8(int B, int NB) { return (long)B * ((NB + 7) / 8); }   // workgroups of two 4-stimulus groups each
// fp16-split kernels with two groups per unit, automatic choice: two draws per workgroup (ssn_duo.hip, 3.4 ms at C3) when that
// still gives every CU a workgroup, else one draw per workgroup (wide form, 5.3 ms at C3 but twice the workgroups)
bool duo_default(int B, int NB) { return units8(B, NB) > 256; }
template <typename T>
int solve_batch_impl(int variant, const T* W, const T* ext, int ext_per_draw, T* r, T* r_prev, int* codes,
                     int* steps, int B, int NB, int M, const ssn_solver_params* p, void* stream, bool dry_run = false) {
    // dry_run: no pointers, nothing is launched; returns the variant the call would run (ssn_solve_batch_variant_for)
    if ((B == 0 || NB == 0) && !dry_run) return 0;   // empty batch: nothing to do (pointers may be null)
    if (!p || (!dry_run && (!W || !ext || !r || !codes)) || B < 0 || NB < 0 || M <= 0 || (M & 1) || p->io_type < 0 ||
        p->io_type > 2 || p->max_iter < 0)
        return refuse("ssn_solve_batch", kInvalid);
    ssn::SolveArgs<T> a;
    a.W = W; a.ext = ext; a.r = r; a.r_prev = r_prev; a.codes = codes; a.steps = steps;
    a.ext_per_draw = ext_per_draw; a.B = B; a.NB = NB; a.M = M; a.N = M / 2;
    a.io = ssn::make_io_consts<T>(*p);
    a.st = ssn::make_step_consts<T>(*p);
    hipStream_t st = (hipStream_t)stream;
    // variant: -1 auto (MFMA for large fp32 NB >= 4 batches, else tile > regw > stream), 0 streaming, 1 register-stationary DPP, 2 tile (shape chosen by
    // the library), 3 tile with split VGPR/LDS residency where instantiated, 4 tile with the whole W tile in VGPRs,
    // 5 fp32 MFMA kernel (NB >= 4), 6 fp16-split MFMA kernel (NB >= 4, asym_tanh; wide form), 7 the same in the alternating form,
    // 8 fp16-split MFMA kernel with two draws per workgroup (ssn_duo.hip)
    const bool tile_ok = ssn::tile_supported<T>(M, NB), regw_ok = ssn::regw_supported<T>(M, NB);
    bool mfma_ok = false;
    if constexpr (sizeof(T) == 4) mfma_ok = ssn::gen_mfma_supported(M, NB);
    bool split_ok = false;
    if constexpr (sizeof(T) == 4) split_ok = mfma_ok && ssn::solve_split_supported(a);
    if ((variant == 1 && !regw_ok) || (variant >= 2 && variant <= 4 && !tile_ok) || (variant == 5 && !mfma_ok) ||
        ((variant == 6 || variant == 7 || variant == 8) && !split_ok) || variant > 8)
        return refuse("ssn_solve_batch", "requested kernel variant has no instantiation for this size");
    // auto: the MFMA solver (variant 5) for fp32 with NB >= 4 stimuli per draw, 2N above the smallest ladder size and
    // enough (draw, 8 stimuli) workgroups to fill the chip -- 71 ms at the C2/NB=8 shape against 85-90 ms for the
    // split tile kernel (which runs one workgroup per (draw, stimulus) and so keeps small batches busier)
    if (variant < 0) {
        const bool big = units8(B, NB) >= 192 && M > 104;
        const int split_variant = duo_default(B, NB) ? 8 : 6;
        variant = (mfma_ok && big) ? ((split_ok && forward_split_default()) ? split_variant : 5) : (tile_ok ? 2 : (regw_ok ? 1 : 0));
    }
    if (dry_run) return variant;
    a.split_form = variant == 7 ? 0 : ssn::gen_split_wide_parts();
    switch (variant) {
        case 2: SSN_TRY(ssn::launch_tile<T>(a, st, 0)); break;
        case 3: SSN_TRY(ssn::launch_tile<T>(a, st, 1)); break;
        case 4: SSN_TRY(ssn::launch_tile<T>(a, st, 2)); break;
        case 5: if constexpr (sizeof(T) == 4) { SSN_TRY(ssn::launch_solve_mfma(a, st)); } break;
        case 6: case 7: if constexpr (sizeof(T) == 4) { SSN_TRY(ssn::launch_solve_split(a, st)); } break;
        case 8: if constexpr (sizeof(T) == 4) { SSN_TRY(ssn::launch_solve_duo(a, st)); } break;
        case 1: SSN_TRY(ssn::launch_regw<T>(a, st)); break;
        default: SSN_TRY(ssn::launch_stream<T>(a, st)); break;
    }
    return 0;
}

// ---- solver: host buffers, per-call arenas ------------------------------------------------------------------------------------
// The reference calls its solver from up to cpu_count() Python threads at once (ssnode.py:436-459), one
// small solve per call.  Each call borrows an Arena -- a non-blocking stream, a device buffer and a pinned
// host staging buffer, all grown on demand and kept -- from a process-wide pool and gives it back on
// return: no hipMalloc / hipFree / hipDeviceSynchronize per call, calls of different threads overlap on the
// device (one stream each), and no state is shared between concurrent calls.  Arenas are never freed (the
// pool outlives every caller; tearing HIP objects down from thread or process exit hooks is not safe).
struct Arena {
    int device = -1;
    hipStream_t stream = nullptr;
    char* dev = nullptr;   size_t dev_bytes = 0;
    char* host = nullptr;  size_t host_bytes = 0;

    hipError_t reserve(size_t need_dev, size_t need_host) {
        if (!stream) {
            hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
            if (e != hipSuccess) return e;
        }
        if (need_dev > dev_bytes) {
            if (dev) { hipStreamSynchronize(stream); hipFree(dev); dev = nullptr; dev_bytes = 0; }
            const size_t n = need_dev < (1u << 20) ? (1u << 20) : need_dev + need_dev / 4;
            hipError_t e = hipMalloc((void**)&dev, n);
            if (e != hipSuccess) return e;
            dev_bytes = n;
        }
        if (need_host > host_bytes) {
            if (host) { hipStreamSynchronize(stream); hipHostFree(host); host = nullptr; host_bytes = 0; }
            const size_t n = need_host < (1u << 20) ? (1u << 20) : need_host + need_host / 4;
            hipError_t e = hipHostMalloc((void**)&host, n, hipHostMallocDefault);
            if (e != hipSuccess) return e;
            host_bytes = n;
        }
        return hipSuccess;
    }
};

class ArenaPool {
    std::mutex mu_;
    std::vector<Arena*> idle_;
public:
    Arena* acquire(int device) {
        {
            std::lock_guard<std::mutex> g(mu_);
            for (size_t i = idle_.size(); i-- > 0;)
                if (idle_[i]->device == device) {
                    Arena* a = idle_[i];
                    idle_.erase(idle_.begin() + (long)i);
                    return a;
                }
        }
        Arena* a = new Arena();
        a->device = device;
        return a;
    }
    void release(Arena* a) {
        std::lock_guard<std::mutex> g(mu_);
        idle_.push_back(a);
    }
};
ArenaPool& arena_pool() {
    static ArenaPool* pool = new ArenaPool();      // leaked on purpose, see above
    return *pool;
}
struct ArenaLease {
    Arena* a = nullptr;
    hipError_t open() {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        a = arena_pool().acquire(dev);
        return hipSuccess;
    }
    // An error return between an asynchronous copy and its wait must not hand staging memory with DMA in flight to the
    // next borrower: drain the arena's stream before it goes back to the pool (a no-op on the normal path, which has
    // already waited for its download).
    ~ArenaLease() {
        if (!a) return;
        if (a->stream) (void)hipStreamSynchronize(a->stream);
        arena_pool().release(a);
    }
};
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// Host buffers below this size go through the pinned staging buffer (one memcpy, then truly asynchronous
// copies); larger ones are handed to hipMemcpyAsync as they are (the runtime stages pageable memory itself).
constexpr size_t kStageLimit = 8u << 20;

// The device image of a solve on host buffers, [W | ext | r | r_prev | codes | steps] (the pinned staging image has the same
// offsets), and where each block lives in the caller's memory: in one buffer (ssn_solve_batch_host_*) or in one buffer per
// draw (solve_group).  A block without pieces is not copied (r_prev and steps are optional outputs).
enum SolveBlock { kW, kExt, kR, kPrev, kCodes, kSteps, kSolveBlocks };
struct HostPiece { void* host; size_t at, bytes; };      // `bytes` of a block, `at` bytes into it
struct SolveImage {
    size_t off[kSolveBlocks], total = 0;
    std::vector<HostPiece> pieces[kSolveBlocks];
    size_t r_end;                                        // W, ext and r are contiguous from 0 up to here: the inputs
    SolveImage(size_t nW, size_t nExt, size_t nR, size_t nCodes) {
        const size_t bytes[kSolveBlocks] = {nW, nExt, nR, nR, nCodes, nCodes};
        for (int b = 0; b < kSolveBlocks; ++b) { off[b] = total; total += align256(bytes[b]); }
        r_end = off[kR] + nR;
    }
    void add(SolveBlock b, const void* host, size_t at, size_t bytes) { pieces[b].push_back({const_cast<void*>(host), at, bytes}); }
    // copy(piece, offset of the piece in the image) for the pieces of the blocks first .. last, piece by piece across them
    // (draw by draw where a block has one piece per draw)
    template <typename Copy>
    hipError_t each(int first, int last, Copy&& copy) const {
        size_t most = 0;
        for (int b = first; b <= last; ++b) most = pieces[b].size() > most ? pieces[b].size() : most;
        for (size_t j = 0; j < most; ++j)
            for (int b = first; b <= last; ++b) {
                if (j >= pieces[b].size()) continue;
                const hipError_t e = copy(pieces[b][j], off[b] + pieces[b][j].at);
                if (e != hipSuccess) return e;
            }
        return hipSuccess;
    }
};
// Upload, solve (automatic kernel choice), download, on a borrowed arena.  Staged (the image fits the pinned buffer): one
// hipMemcpyAsync up to the end of r, the launch, one down from r on, one wait.  Else one copy per piece.
template <typename T>
int solve_image(const SolveImage& im, int ext_per_draw, int B, int NB, int M, const ssn_solver_params* p) {
    const bool staged = im.total <= kStageLimit;
    ArenaLease lease;
    SSN_TRY(lease.open());
    Arena& A = *lease.a;
    SSN_TRY(A.reserve(im.total, staged ? im.total : 0));
    hipStream_t st = A.stream;
    if (staged) {
        (void)im.each(kW, kR, [&](const HostPiece& h, size_t at) { std::memcpy(A.host + at, h.host, h.bytes); return hipSuccess; });
        SSN_TRY(hipMemcpyAsync(A.dev, A.host, im.r_end, hipMemcpyHostToDevice, st));
    } else {
        const auto upload = [&](const HostPiece& h, size_t at) {
            return hipMemcpyAsync(A.dev + at, h.host, h.bytes, hipMemcpyHostToDevice, st);
        };
        SSN_TRY(im.each(kW, kR, upload));
    }
    int rc = solve_batch_impl<T>(-1, (T*)(A.dev + im.off[kW]), (T*)(A.dev + im.off[kExt]), ext_per_draw, (T*)(A.dev + im.off[kR]),
                                 (T*)(A.dev + im.off[kPrev]), (int*)(A.dev + im.off[kCodes]), (int*)(A.dev + im.off[kSteps]), B, NB,
                                 M, p, st);
    if (rc) return rc;
    if (staged) {
        SSN_TRY(hipMemcpyAsync(A.host + im.off[kR], A.dev + im.off[kR], im.total - im.off[kR], hipMemcpyDeviceToHost, st));
        SSN_TRY(hipStreamSynchronize(st));
        (void)im.each(kR, kSteps, [&](const HostPiece& h, size_t at) { std::memcpy(h.host, A.host + at, h.bytes); return hipSuccess; });
    } else {
        const auto download = [&](const HostPiece& h, size_t at) {
            return hipMemcpyAsync(h.host, A.dev + at, h.bytes, hipMemcpyDeviceToHost, st);
        };
        SSN_TRY(im.each(kR, kPrev, download));
        SSN_TRY(im.each(kCodes, kSteps, download));
        SSN_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

template <typename T>
int solve_batch_host_impl(const T* W, const T* ext, int ext_per_draw, T* r, T* r_prev, int* codes, int* steps,
                          int B, int NB, int M, const ssn_solver_params* p) {
    if (B == 0 || NB == 0) return 0;
    if (!p || !W || !ext || !r || !codes || B < 0 || NB < 0 || M <= 0 || (M & 1)) return refuse("ssn_solve_batch_host", kInvalid);
    const size_t nW = (size_t)B * M * M * sizeof(T);
    const size_t nE = (size_t)(ext_per_draw ? B : 1) * NB * M * sizeof(T);
    const size_t nR = (size_t)B * NB * M * sizeof(T);
    const size_t nC = (size_t)B * NB * sizeof(int);
    SolveImage im(nW, nE, nR, nC);
    im.add(kW, W, 0, nW);
    im.add(kExt, ext, 0, nE);
    im.add(kR, r, 0, nR);
    if (r_prev) im.add(kPrev, r_prev, 0, nR);
    im.add(kCodes, codes, 0, nC);
    if (steps) im.add(kSteps, steps, 0, nC);
    return solve_image<T>(im, ext_per_draw, B, NB, M, p);
}

// ---- solver: the reference's single-solve entry point ---------------------------------------------------------------------
// One call = one (W, ext) pair = one workgroup of the fp64 kernel: latency-bound (~1 us per Euler step), and the
// runtime multiplexes streams onto a handful of hardware queues, so 16 caller threads with a stream each still run
// only ~4 solves at a time.  Calls that are in flight together are therefore COMBINED: a caller enqueues its request;
// whoever finds no leader active becomes the leader, takes every queued request with the same size and parameters,
// runs them as ONE batched launch (B = number of callers, one workgroup each) and hands the results back.  While a
// batch runs, the other threads' next calls queue up and form the next batch.  A lone caller is a batch of one.
// Results do not depend on the batching: every (draw, stimulus) pair is solved by its own workgroup with its own stop
// logic (tests/test_solver_gpu.py: batch-independence is bitwise).
struct SolveReq {
    int device, N;
    const double *W, *ext;
    double *r0, *r1;
    ssn_solver_params p;
    int code = -1, steps = 0, rc = 0;
    std::string error;                 // the batch leader's message when rc != 0 (thread-local on ITS thread)
    bool done = false;
    bool same_shape(const SolveReq& o) const {
        return device == o.device && N == o.N && p.io_type == o.p.io_type && p.max_iter == o.p.max_iter && p.k == o.p.k &&
               p.n == o.p.n && p.tau_E == o.p.tau_E && p.tau_I == o.p.tau_I && p.dt == o.p.dt && p.atol == o.p.atol &&
               p.rate_soft_bound == o.p.rate_soft_bound && p.rate_hard_bound == o.p.rate_hard_bound;
    }
};

// Solve a group of same-shaped requests in one launch.  Returns 0 or an SSN_ERR code (applies to the whole group).
int solve_group(const std::vector<SolveReq*>& grp) {
    const int B = (int)grp.size(), M = 2 * grp[0]->N;
    const size_t nW1 = (size_t)M * M * sizeof(double), nV1 = (size_t)M * sizeof(double);
    SolveImage im(B * nW1, B * nV1, B * nV1, B * sizeof(int));
    std::vector<int> cs(2 * (size_t)B);                  // codes, then steps
    for (int b = 0; b < B; ++b) {
        im.add(kW, grp[b]->W, b * nW1, nW1);
        im.add(kExt, grp[b]->ext, b * nV1, nV1);
        im.add(kR, grp[b]->r0, b * nV1, nV1);            // in: the start; out: the newest state
        im.add(kPrev, grp[b]->r1, b * nV1, nV1);         // out: the state one step before
    }
    im.add(kCodes, cs.data(), 0, B * sizeof(int));
    im.add(kSteps, cs.data() + B, 0, B * sizeof(int));
    // the group runs on ITS callers' device; the leader's own current device is put back on return
    struct DeviceScope {
        int prev = -1; bool changed = false;
        explicit DeviceScope(int want) { if (hipGetDevice(&prev) == hipSuccess && prev != want) changed = hipSetDevice(want) == hipSuccess; }
        ~DeviceScope() { if (changed) (void)hipSetDevice(prev); }
    } scope(grp[0]->device);
    int rc = solve_image<double>(im, /*ext_per_draw=*/1, B, 1, M, &grp[0]->p);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) {
        SolveReq& q = *grp[b];
        q.code = cs[b]; q.steps = cs[B + b];
        // Now r0 = newest, r1 = previous.  Which caller buffer plays "r0" after `swaps` role exchanges
        // (ssnode.c:104-106) decides where the reference would have left them.
        if (q.code == 0) {
            // converged: the newest state is copied into the current "r0" role, so BOTH buffers hold it
            std::memcpy(q.r1, q.r0, nV1);
        } else {
            // code 2: return before the exchange -> swaps = steps-1, newest is in the "r1" role.
            // code 1: all max_iter exchanges done -> newest is in the "r0" role after `steps` swaps.
            const int swaps = (q.code == 2) ? q.steps - 1 : q.steps;
            const bool r0_role_is_caller_r0 = (swaps % 2 == 0);
            const bool newest_in_r0_role = (q.code == 1);
            if (newest_in_r0_role != r0_role_is_caller_r0)
                for (int i = 0; i < M; ++i) std::swap(q.r0[i], q.r1[i]);
        }
    }
    return 0;
}

class SolveCombiner {
    std::mutex mu_;
    std::condition_variable cv_;
    bool leader_active_ = false;
    std::vector<SolveReq*> pending_;
    static constexpr size_t kMaxGroup = 256;
public:
    int submit(SolveReq& q) {
        std::unique_lock<std::mutex> lk(mu_);
        pending_.push_back(&q);
        while (!q.done) {
            if (leader_active_) { cv_.wait(lk); continue; }
            // become the leader for one batch: the oldest request and everything queued that matches it
            leader_active_ = true;
            std::vector<SolveReq*> grp, rest;
            for (SolveReq* r : pending_)
                (grp.size() < kMaxGroup && (grp.empty() || r->same_shape(*grp[0])) ? grp : rest).push_back(r);
            pending_.swap(rest);
            lk.unlock();
            int rc = solve_group(grp);
            const std::string err = g_last_error;      // the leader's thread-local message, for every member
            lk.lock();
            for (SolveReq* r : grp) { r->rc = rc; if (rc) r->error = err; r->done = true; }
            leader_active_ = false;
            cv_.notify_all();
        }
        if (q.rc) g_last_error = q.error;              // every member of a failed batch reports the batch's error
        return q.rc;
    }
};
SolveCombiner& combiner() {
    static SolveCombiner* c = new SolveCombiner();     // leaked on purpose, like the arena pool
    return *c;
}

// Leaves the caller's two buffers as ssnode.c's pointer-swapping loop would (DESIGN.md "buffer parity").
int legacy_solve(int io_type, int N, double* W, double* ext, double k, double n, double* r0, double* r1,
                 double tau_E, double tau_I, double dt, int max_iter, double atol, double soft, double hard) {
    if (N <= 0 || !W || !ext || !r0 || !r1) return refuse("solve_dynamics", kInvalid);
    if (max_iter <= 0) return 1;   // ssnode.c: loop body never runs, buffers untouched
    SolveReq q;
    q.N = N; q.W = W; q.ext = ext; q.r0 = r0; q.r1 = r1;
    q.p.io_type = io_type; q.p.max_iter = max_iter; q.p.k = k; q.p.n = n; q.p.tau_E = tau_E;
    q.p.tau_I = tau_I; q.p.dt = dt; q.p.atol = atol; q.p.rate_soft_bound = soft; q.p.rate_hard_bound = hard;
    SSN_TRY(hipGetDevice(&q.device));
    const int rc = combiner().submit(q);
    if (rc) { if (g_last_error.empty()) g_last_error = "solve_dynamics: batched launch failed"; return rc; }
    return q.code;
}

// Scalar helpers of the drop-in surface: `count` doubles in, `count_out` doubles out, one small kernel
// between them, on a borrowed arena (no allocation per call).
template <typename Launch>
bool scalar_roundtrip(const double* in, size_t n_in, double* out, size_t n_out, Launch&& launch) {
    ArenaLease lease;
    if (lease.open() != hipSuccess) return false;
    Arena& A = *lease.a;
    const size_t bytes = (n_in + n_out) * sizeof(double);
    if (A.reserve(bytes, bytes) != hipSuccess) return false;
    double* h = (double*)A.host;
    double* d = (double*)A.dev;
    std::memcpy(h, in, n_in * sizeof(double));
    if (hipMemcpyAsync(d, h, n_in * sizeof(double), hipMemcpyHostToDevice, A.stream) != hipSuccess) return false;
    if (launch(d, d + n_in, A.stream) != hipSuccess) return false;
    if (hipMemcpyAsync(h + n_in, d + n_in, n_out * sizeof(double), hipMemcpyDeviceToHost, A.stream) != hipSuccess) return false;
    if (hipStreamSynchronize(A.stream) != hipSuccess) return false;
    std::memcpy(out, h + n_in, n_out * sizeof(double));
    return true;
}

double legacy_io(int io_type, double v, double r0, double r1, double v0, double k, double n) {
    // The reference's scalar helpers take v0 explicitly (ssnode.c:25-53), so the constants are
    // filled in directly instead of being derived from the soft bound.
    ssn::IoConsts<double> c;
    c.io_type = io_type; c.k = k; c.n = n; c.v0 = v0; c.soft = r0; c.hard = r1;
    c.lin_slope = k * std::pow(v0, n - 1.0) * n;
    c.tanh_gain = n * r0 / ((r1 - r0) * v0);
    c.span = r1 - r0;
    c.span_gain = c.span * c.tanh_gain;
    c.log2k = std::log2(k);
    double out = std::numeric_limits<double>::quiet_NaN();
    scalar_roundtrip(&v, 1, &out, 1, [&](double* dv, double* dout, hipStream_t st) {
        return ssn::launch_io_eval<double>(dv, dout, 1, c, st);
    });
    return out;
}

// ---- weights and stimuli ------------------------------------------------------------------------------------------------------
// (ssn_build_w_*, ssn_build_w_philox_* and ssn_io_eval_* check nothing: a null J / D / S or p is read on the host)
template <typename T>
int build_w_impl(const T* z, const T* J, const T* D, const T* S, T* W, int B, int N, void* stream) {
    T jds[12];
    pack_jds(J, D, S, jds);
    SSN_TRY(ssn::launch_build_w<T>(z, jds, W, B, N, (hipStream_t)stream));
    return 0;
}
template <typename T>
int build_w_philox_impl(unsigned long long seed, unsigned long long offset, const T* J, const T* D, const T* S, T* W, T* z, int B,
                        int N, void* stream) {
    T jds[12];
    pack_jds(J, D, S, jds);
    SSN_TRY(ssn::launch_build_w_philox<T>(seed, offset, jds, W, z, B, N, (hipStream_t)stream));
    return 0;
}
// S parameter sets on one shared noise draw; `fn`: the pair's messages name the entry with its suffix
template <typename T>
int build_w_table_impl(const char* fn, const T* z, const T* jds_table, T* W, int S, int B, int N, void* stream) {
    if (S < 0 || B < 0 || N < 1 || ((long)S * B > 0 && (!z || !jds_table || !W))) return refuse(fn, kInvalid);
    SSN_TRY(ssn::launch_build_w_table(z, jds_table, W, S, B, N, (hipStream_t)stream));
    return 0;
}
// amp: null for the plain stimulus (ssn_stimulus_*), the per-draw amplitudes of ssn_stimulus_amp_*
template <typename T>
int stimulus_impl(const T* bw, const T* con, T smoothness, const T* amp, T* ext, int B, int NB, int N, void* stream) {
    SSN_TRY(ssn::launch_stimulus<T>(bw, con, smoothness, amp, ext, B, NB, N, (hipStream_t)stream));
    return 0;
}
template <typename T>
int io_eval_impl(const T* v, T* out, long count, const ssn_solver_params* p, void* stream) {
    SSN_TRY(ssn::launch_io_eval<T>(v, out, count, ssn::make_io_consts<T>(*p), (hipStream_t)stream));
    return 0;
}

// ---- the fixed-time generator: one choice of kernels ---------------------------------------------------------
// gen_forward_path and gen_backward_path are the ONLY places that decide which kernels run a generator pass.  Both validate all
// but the pointers, fill the arg struct and answer in the numbering of ssn_gen_forward_variant (1 tile / stream, 2 / 3 fp32 MFMA,
// 4 - 7 fp16-split MFMA, 8 two draws per workgroup), or refuse: >= SSN_ERR_BASE with the error string set.
template <typename T>
ssn::IoConsts<T> gen_io_consts(const ssn_gen_params& g) {
    ssn_solver_params p;
    std::memset(&p, 0, sizeof(p));
    p.io_type = g.io_type; p.k = g.k; p.n = g.n; p.rate_soft_bound = g.rate_soft_bound; p.rate_hard_bound = g.rate_hard_bound;
    return ssn::make_io_consts<T>(p);
}
const char* const kGenInvalid = "invalid argument, unsupported size or kernel not one of 0 (automatic), 1 (tile), 2 / 3 (fp32 MFMA), "
                                "4 / 5 / 6 (fp16-split), 8 (two-draw)";
const char* const kGenMfma = "the MFMA kernels need fp32, NB >= 4, 2N <= 208 and NB T 2N < 2^29";
template <typename T>
bool gen_call_ok(int M, const ssn_gen_params* g) {
    return g && M > 0 && !(M & 1) && g->seqlen >= 1 && g->skip_steps >= 0 && g->skip_steps < g->seqlen && g->kernel >= 0 &&
           g->kernel <= 8 && g->kernel != 7 && ssn::gen_supported<T>(M);
}
template <typename T, typename Args>   // what GenFwdArgs and GenBwdArgs take from the call's shape and parameters
void gen_fill(Args& a, int B, int NB, int M, const ssn_gen_params& g) {
    a.B = B; a.NB = NB; a.M = M; a.seqlen = g.seqlen; a.skip = g.skip_steps;
    a.eps_E = (T)(g.dt / g.tau_E); a.eps_I = (T)(g.dt / g.tau_I); a.theta = (T)g.rate_penalty_threshold;
}
// 4-stimulus groups per workgroup of a matrix-core launch: what the code names, or for 0 what fills the chip -- two when that
// already gives >= 192 workgroups, one when only that does (128 draws x 8 stimuli of the paper's runs), else 0: the tile
// kernels, which run one workgroup per (draw, stimulus)
int gen_groups(int kernel, int B, int NB) {
    if (kernel) return kernel == 1 ? 0 : (kernel == 3 || kernel == 5 ? 1 : 2);
    return units8(B, NB) >= 192 ? 2 : ((long)B * ((NB + 3) / 4) >= 192 ? 1 : 0);
}
// save: the call stores trajectory and f' (their stores address one draw's block with 32-bit byte offsets)
template <typename T>
int gen_forward_path(ssn::GenFwdArgs<T>& a, int B, int NB, int M, bool save, const ssn_gen_params* g) {
    if (!gen_call_ok<T>(M, g) || g->io_type < 0 || g->io_type > 2) return refuse("ssn_gen_forward", kGenInvalid);
    gen_fill<T>(a, B, NB, M, *g);
    a.io = gen_io_consts<T>(*g);
    if constexpr (sizeof(T) == 4) {
        const int k = g->kernel;
        const bool mfma_ok = ssn::gen_mfma_supported(M, NB) && (!save || (long)NB * g->seqlen * M < (1L << 29));
        const bool split_ok = mfma_ok && ssn::gen_split_rshift(a) >= 0;
        if (k >= 2 && !mfma_ok) return refuse("ssn_gen_forward", kGenMfma);
        if (k >= 4 && !split_ok)
            return refuse("ssn_gen_forward", "the fp16-split MFMA kernels need asym_tanh, rate_hard_bound < 3e4 and dt <= tau");
        const int groups = mfma_ok ? gen_groups(k, B, NB) : 0;
        if (!groups) return 1;
        a.mfma_groups = groups;
        if (k == 2 || k == 3 || (k == 0 && !(split_ok && forward_split_default()))) return groups == 2 ? 2 : 3;
        if (groups == 1) return 5;
        if (k == 8 || (k == 0 && duo_default(B, NB))) return 8;
        a.split_form = k == 6 ? 0 : ssn::gen_split_wide_parts();
        return a.split_form == 0 ? 6 : (a.split_form == 3 ? 7 : 4);
    }
    return 1;
}
// NOT the forward's rule: the fp16-split sweep (one form: code 6 runs 4) and the two-draw sweep scale by the data, not by a rate
// bound, so they take any I/O function -- with asym_power under the default operand precision the automatic adjoint is the
// split or two-draw sweep behind an fp32 MFMA forward.
template <typename T>
int gen_backward_path(ssn::GenBwdArgs<T>& a, int B, int NB, int M, const ssn_gen_params* g) {
    if (!gen_call_ok<T>(M, g)) return refuse("ssn_gen_backward", kGenInvalid);
    gen_fill<T>(a, B, NB, M, *g);
    if constexpr (sizeof(T) == 4) {
        const int k = g->kernel;
        const bool mfma_ok = ssn::gen_mfma_supported(M, NB) && (long)NB * g->seqlen * M < (1L << 29);
        if (k >= 2 && !mfma_ok) return refuse("ssn_gen_backward", kGenMfma);
        const int groups = mfma_ok ? gen_groups(k, B, NB) : 0;
        if (!groups) return 1;
        a.mfma_groups = groups;
        if (k == 2 || k == 3 || (k == 0 && !forward_split_default())) return groups == 2 ? 2 : 3;
        if (k == 8 || (k == 0 && duo_default(B, NB))) return 8;
        return groups == 2 ? 4 : 5;
    }
    return 1;
}

template <typename T>
int gen_forward_impl(const T* W, const T* ext, T* time_avg, T* dyn_row, T* rate_row, T* traj, T* df, int B, int NB,
                     int M, const ssn_gen_params* g, void* stream) {
    if (B == 0 || NB == 0) return 0;
    if (!W || !ext || !time_avg || !dyn_row || !rate_row || (traj == nullptr) != (df == nullptr))
        return refuse("ssn_gen_forward", kGenInvalid);
    ssn::GenFwdArgs<T> a;
    a.W = W; a.ext = ext; a.time_avg = time_avg; a.dyn_row = dyn_row; a.rate_row = rate_row; a.traj = traj; a.df = df;
    const int variant = gen_forward_path(a, B, NB, M, traj != nullptr, g);
    if (variant >= SSN_ERR_BASE) return variant;
    hipStream_t st = (hipStream_t)stream;
    if constexpr (sizeof(T) == 4) switch (variant) {
        case 2: case 3: SSN_TRY(ssn::launch_gen_forward_mfma(a, st)); return 0;
        case 4: case 5: case 6: case 7: SSN_TRY(ssn::launch_gen_forward_split(a, st)); return 0;
        case 8: SSN_TRY(ssn::launch_gen_forward_duo(a, st)); return 0;
    }
    SSN_TRY(ssn::launch_gen_forward<T>(a, st));
    return 0;
}

template <typename T>
int gen_backward_impl(const T* W, const T* traj, T* delta, const T* gta, T* g_ext, double c_dyn, double c_rate, int B,
                      int NB, int M, const ssn_gen_params* g, void* stream, float* dmax = nullptr, int* tracked = nullptr) {
    if (tracked) *tracked = 0;
    if (B == 0 || NB == 0) return 0;
    if (!W || !traj || !delta || !gta) return refuse("ssn_gen_backward", kGenInvalid);
    ssn::GenBwdArgs<T> a;
    a.W = W; a.traj = traj; a.delta = delta; a.g_time_avg = gta; a.g_ext = g_ext; a.c_dyn = (T)c_dyn; a.c_rate = (T)c_rate;
    const int variant = gen_backward_path(a, B, NB, M, g);
    if (variant >= SSN_ERR_BASE) return variant;
    hipStream_t st = (hipStream_t)stream;
    if constexpr (sizeof(T) == 4) {
        if (variant >= 4 && dmax && tracked) {       // max |delta| per draw for ssn_weight_grad_scaled_f32 (atomic max of bit
            SSN_TRY(hipMemsetAsync(dmax, 0, sizeof(float) * (size_t)B, st));   // patterns): the fp16-split sweeps keep it for
            a.dmax = reinterpret_cast<unsigned*>(dmax);                         // their own scaling
            *tracked = 1;
        }
        switch (variant) {
            case 2: case 3: SSN_TRY(ssn::launch_gen_backward_mfma(a, st)); return 0;
            case 4: case 5: SSN_TRY(ssn::launch_gen_backward_split(a, st)); return 0;
            case 8: SSN_TRY(ssn::launch_gen_backward_duo(a, st)); return 0;
        }
    }
    SSN_TRY(ssn::launch_gen_backward<T>(a, st));
    return 0;
}

// ---- weight and parameter gradients ---------------------------------------------------------------------------------------------
template <typename T>
int weight_grad_impl(const T* delta, const T* traj, T* gW, int B, long K, int M, int kernel, void* stream) {
    if (B < 0 || K < 0 || M < 0 || (B > 0 && M > 0 && (!gW || (K > 0 && (!delta || !traj)))))
        return refuse("ssn_weight_grad", kInvalid);
    SSN_TRY(ssn::launch_weight_grad<T>(delta, traj, gW, B, K, M, kernel, (hipStream_t)stream));
    return 0;
}
template <typename T>       // (no check: a null J / D / S is read on the host)
int jds_grad_impl(const T* gW, const T* z, const T* J, const T* D, const T* S, double* out, int B, int N, void* stream) {
    T jds[12];
    pack_jds(J, D, S, jds);
    SSN_TRY(ssn::launch_jds_grad<T>(gW, z, jds, out, B, N, (hipStream_t)stream));
    return 0;
}
template <typename T>
int probe_scatter_impl(const T* g, const long* ids, const long* probes, T* g_ta, int n, int B, int NB, int M, void* stream) {
    if (n < 0 || B < 0 || NB < 0 || M < 0 || ((long)B * NB * M > 0 && !g_ta) || (n > 0 && (!g || !ids || !probes)))
        return refuse("ssn_probe_scatter", kInvalid);
    SSN_TRY(ssn::launch_probe_scatter<T>(g, ids, probes, g_ta, n, B, NB, M, (hipStream_t)stream));
    return 0;
}
// The penalty means, and with nsamp > 0 the gather of the probed tuning curves in the same launch (the _probe entries, which
// refuse under their own name `fn`).  The plain entries are the probe form with nsamp = NB = M = 0 and no probe pointers.
template <typename T>
int penalty_means_impl(const char* fn, const T* dyn, const T* rate, long n, double scale_dyn, double scale_rate, double* ws,
                       double* out, const T* time_avg, const long* ids, const long* probes, T* tc, int nsamp, int NB, int M,
                       void* stream) {
    if (n < 0 || !ws || !out || (n > 0 && (!dyn || !rate)) || nsamp < 0 || NB < 0 || M < 0 ||
        (nsamp > 0 && (!time_avg || !ids || !probes || !tc)))
        return refuse(fn, kInvalid);
    SSN_TRY(ssn::launch_penalty_means<T>(dyn, rate, n, scale_dyn, scale_rate, ws, out, (hipStream_t)stream, time_avg, ids, probes,
                                         nsamp > 0 ? tc : nullptr, nsamp, NB, M));
    return 0;
}
// gate, gate_bound: the critic step that is dropped on the device (ssn_critic_step_gated_run); clip_lo_v .. record_tail: the
// per-element bounds and the record of a generator step (ssn_gen_apply_f32).  All null for ssn_optimizer_step.
int optimizer_step_full(float* p, const float* g, float* s1, float* s2, long n, const ssn_opt_params* o, const double* gate,
                        double gate_bound, const float* clip_lo_v, const float* clip_hi_v, float* record, const float* record_tail,
                        void* stream) {
    if (!o || n < 0 || o->kind < 0 || o->kind > 2) return refuse("ssn_optimizer_step", kInvalid);
    ssn::OptArgs a;
    a.gate = gate; a.gate_bound = gate_bound;
    a.clip_lo_v = clip_lo_v; a.clip_hi_v = clip_hi_v; a.record = record; a.record_tail = record_tail;
    a.p = p; a.g = g; a.s1 = s1; a.s2 = s2; a.n = n; a.kind = o->kind;
    a.lr = (float)o->learning_rate; a.beta1 = (float)o->beta1; a.beta2 = (float)o->beta2; a.eps = (float)o->epsilon;
    a.rho = (float)o->rho;
    // lasagne.updates.adam: a_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t)
    a.a_t = (float)(o->learning_rate * std::sqrt(1.0 - std::pow(o->beta2, o->step)) / (1.0 - std::pow(o->beta1, o->step)));
    a.l2_penalty = (float)o->reg_l2_penalty; a.l1_penalty = (float)o->reg_l1_penalty;
    a.l2_decay = (float)o->reg_l2_decay; a.l1_decay = (float)o->reg_l1_decay;
    a.clip = o->clip; a.clip_lo = (float)o->clip_lo; a.clip_hi = (float)o->clip_hi;
    a.skip_nonfinite = (o->reserved & 1) && n <= 64 && record;        // ssn_opt_params.reserved bit 0 (ssn_gen_apply_f32)
    SSN_TRY(ssn::optimizer_step(a, (hipStream_t)stream));
    return 0;
}

// ---- the WGAN-GP critic: one description, one choice of kernels ---------------------------------------------------------------
// Every exported critic pass describes its critic as an ssn::CriticSpec (ssn_host.h, built by one helper per family of entry
// points further down) and goes through the four functions below; critic_path is the ONLY place that decides which kernels
// compute a critic.  The back ends read the flat parameter vector through ssn::critic_layout (ssn_host.h), the ONLY walk of it.
using ssn::CriticSpec;
// Critics whose layers are all <= 128 wide fit the fused row-block kernels (ssn_critic_fused.hip: 3 launches per update, fp32
// arithmetic whatever `precision` says).  Above ~2048 stacked rows the layer-by-layer chain (fixed ~250 us of launch latency,
// MFMA arithmetic) is as fast as they are (plain FMAs, time proportional to the rows).  SSN_CRITIC_FUSED=0 in the environment
// switches them off (A/B timing, tests of the other paths).
bool fused_ok(const int* dims, int nlayers, long rows) {
    static const bool enabled = [] { const char* v = std::getenv("SSN_CRITIC_FUSED"); return !(v && v[0] == '0'); }();
    return enabled && rows <= 2048 && ssn::critic_fused_supported(dims, nlayers);
}
// Fused: the row-block kernels above (rectify, with or without layer normalisation; conditional critics only).
// Plain: the layer-by-layer MFMA GEMM chain of ssn_critic.hip (plain layers, any slope; wide layers take its row-block form,
//        ssn_critic_rows.hip, inside ssn::critic_loss_grad).
// General: the chain of ssn_critic_ln.hip (layer normalisation, scales, smooth nonlinearities).
enum class CriticPath { Fused, Plain, General };
// rows: the stacked rows of the pass; conds: every condition pointer of the call is given
CriticPath critic_path(const CriticSpec& net, long rows, bool conds) {
    bool norm = false, scaled = false;
    for (int l = 0; net.flags && l < net.nlayers; ++l) { norm = norm || (net.flags[l] & 1); scaled = scaled || (net.flags[l] & 2); }
    if (scaled || net.act >= 4 || (norm && net.leak != 0.f)) return CriticPath::General;
    if (!norm && net.leak != 0.f) return CriticPath::Plain;        // (the fused kernels have no slope)
    if (conds && fused_ok(net.dims, net.nlayers, rows)) return CriticPath::Fused;
    return norm ? CriticPath::General : CriticPath::Plain;
}
int critic_net_forward(const CriticSpec& n, const float* x, const float* cond, int batch, float* out, float* ws, hipStream_t st) {
    switch (critic_path(n, batch, cond != nullptr)) {
    case CriticPath::Fused: SSN_TRY(ssn::critic_fused_forward(n, x, cond, batch, out, ws, st)); break;
    case CriticPath::Plain: SSN_TRY(ssn::critic_forward(n, x, cond, batch, out, ws, st)); break;
    case CriticPath::General: SSN_TRY(ssn::critic_norm_forward(n, x, cond, batch, out, ws, st)); break;
    }
    return 0;
}
// (eps, xp_out: the plain chain builds the penalty points and its three input blocks in ONE launch -- critic_step_impl; nullptr
// on every other path)
int critic_net_loss_grad(const CriticSpec& n, const float* xg, const float* cg, const float* xd, const float* cd, const float* xp,
                         const float* cp, int ng, int nd, int np, float lmd, float* grads, float* stats, float* dvals, float* ws,
                         hipStream_t st, const float* eps, float* xp_out) {
    switch (critic_path(n, (long)ng + nd + np, cg && cd && cp)) {
    case CriticPath::Fused:
        SSN_TRY(ssn::critic_fused_loss_grad(n, xg, cg, xd, cd, xp, cp, ng, nd, np, lmd, grads, stats, dvals, ws, st));
        break;
    case CriticPath::Plain:
        SSN_TRY(ssn::critic_loss_grad(n, xg, cg, xd, cd, xp, cp, ng, nd, np, lmd, grads, stats, dvals, ws, st, eps, xp_out));
        break;
    case CriticPath::General:
        SSN_TRY(ssn::critic_norm_loss_grad(n, xg, cg, xd, cd, xp, cp, ng, nd, np, lmd, grads, stats, dvals, ws, st));
        break;
    }
    return 0;
}
int critic_net_input_grad(const CriticSpec& n, const float* x, const float* cond, int batch, float scale, float* gx, float* stats,
                          float* ws, hipStream_t st) {
    switch (critic_path(n, batch, cond != nullptr)) {
    case CriticPath::Fused: SSN_TRY(ssn::critic_fused_input_grad(n, x, cond, batch, scale, gx, stats, ws, st)); break;
    case CriticPath::Plain: SSN_TRY(ssn::critic_input_grad(n, x, cond, batch, scale, gx, stats, ws, st)); break;
    case CriticPath::General: SSN_TRY(ssn::critic_norm_input_grad(n, x, cond, batch, scale, gx, stats, ws, st)); break;
    }
    return 0;
}
// dvals[0:ng] = D(xg), dvals[ng:ng+nd] = D(xd): what the accuracy mean D(xg) - mean D(xd) is reduced from.
int critic_net_accuracy_forwards(const CriticSpec& n, const float* xg, const float* cg, const float* xd, const float* cd, int ng,
                                 int nd, float* dvals, float* ws, hipStream_t st, bool inputs_ready) {
    const bool conds = cg && cd;
    // a critic of fused size keeps one forward per input, on whichever path it takes (every leaky one included: those run
    // the plain chain twice)
    const bool fused_size = conds && (fused_ok(n.dims, n.nlayers, ng) || fused_ok(n.dims, n.nlayers, nd));
    if (!fused_size && critic_path(n, ng, conds) == CriticPath::Plain) {
        // ONE pass of the plain chain over the stacked rows [xg; xd] (the values of two separate forwards, bit for bit).
        // inputs_ready: the workspace already starts with the input block of those rows (ssn_host.h)
        SSN_TRY(ssn::critic_forward2(n, xg, cg, ng, xd, cd, nd, dvals, ws, st, inputs_ready));
        return 0;
    }
    int rc = ng > 0 ? critic_net_forward(n, xg, cg, ng, dvals, ws, st) : 0;
    if (!rc && nd > 0) rc = critic_net_forward(n, xd, cd, nd, dvals + ng, ws, st);
    return rc;
}
// mean D(xg) - mean D(xd) in one call (the critic's values of both inputs into `dvals`, one reduction in a fixed order)
int critic_accuracy(const CriticSpec& s, const float* xg, const float* cg, const float* xd, const float* cd, int ng, int nd,
                    float* acc, float* dvals, float* workspace, void* stream) {
    if (int rc = critic_net_accuracy_forwards(s, xg, cg, xd, cd, ng, nd, dvals, workspace, (hipStream_t)stream, false)) return rc;
    SSN_TRY(ssn::launch_mean_diff(dvals, ng, nd, acc, (hipStream_t)stream));
    return 0;
}

// One helper per family of entry points (include/ssnode_mi355x.h): the family's arguments as a CriticSpec, or a refusal under
// the name `fn` of the entry point that was called.  What every family refuses is what ssn::critic_layout refuses.
int checked_spec(const char* fn, const CriticSpec& s) {
    ssn::CriticLayout lay;
    return ssn::critic_layout(s, lay) ? 0 : refuse(fn, "invalid layer flags / activation / slope, or more than 8 layers");
}
// -- norm: rectify, per-layer normalisation flags 0 / 1 -- and, for the accuracy and the one-call step, a slope next to plain
//    layers (a slope next to a normalisation is a critic in its general form: the _act entry points)
int norm_spec(const char* fn, const float* params, const int* dims, const int* layer_norm, int nlayers, float leak, int hide_cell_type,
              int precision, CriticSpec& s) {
    bool norm = false;
    for (int l = 0; layer_norm && l < nlayers; ++l) {
        if (layer_norm[l] != 0 && layer_norm[l] != 1)
            return refuse(fn, "layer_norm flags are 0 / 1 (scaled layers: the _act entry points)");
        norm = norm || layer_norm[l] != 0;
    }
    if (leak != 0.f && norm) return refuse(fn, "leak with layer-normalised layers (that critic: the _act entry points)");
    s = CriticSpec{params, dims, layer_norm, nlayers, 0, leak, hide_cell_type, precision == 0};
    return checked_spec(fn, s);
}
// -- leaky: plain layers, a hidden nonlinearity x > 0 ? x : leak * x (lasagne's leaky_rectify = 0.01, very_leaky_rectify = 1/3,
//    linear = 1)
int leaky_spec(const char* fn, const float* params, const int* dims, int nlayers, float leak, int hide_cell_type, int precision,
               CriticSpec& s) {
    return norm_spec(fn, params, dims, nullptr, nlayers, leak, hide_cell_type, precision, s);
}
// -- plain: rectify, plain layers
int plain_spec(const char* fn, const float* params, const int* dims, int nlayers, int hide_cell_type, int precision, CriticSpec& s) {
    return leaky_spec(fn, params, dims, nlayers, 0.f, hide_cell_type, precision, s);
}
// -- act: any critic -- activation code, per-layer flags 0 / 1 / 3
int act_spec(const char* fn, const float* params, const int* dims, const int* layer_flags, int nlayers, int act, int hide_cell_type,
             int precision, CriticSpec& s) {
    ssn::ActSpec a{};
    if (!ssn::act_from_code(act, a)) return refuse(fn, "invalid layer flags / activation");
    s = CriticSpec{params, dims, layer_flags, nlayers, act, a.leak, hide_cell_type, precision == 0};
    return checked_spec(fn, s);
}
long critic_num_params(const int* dims, const int* layer_flags, int nlayers) {
    ssn::CriticLayout lay;
    return dims && ssn::critic_layout(CriticSpec{nullptr, dims, layer_flags, nlayers, 0, 0.f, 0, false}, lay) ? lay.nparams : -1;
}
size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

// One critic update in one call: penalty points, loss pass, optimizer step (dropped on the device when *gate > gate_bound;
// gate null: always taken), accuracy, and the sums of squares and the head of the record in one finishing launch.
int critic_step_impl(const ssn_critic_step* a, const double* gate, double gate_bound, void* stream) {
    if (!a || !a->params || !a->dims || !a->xg || !a->xd || !a->eps || !a->xp || !a->grads || !a->stats || !a->dvals ||
        !a->workspace || !a->opt || !a->acc_dvals || !a->tail || a->n <= 0 || a->nseg < 0)
        return refuse("ssn_critic_step_run", kInvalid);
    CriticSpec net;
    if (int rc = norm_spec("ssn_critic_step_run", a->params, a->dims, a->layer_norm, a->nlayers, a->leak, a->hide_cell_type,
                           a->precision, net)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const int n = a->n, nx = a->dims[0] - (a->cond ? 3 : 0);        // cond NULL: the unconditional critic (dims[0] = nx)
    int rc;
    // the plain chain with the one condition array of the loop: the penalty points and the three input blocks come from ONE
    // launch inside the loss pass (the bits of ssn_interpolate_f32 + the input kernels).  Not for a critic of fused size, a
    // leaky one included.
    const bool one_launch_inputs = critic_path(net, 3L * n, a->cond != nullptr) == CriticPath::Plain && a->cond &&
                                   !fused_ok(a->dims, a->nlayers, 3L * n);
    if (!one_launch_inputs && (rc = ssn_interpolate_f32(a->eps, a->xd, a->xg, a->xp, n, nx, stream))) return rc;
    if ((rc = critic_net_loss_grad(net, a->xg, a->cond, a->xd, a->cond, a->xp, a->cond, n, n, n, a->lmd, a->grads, a->stats, a->dvals,
                                   a->workspace, st, one_launch_inputs ? a->eps : nullptr, one_launch_inputs ? a->xp : nullptr))) return rc;
    const long nparams = ssn_critic_num_params(a->dims, a->nlayers);
    if ((rc = optimizer_step_full(a->params, a->grads, a->opt_s1, a->opt_s2, nparams, a->opt, gate, gate_bound, nullptr, nullptr,
                                  nullptr, nullptr, stream))) return rc;
    // (the loss pass of the one-launch-inputs form left the input block of [xg; xd] at the head of the workspace, where the
    // stacked forward of the accuracy builds it: same rows, same conditions -- not built again)
    if ((rc = critic_net_accuracy_forwards(net, a->xg, a->cond, a->xd, a->cond, n, n, a->acc_dvals, a->workspace, st, one_launch_inputs)))
        return rc;
    if (a->nseg > 0 && (!a->seg_bounds || !a->seg_ws)) return refuse("ssn_critic_step_run", kInvalid);
    // accuracy, sums of squares and the head of the record: the chunk sums, then ONE finishing launch (same bits as
    // ssn_critic_accuracy + ssn_segment_sqnorms2_f32 + the head kernel)
    SSN_TRY(ssn::launch_step_finish(a->params, a->seg_bounds, a->nseg, a->seg_ws, a->acc_dvals, n, n, a->pens64, a->stats, a->tail, st));
    return 0;
}

// ---- feed-forward model ---------------------------------------------------------------------------------------------------------
bool ff_params_ok(const ssn_ff_params* p) {
    return p && p->nsam >= 0 && p->nhid >= 1 && p->ni >= 1 && p->ni <= 32 && p->box >= 1;
}
ssn::FFArgs ff_args(const ssn_ff_params& p) {
    ssn::FFArgs a{};
    a.nsam = p.nsam; a.nhid = p.nhid; a.ni = p.ni; a.box = p.box;
    a.RF_l = (float)p.RF_l; a.RF_d = (float)p.RF_d; a.TH = (float)p.TH; a.TH_d = (float)p.TH_d;
    a.J = (float)p.J; a.a = (float)p.a;
    return a;
}
// Is the stimulus set a 3 x 3 x 3 product lattice in the model script's order?  (27 x 3 floats: read back once per call.)
bool ff_lattice(const float* stim, int ni, ssn::FFLattice& lat, void* stream) {
    if (ni != 27) return false;
    float hs[27][3];
    if (hipMemcpyAsync(hs, stim, sizeof(hs), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return false;
    for (int k = 0; k < 3; ++k) { lat.x[k] = hs[9 * k][0]; lat.y[k] = hs[3 * k][1]; lat.z[k] = hs[k][2]; }
    bool lattice = true;
    for (int i = 0; i < 27 && lattice; ++i)
        lattice = hs[i][0] == lat.x[i / 9] && hs[i][1] == lat.y[(i / 3) % 3] && hs[i][2] == lat.z[i % 3];
    return lattice;
}
// The dense kernels read RF_w, FF_con, FF_str with 16-byte loads whenever box^3 % 4 == 0 (a sample's and a unit's rows then
// start at multiples of 16 bytes from the base): the bases must be 16-byte aligned.  Decided on the host, before any launch;
// the backward has the same contract as the forward whose tensors it takes.  0 or the refusal of the dense entry `fn`.
int ff_dense_alignment(const char* fn, const ssn_ff_params& p, const float* RF_w, const float* FF_con, const float* FF_str) {
    if (((long long)p.box * p.box * p.box) % 4 != 0) return 0;
    if ((((uintptr_t)RF_w | (uintptr_t)FF_con | (uintptr_t)FF_str) % 16) == 0) return 0;
    return refuse(fn, "RF_w, FF_con, FF_str must be 16-byte aligned when box^3 % 4 == 0");
}

// ---- steady-state gradient ------------------------------------------------------------------------------------------------------
template <typename T>
int build_dw_impl(const T* z, const T* J, const T* D, const T* S, int which, T* dW, int B, int N, void* stream) {
    if (B < 0 || N < 1 || which < 0 || which > 2 || (B > 0 && (!dW || (which > 0 && !z) || !J || !D || !S)))
        return refuse("ssn_build_dw", kInvalid);
    T jds[12];
    pack_jds(J, D, S, jds);
    SSN_TRY(ssn::launch_build_dw<T>(z, jds, which, dW, B, N, (hipStream_t)stream));
    return 0;
}
template <typename T>
int ss_system_impl(const T* R, const T* W, const T* dW, int dw_per_draw, const T* I, int i_per_draw, int nz,
                   int nb, int M, const ssn_solver_params* p, T* A, T* rhs, void* stream) {
    if (nz == 0 || nb == 0) return 0;
    if (!p || !R || !W || !dW || !I || !A || !rhs || nz < 0 || nb < 0 || M <= 0 || (M & 1) || p->io_type < 0 ||
        p->io_type > 2)
        return refuse("ssn_ss_grad_system", kInvalid);
    SSN_TRY(ssn::launch_ss_system<T>(R, W, dW, dw_per_draw, I, i_per_draw, ssn::make_io_consts<T>(*p), nz, nb, M, A, rhs,
                                     (hipStream_t)stream));
    return 0;
}
template <typename T>
int lu_solve_impl(T* A, T* rhs, int* info, int nsys, int M, int nrhs, void* stream) {
    if (nsys < 0 || M < 0 || (nsys > 0 && M > 0 && (!A || !rhs))) return refuse("ssn_lu_solve", kInvalid);
    SSN_TRY(ssn::launch_lu_solve<T>(A, rhs, info, nsys, M, nrhs, (hipStream_t)stream));
    return 0;
}

// ---- ensembles ------------------------------------------------------------------------------------------------------------------
// what both gradient entries hand to the launcher; l0: null (L0 from the moments in the record), or L0 per member with D == 0
int ens_gen_grads_launch(const ssn_ens_grads* a, const double* l0, void* stream) {
    ssn::EnsGradsArgs g{};
    g.K = a->K; g.B = a->B; g.nv = a->nv; g.NB = a->NB; g.M = a->M; g.D = a->D;
    g.part = a->part; g.g_ext = a->g_ext; g.ext_base = a->ext_base; g.zin = a->zin; g.dyn_row = a->dyn_row; g.rate_row = a->rate_row;
    g.scale_dyn = a->scale_dyn; g.scale_rate = a->scale_rate;
    g.data_moments = a->data_moments; g.weights = a->weights; g.costs = a->costs; g.grads = a->grads; g.rec = a->rec;
    g.rstride = a->rstride; g.l0 = l0;
    SSN_TRY(ssn::launch_ens_gen_grads(g, (hipStream_t)stream));
    return 0;
}

// ---- scorer and sliced Wasserstein ----------------------------------------------------------------------------------------------
const char* const kTooManyDirections = "more than 4096 directions";
// the two KS entries: `wnum` is the W1 entry's (required there), null for the plain one
int ks_columns(const char* fn, bool w1, const float* x, const float* truth_sorted, const int* m, int S, int B, int C, int T,
               int* n, long long* num, double* wnum, void* stream) {
    if (B > SSN_KS_MAX_DRAWS) return refuse(fn, "more than 16384 values per column (the sort runs in 64 KiB of LDS)");
    if (S < 0 || B < 1 || C < 0 || T < 0 ||
        ((long)S * C > 0 && (!x || !m || !n || !num || (w1 && !wnum) || (T > 0 && !truth_sorted))))
        return refuse(fn, kInvalid);
    if (w1) SSN_TRY(ssn::launch_ks_w1_columns(x, truth_sorted, m, S, B, C, T, n, num, wnum, (hipStream_t)stream));
    else    SSN_TRY(ssn::launch_ks_columns(x, truth_sorted, m, S, B, C, T, n, num, (hipStream_t)stream));
    return 0;
}
static_assert(SSN_ENS_SWD_MAX_MEMBERS == ssn::SWD_ENS_MAX_MEMBERS && SSN_SWD_WAVE_MAX_BATCH == ssn::SWD_WAVE_MAX_BATCH &&
              SSN_SWD_FORM_AUTO == ssn::SWD_FORM_AUTO && SSN_SWD_FORM_GENERAL == ssn::SWD_FORM_GENERAL &&
              SSN_SWD_FORM_WAVE == ssn::SWD_FORM_WAVE, "the header's macros are the library's constants");
// the limits the three ssn_ens_swd_* entries share; 0 when none is passed
int ens_swd_limits(const char* name, int K, int B, int L) {
    const char* what = K > SSN_ENS_SWD_MAX_MEMBERS ? "more than 2048 members"
                       : B > SSN_SWD_MAX_BATCH ? "more than 4096 rows per member (keys and values are sorted in 48 KiB of LDS)"
                       : L > SSN_W1_MAX_DIRECTIONS ? kTooManyDirections : nullptr;
    return what ? refuse(name, what) : 0;
}
// one round of the device rejection sampler (ssn_fp_select_f64 / _f32)
template <typename T>
int fp_select_impl(const char* name, const int* codes, const T* x, int A, int R, int NB, int M, const int* probes, int nprobe,
                   const int* set_of, int cand0, int NZ, int* verdict, T* out, int* accepted, int* used, int* rejections,
                   int* draw_index, void* stream) {
    if (R > ssn::fp_select_max_candidates())
        return refuse(name, "more than " + std::to_string(ssn::fp_select_max_candidates()) +
                                " candidates in one round (the accepted indices of a round are kept in LDS)");
    if (A < 0 || R < 0 || NB < 1 || M <= 0 || (M & 1) || nprobe < 0 || NZ < 1 || cand0 < 0 || (long)NB * M >= (1L << 31) ||
        (long)NZ * NB * nprobe >= (1L << 31) || (long)cand0 + R >= (1L << 31) ||
        ((long)A * R > 0 && (!codes || !x || !set_of || !verdict || !out || !accepted || !used || !rejections || !draw_index ||
                             (nprobe > 0 && !probes))))
        return refuse(name, kInvalid);
    if ((long)A * R == 0) return 0;                           // empty batch
    ssn::FpSelectArgs<T> a;
    a.codes = codes; a.x = x; a.A = A; a.R = R; a.NB = NB; a.M = M; a.probes = probes; a.nprobe = nprobe; a.set_of = set_of;
    a.cand0 = cand0; a.NZ = NZ; a.verdict = verdict; a.out = out; a.accepted = accepted; a.used = used; a.rejections = rejections;
    a.draw_index = draw_index;
    SSN_TRY(ssn::launch_fp_select<T>(a, (hipStream_t)stream));
    return 0;
}

// ---- MT19937 / Philox -----------------------------------------------------------------------------------------------------------
// the device MT19937 draw (ssn_mt19937.hip): one body per _f32 / _f64 pair, and the tail of a call
template <typename T>
int mt_sample(unsigned int* key, int* pos, unsigned long long total, unsigned long long skip, unsigned long long count, T* out,
              void* stream) {
    if (!key || !pos) return refuse("ssn_mt19937_random_sample", "null state");
    SSN_TRY(ssn::mt19937_draw(key, pos, total, skip, count, out, (int)sizeof(T), (hipStream_t)stream));
    return 0;
}
// what every *_begin entry does once its arguments are checked: no ticket yet, then the draw (W, jds12, N: the W builder's; tail)
int mt_begin(const unsigned int* key, int pos, unsigned long long total, unsigned long long skip, unsigned long long count, void* out,
             int elem, void* stream, int* ticket, float* W = nullptr, const float* jds12 = nullptr, int N = 0,
             const ssn::MtTail* tail = nullptr) {
    *ticket = -1;
    SSN_TRY(ssn::mt19937_begin(key, pos, total, skip, count, out, elem, (hipStream_t)stream, ticket, W, jds12, N, tail));
    return 0;
}
template <typename T>
int mt_sample_begin(const unsigned int* key, int pos, unsigned long long total, unsigned long long skip, unsigned long long count,
                    T* out, void* stream, int* ticket) {
    if (!key || !ticket) return refuse("ssn_mt19937_random_sample_begin", "null state / ticket");
    return mt_begin(key, pos, total, skip, count, out, (int)sizeof(T), stream, ticket);
}
ssn::MtTail mt_tail(int kind, unsigned long long total, unsigned long long skip, unsigned long long count, float* out) {
    ssn::MtTail tail;
    tail.kind = kind; tail.total = total; tail.skip = skip; tail.count = count; tail.out = out;
    return tail;
}
template <typename T>
int philox_amp_impl(unsigned long long seed, unsigned long long offset, const T* v, T* zin, T* amp, unsigned long long n, int M,
                    int bernoulli, void* stream) {
    if (n > 0 && (!v || !zin || !amp || M <= 0)) return refuse("ssn_philox_amp", kInvalid);
    SSN_TRY(ssn::launch_philox_amp<T>(seed, offset, v, zin, amp, n, M, bernoulli, (hipStream_t)stream));
    return 0;
}
template <typename T>
int philox_uniform_impl(unsigned long long seed, unsigned long long offset, T* out, unsigned long long n, void* stream) {
    if (n > 0 && !out) return refuse("ssn_philox_uniform", "null output");
    SSN_TRY(ssn::launch_philox_uniform<T>(seed, offset, out, n, (hipStream_t)stream));
    return 0;
}

}  // namespace

extern "C" {

// ---- errors / version / device --------------------------------------------------------------------------------------------------
int ssn_abi_version(void) { return 1; }
const char* ssn_last_error(void) { return g_last_error.c_str(); }
int ssn_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { fail(e, "hipGetDeviceCount"); return -(int)e; }
    return n;
}

// ---- solver: device buffers, host buffers, drop-in ------------------------------------------------------------------------------
int ssn_solver_fast_path(int M, int NB, int dtype_bytes) {
    if (M <= 0 || (M & 1)) return 0;
    const bool tile = dtype_bytes == 8 ? ssn::tile_supported<double>(M, NB) : ssn::tile_supported<float>(M, NB);
    const bool regw = dtype_bytes == 8 ? ssn::regw_supported<double>(M, NB) : ssn::regw_supported<float>(M, NB);
    return tile ? 2 : (regw ? 1 : 0);
}
int ssn_set_operand_precision(int mode) { return operand_precision_state().exchange(mode ? 1 : 0); }
int ssn_get_operand_precision(void) { return operand_precision_state().load(); }
int ssn_solve_batch_variant_for(int B, int NB, int M, int dtype_bytes, const ssn_solver_params* p) {
    if (B <= 0 || NB <= 0) return -1;
    const int v = dtype_bytes == 8
        ? solve_batch_impl<double>(-1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, B, NB, M, p, nullptr, true)
        : solve_batch_impl<float>(-1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, B, NB, M, p, nullptr, true);
    return v >= SSN_ERR_BASE ? -1 : v;
}
int ssn_solve_batch_f32(const float* W, const float* ext, int ext_per_draw, float* r, float* r_prev, int* codes,
                        int* steps, int B, int NB, int M, const ssn_solver_params* p, void* stream) {
    return solve_batch_impl<float>(-1, W, ext, ext_per_draw, r, r_prev, codes, steps, B, NB, M, p, stream);
}
int ssn_solve_batch_f64(const double* W, const double* ext, int ext_per_draw, double* r, double* r_prev,
                        int* codes, int* steps, int B, int NB, int M, const ssn_solver_params* p, void* stream) {
    return solve_batch_impl<double>(-1, W, ext, ext_per_draw, r, r_prev, codes, steps, B, NB, M, p, stream);
}
int ssn_solve_batch_f32_variant(int variant, const float* W, const float* ext, int ext_per_draw, float* r,
                                float* r_prev, int* codes, int* steps, int B, int NB, int M,
                                const ssn_solver_params* p, void* stream) {
    return solve_batch_impl<float>(variant, W, ext, ext_per_draw, r, r_prev, codes, steps, B, NB, M, p, stream);
}
int ssn_solve_batch_f64_variant(int variant, const double* W, const double* ext, int ext_per_draw, double* r,
                                double* r_prev, int* codes, int* steps, int B, int NB, int M,
                                const ssn_solver_params* p, void* stream) {
    return solve_batch_impl<double>(variant, W, ext, ext_per_draw, r, r_prev, codes, steps, B, NB, M, p, stream);
}
int ssn_solve_batch_host_f32(const float* W, const float* ext, int ext_per_draw, float* r, float* r_prev,
                             int* codes, int* steps, int B, int NB, int M, const ssn_solver_params* p) {
    return solve_batch_host_impl<float>(W, ext, ext_per_draw, r, r_prev, codes, steps, B, NB, M, p);
}
int ssn_solve_batch_host_f64(const double* W, const double* ext, int ext_per_draw, double* r, double* r_prev,
                             int* codes, int* steps, int B, int NB, int M, const ssn_solver_params* p) {
    return solve_batch_host_impl<double>(W, ext, ext_per_draw, r, r_prev, codes, steps, B, NB, M, p);
}
// drop-in symbols (tc_gan/ext/ssnode.c exports)
int solve_dynamics_asym_power_euler(int N, double* W, double* ext, double k, double n, double* r0, double* r1,
                                    double tau_E, double tau_I, double dt, int max_iter, double atol,
                                    double rate_soft_bound, double rate_hard_bound) {
    return legacy_solve(SSN_IO_POWER, N, W, ext, k, n, r0, r1, tau_E, tau_I, dt, max_iter, atol, rate_soft_bound, rate_hard_bound);
}
int solve_dynamics_asym_linear_euler(int N, double* W, double* ext, double k, double n, double* r0, double* r1,
                                     double tau_E, double tau_I, double dt, int max_iter, double atol,
                                     double rate_soft_bound, double rate_hard_bound) {
    return legacy_solve(SSN_IO_LINEAR, N, W, ext, k, n, r0, r1, tau_E, tau_I, dt, max_iter, atol, rate_soft_bound, rate_hard_bound);
}
int solve_dynamics_asym_tanh_euler(int N, double* W, double* ext, double k, double n, double* r0, double* r1,
                                   double tau_E, double tau_I, double dt, int max_iter, double atol,
                                   double rate_soft_bound, double rate_hard_bound) {
    return legacy_solve(SSN_IO_TANH, N, W, ext, k, n, r0, r1, tau_E, tau_I, dt, max_iter, atol, rate_soft_bound, rate_hard_bound);
}
double io_pow(double v, double r0, double r1, double v0, double k, double n) { return legacy_io(SSN_IO_POWER, v, r0, r1, v0, k, n); }
double io_alin(double v, double r0, double r1, double v0, double k, double n) { return legacy_io(SSN_IO_LINEAR, v, r0, r1, v0, k, n); }
double io_atanh(double v, double r0, double r1, double v0, double k, double n) { return legacy_io(SSN_IO_TANH, v, r0, r1, v0, k, n); }
double rate_to_volt(double rate, double k, double n) {
    // (rate/k)^(1/n) == the v at which io_pow(v) = rate: evaluate on the device through the same
    // pow routine the kernels use:  k' * x^n' with k' = 1, x = rate/k, n' = 1/n.
    ssn_solver_params p;
    std::memset(&p, 0, sizeof(p));
    p.io_type = SSN_IO_POWER; p.k = 1.0; p.n = 1.0 / n; p.rate_soft_bound = 1.0; p.rate_hard_bound = 2.0;
    const double x = rate / k;
    double out = std::numeric_limits<double>::quiet_NaN();
    const ssn::IoConsts<double> c = ssn::make_io_consts<double>(p);
    scalar_roundtrip(&x, 1, &out, 1, [&](double* dv, double* dout, hipStream_t st) {
        return ssn::launch_io_eval<double>(dv, dout, 1, c, st);
    });
    return out;
}
double dot(int dim, const double* x, const double* y) {
    if (dim <= 0) return 0.0;
    double out = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> xy(2 * (size_t)dim);
    std::memcpy(xy.data(), x, dim * sizeof(double));
    std::memcpy(xy.data() + dim, y, dim * sizeof(double));
    scalar_roundtrip(xy.data(), xy.size(), &out, 1, [&](double* d, double* dout, hipStream_t st) {
        return ssn::launch_dot<double>(d, d + dim, dout, dim, st);
    });
    return out;
}

// ---- weights and stimuli ------------------------------------------------------------------------------------------------------
int ssn_build_w_f32(const float* z, const float* J, const float* D, const float* S, float* W, int B, int N, void* stream) {
    return build_w_impl<float>(z, J, D, S, W, B, N, stream);
}
int ssn_build_w_f64(const double* z, const double* J, const double* D, const double* S, double* W, int B, int N, void* stream) {
    return build_w_impl<double>(z, J, D, S, W, B, N, stream);
}
int ssn_build_w_devparams_f32(const float* z, const float* jds_dev, float* W, int B, int N, void* stream) {
    if (!jds_dev || (B > 0 && (!z || !W)) || N < 1 || B < 0) return refuse("ssn_build_w_devparams_f32", kInvalid);
    SSN_TRY(ssn::launch_build_w<float>(z, nullptr, W, B, N, (hipStream_t)stream, jds_dev));
    return 0;
}
int ssn_build_w_philox_f32(unsigned long long seed, unsigned long long offset, const float* J, const float* D, const float* S,
                           float* W, float* z, int B, int N, void* stream) {
    return build_w_philox_impl<float>(seed, offset, J, D, S, W, z, B, N, stream);
}
int ssn_build_w_philox_f64(unsigned long long seed, unsigned long long offset, const double* J, const double* D, const double* S,
                           double* W, double* z, int B, int N, void* stream) {
    return build_w_philox_impl<double>(seed, offset, J, D, S, W, z, B, N, stream);
}
int ssn_build_w_table_f32(const float* z, const float* jds_table, float* W, int S, int B, int N, void* stream) {
    return build_w_table_impl<float>("ssn_build_w_table_f32", z, jds_table, W, S, B, N, stream);
}
int ssn_build_w_table_f64(const double* z, const double* jds_table, double* W, int S, int B, int N, void* stream) {
    return build_w_table_impl<double>("ssn_build_w_table_f64", z, jds_table, W, S, B, N, stream);
}
int ssn_stimulus_f32(const float* bw, const float* con, float smoothness, float* ext, int B, int NB, int N, void* stream) {
    return stimulus_impl<float>(bw, con, smoothness, nullptr, ext, B, NB, N, stream);
}
int ssn_stimulus_f64(const double* bw, const double* con, double smoothness, double* ext, int B, int NB, int N, void* stream) {
    return stimulus_impl<double>(bw, con, smoothness, nullptr, ext, B, NB, N, stream);
}
int ssn_stimulus_amp_f32(const float* bw, const float* con, float smoothness, const float* amp, float* ext, int B, int NB,
                         int N, void* stream) {
    return stimulus_impl<float>(bw, con, smoothness, amp, ext, B, NB, N, stream);
}
int ssn_stimulus_amp_f64(const double* bw, const double* con, double smoothness, const double* amp, double* ext, int B,
                         int NB, int N, void* stream) {
    return stimulus_impl<double>(bw, con, smoothness, amp, ext, B, NB, N, stream);
}
int ssn_stimulus_hetero_f32(const float* bw, const float* con, float smoothness, const float* zin, const float* v, int nv, float* ext,
                            int B, int NB, int N, void* stream) {
    if (!zin || !v || (nv != 1 && nv != 2 && nv != 2 * N) || B < 0 || NB < 0 || N < 1)
        return refuse("ssn_stimulus_hetero", kInvalid);
    SSN_TRY(ssn::launch_stimulus_hetero(bw, con, smoothness, zin, v, nv, ext, B, NB, N, (hipStream_t)stream));
    return 0;
}
int ssn_gen_inputs_philox_f32(const ssn_gen_inputs* a, void* stream) {
    if (!a || !a->J || !a->D || !a->S || !a->bw || !a->con || !a->W || !a->ext || a->B < 0 || a->NB < 0 || a->N <= 0 ||
        (a->v && (!a->zin || !a->amp)))
        return refuse("ssn_gen_inputs_philox", kInvalid);
    // one launch (ssn_aux.hip: gen_inputs_kernel): the numbers of ssn_philox_amp_f32, ssn_stimulus_amp_f32 and
    // ssn_build_w_philox_f32 called in that order
    ssn::GenInputsArgs g{};
    g.seed = a->seed; g.off_z = a->off_z; g.off_zin = a->off_zin;
    g.bw = a->bw; g.con = a->con; g.v = a->v; g.inv_l = 1.f / a->smoothness; g.bernoulli = a->bernoulli;
    g.W = a->W; g.z = a->z; g.zin = a->zin; g.amp = a->amp; g.ext = a->ext;
    g.B = a->B; g.NB = a->NB; g.N = a->N;
    float jds12[12];
    pack_jds(a->J, a->D, a->S, jds12);
    SSN_TRY(ssn::launch_gen_inputs(g, jds12, (hipStream_t)stream));
    return 0;
}
int ssn_io_eval_f32(const float* v, float* out, long count, const ssn_solver_params* p, void* stream) {
    return io_eval_impl<float>(v, out, count, p, stream);
}
int ssn_io_eval_f64(const double* v, double* out, long count, const ssn_solver_params* p, void* stream) {
    return io_eval_impl<double>(v, out, count, p, stream);
}

// ---- generator ------------------------------------------------------------------------------------------------------------------
int ssn_gen_supported(int M, int dtype_bytes) {
    if (M <= 0 || (M & 1)) return 0;
    return dtype_bytes == 8 ? ssn::gen_supported<double>(M) : ssn::gen_supported<float>(M);
}
int ssn_gen_forward_variant(int B, int NB, int M, int seqlen, int save, const ssn_gen_params* g) {
    if (!g || B <= 0 || NB <= 0) return -1;
    ssn_gen_params p = *g;
    p.seqlen = seqlen;
    ssn::GenFwdArgs<float> a{};
    const int v = gen_forward_path(a, B, NB, M, save != 0, &p);
    return v >= SSN_ERR_BASE ? -1 : v;
}
int ssn_gen_forward_f32(const float* W, const float* ext, float* time_avg, float* dyn_row, float* rate_row, float* traj,
                        float* df, int B, int NB, int M, const ssn_gen_params* p, void* stream) {
    return gen_forward_impl<float>(W, ext, time_avg, dyn_row, rate_row, traj, df, B, NB, M, p, stream);
}
int ssn_gen_forward_f64(const double* W, const double* ext, double* time_avg, double* dyn_row, double* rate_row,
                        double* traj, double* df, int B, int NB, int M, const ssn_gen_params* p, void* stream) {
    return gen_forward_impl<double>(W, ext, time_avg, dyn_row, rate_row, traj, df, B, NB, M, p, stream);
}
int ssn_gen_backward_f32(const float* W, const float* traj, float* df_delta, const float* g_time_avg, double c_dyn,
                         double c_rate, int B, int NB, int M, const ssn_gen_params* p, void* stream) {
    return gen_backward_impl<float>(W, traj, df_delta, g_time_avg, nullptr, c_dyn, c_rate, B, NB, M, p, stream);
}
int ssn_gen_backward_f64(const double* W, const double* traj, double* df_delta, const double* g_time_avg, double c_dyn,
                         double c_rate, int B, int NB, int M, const ssn_gen_params* p, void* stream) {
    return gen_backward_impl<double>(W, traj, df_delta, g_time_avg, nullptr, c_dyn, c_rate, B, NB, M, p, stream);
}
int ssn_gen_backward_ext_f32(const float* W, const float* traj, float* df_delta, const float* g_time_avg, float* g_ext,
                             double c_dyn, double c_rate, int B, int NB, int M, const ssn_gen_params* p, void* stream) {
    return gen_backward_impl<float>(W, traj, df_delta, g_time_avg, g_ext, c_dyn, c_rate, B, NB, M, p, stream);
}
int ssn_gen_backward_ext_f64(const double* W, const double* traj, double* df_delta, const double* g_time_avg,
                             double* g_ext, double c_dyn, double c_rate, int B, int NB, int M, const ssn_gen_params* p,
                             void* stream) {
    return gen_backward_impl<double>(W, traj, df_delta, g_time_avg, g_ext, c_dyn, c_rate, B, NB, M, p, stream);
}
int ssn_gen_backward_max_f32(const float* W, const float* traj, float* df_delta, const float* g_time_avg, float* g_ext,
                             float* dmax, int* tracked, double c_dyn, double c_rate, int B, int NB, int M,
                             const ssn_gen_params* p, void* stream) {
    return gen_backward_impl<float>(W, traj, df_delta, g_time_avg, g_ext, c_dyn, c_rate, B, NB, M, p, stream, dmax, tracked);
}
int ssn_gen_backward_fused_supported(int B, int NB, int M, const ssn_gen_params* p, float xmax) {
    if (!p) return 0;
    ssn::GenBwdArgs<float> a{};
    gen_fill<float>(a, B, NB, M, *p);
    return p->skip_steps >= 0 && p->skip_steps < p->seqlen && (long)NB * p->seqlen * M < (1L << 29) &&
           ssn::gen_backward_fused_supported(a, xmax);
}
int ssn_gen_backward_fused_f32(const float* W, const float* traj, const float* df, const float* g_time_avg, float* g_ext,
                               float* gW, float* dmax, float xmax, double c_dyn, double c_rate, int B, int NB, int M,
                               const ssn_gen_params* p, void* stream) {
    if (B == 0 || NB == 0) return 0;
    if (!p || !W || !traj || !df || !g_time_avg || !gW || !ssn_gen_backward_fused_supported(B, NB, M, p, xmax))
        return refuse("ssn_gen_backward_fused", "invalid argument or unsupported size (fp32, NB <= 8, even 2N <= 208, "
                                                "NB T 2N < 2^29, 0 < xmax < inf)");
    ssn::GenBwdArgs<float> a;
    a.W = W; a.traj = traj; a.delta = const_cast<float*>(df); a.g_time_avg = g_time_avg; a.g_ext = g_ext;
    a.c_dyn = (float)c_dyn; a.c_rate = (float)c_rate;
    gen_fill<float>(a, B, NB, M, *p);
    if (dmax) {
        SSN_TRY(hipMemsetAsync(dmax, 0, sizeof(float) * (size_t)B, (hipStream_t)stream));
        a.dmax = reinterpret_cast<unsigned*>(dmax);
    }
    SSN_TRY(ssn::launch_gen_backward_fused(a, gW, xmax, (hipStream_t)stream));
    return 0;
}
long ssn_gen_grads_ws_doubles(void) { return 2 * 128 + 1; }
int ssn_gen_grads_f32(const ssn_gen_grads* a, void* stream) {
    if (!a || !a->jds_part || a->B < 0 || a->nv < 0 || a->nv > 2 || !a->dmean || !a->ws || !a->out ||
        (a->nv > 0 && (!a->g_ext || !a->ext_base || !a->zin || a->NB <= 0 || a->M <= 0 || (a->M & 1))))
        return refuse("ssn_gen_grads", kInvalid);
    ssn::GenGradsArgs g{};
    g.part = a->jds_part; g.B = a->B; g.nv = a->nv; g.g_ext = a->g_ext; g.ext_base = a->ext_base; g.zin = a->zin;
    g.NB = a->NB; g.M = a->M; g.dmean = a->dmean; g.pens = a->pens64; g.dynamics_cost = a->dynamics_cost; g.rate_cost = a->rate_cost;
    g.ws = a->ws; g.out = a->out;
    SSN_TRY(ssn::launch_gen_grads(g, (hipStream_t)stream));
    return 0;
}
int ssn_gen_apply_f32(float* params, const float* grads, float* s1, float* s2, int n, const ssn_opt_params* opt, const float* clip_lo,
                      const float* clip_hi, float* record, void* stream) {
    if (!params || !grads || n <= 0 || (clip_lo == nullptr) != (clip_hi == nullptr)) return refuse("ssn_gen_apply", kInvalid);
    return optimizer_step_full(params, grads, s1, s2, n, opt, nullptr, 0.0, clip_lo, clip_hi, record, record ? grads + n : nullptr, stream);
}

// ---- weight and parameter gradients ---------------------------------------------------------------------------------------------
int ssn_weight_grad_f32(const float* delta, const float* traj, float* gW, int B, long K, int M, int kernel, void* stream) {
    return weight_grad_impl<float>(delta, traj, gW, B, K, M, kernel, stream);
}
int ssn_weight_grad_f64(const double* delta, const double* traj, double* gW, int B, long K, int M, int kernel, void* stream) {
    return weight_grad_impl<double>(delta, traj, gW, B, K, M, kernel, stream);
}
int ssn_weight_grad_scaled_f32(const float* delta, const float* traj, float* gW, int B, long K, int M, const float* dmax,
                               float xmax, void* stream) {
    if (!delta || !traj || !gW || !dmax || B < 0 || K < 0 || M <= 0 || M > 224 || !(xmax > 0.f) || !(xmax < __builtin_inff()) ||
        K * (long)M * 4 >= (1L << 31))
        return refuse("ssn_weight_grad_scaled",
                      "invalid argument (fp32, M <= 224, K M < 2^29, dmax on the device, 0 < xmax < inf)");
    SSN_TRY(ssn::launch_weight_grad_scaled(delta, traj, gW, B, K, M, reinterpret_cast<const unsigned*>(dmax), xmax,
                                           (hipStream_t)stream));
    return 0;
}
int ssn_jds_grad_f32(const float* gW, const float* z, const float* J, const float* D, const float* S, double* out,
                     int B, int N, void* stream) {
    return jds_grad_impl<float>(gW, z, J, D, S, out, B, N, stream);
}
int ssn_jds_grad_f64(const double* gW, const double* z, const double* J, const double* D, const double* S, double* out,
                     int B, int N, void* stream) {
    return jds_grad_impl<double>(gW, z, J, D, S, out, B, N, stream);
}
int ssn_probe_scatter_f32(const float* g, const long* ids, const long* probes, float* g_ta, int n, int B, int NB, int M, void* stream) {
    return probe_scatter_impl<float>(g, ids, probes, g_ta, n, B, NB, M, stream);
}
int ssn_probe_scatter_f64(const double* g, const long* ids, const long* probes, double* g_ta, int n, int B, int NB, int M, void* stream) {
    return probe_scatter_impl<double>(g, ids, probes, g_ta, n, B, NB, M, stream);
}
int ssn_penalty_means_f32(const float* dyn, const float* rate, long n, double scale_dyn, double scale_rate, double* ws, double* out,
                          void* stream) {
    return penalty_means_impl<float>("ssn_penalty_means", dyn, rate, n, scale_dyn, scale_rate, ws, out, nullptr, nullptr, nullptr,
                                     nullptr, 0, 0, 0, stream);
}
int ssn_penalty_means_f64(const double* dyn, const double* rate, long n, double scale_dyn, double scale_rate, double* ws, double* out,
                          void* stream) {
    return penalty_means_impl<double>("ssn_penalty_means", dyn, rate, n, scale_dyn, scale_rate, ws, out, nullptr, nullptr, nullptr,
                                      nullptr, 0, 0, 0, stream);
}
int ssn_penalty_means_probe_f32(const float* dyn, const float* rate, long n, double scale_dyn, double scale_rate, double* ws, double* out,
                                const float* time_avg, const long* ids, const long* probes, float* tc, int nsamp, int NB, int M,
                                void* stream) {
    return penalty_means_impl<float>("ssn_penalty_means_probe", dyn, rate, n, scale_dyn, scale_rate, ws, out, time_avg, ids, probes,
                                     tc, nsamp, NB, M, stream);
}
int ssn_penalty_means_probe_f64(const double* dyn, const double* rate, long n, double scale_dyn, double scale_rate, double* ws, double* out,
                                const double* time_avg, const long* ids, const long* probes, double* tc, int nsamp, int NB, int M,
                                void* stream) {
    return penalty_means_impl<double>("ssn_penalty_means_probe", dyn, rate, n, scale_dyn, scale_rate, ws, out, time_avg, ids, probes,
                                      tc, nsamp, NB, M, stream);
}
long ssn_segment_sqnorms_ws_doubles(int n) { return ssn::segment_sqnorms_ws_doubles(n); }
int ssn_segment_sqnorms2_f32(const float* x, const long* bounds, int n, float* out, double* ws, void* stream) {
    if (n < 0 || (n > 0 && (!x || !bounds || !out || !ws))) return refuse("ssn_segment_sqnorms2", kInvalid);
    SSN_TRY(ssn::launch_segment_sqnorms(x, bounds, n, out, ws, (hipStream_t)stream));
    return 0;
}
// The round-2 signature (no scratch argument), kept under its name so that a caller built against the older header still
// gets what it asked for: the scratch comes from the stream-ordered allocator and goes back behind the two launches.
int ssn_segment_sqnorms_f32(const float* x, const long* bounds, int n, float* out, void* stream) {
    if (n < 0 || (n > 0 && (!x || !bounds || !out))) return refuse("ssn_segment_sqnorms", kInvalid);
    if (n == 0) return 0;
    double* ws = nullptr;
    SSN_TRY(hipMallocAsync((void**)&ws, sizeof(double) * (size_t)ssn::segment_sqnorms_ws_doubles(n), (hipStream_t)stream));
    const hipError_t e = ssn::launch_segment_sqnorms(x, bounds, n, out, ws, (hipStream_t)stream);
    const hipError_t f = hipFreeAsync(ws, (hipStream_t)stream);
    SSN_TRY(e);
    SSN_TRY(f);
    return 0;
}

// ---- critic, its optimizer and the one-call step ----------------------------------------------------------------------------
long ssn_critic_num_params(const int* dims, int nlayers) { return critic_num_params(dims, nullptr, nlayers); }
long ssn_critic_num_params_act(const int* dims, const int* layer_flags, int nlayers) {
    return critic_num_params(dims, layer_flags, nlayers);
}
// The workspace queries cover whichever path the sizes select (critic_path, above).  The _norm one covers every path: a caller
// of the routed entry points who asks it is safe whatever critic he describes.
size_t ssn_critic_workspace_floats(const int* dims, int nlayers, int batch_gd, int batch_p) {
    const size_t base = ssn::critic_workspace_floats(dims, nlayers, batch_gd, batch_p);
    return ssn::critic_fused_supported(dims, nlayers) ? max_sz(base, ssn::critic_fused_workspace_floats(dims, nlayers, batch_gd, batch_p)) : base;
}
size_t ssn_critic_norm_workspace_floats(const int* dims, int nlayers, int batch_gd, int batch_p) {
    return max_sz(ssn::critic_norm_workspace_floats(dims, nlayers, batch_gd, batch_p), ssn_critic_workspace_floats(dims, nlayers, batch_gd, batch_p));
}
// The critic's passes.  Four families of entry points have accumulated (include/ssnode_mi355x.h); each describes its critic with
// its family's helper (plain_spec, leaky_spec, norm_spec, act_spec above) and leaves the rest to critic_net_* above.
// -- plain
int ssn_critic_forward(const float* params, const int* dims, int nlayers, const float* x, const float* cond, int batch,
                       int hide_cell_type, float* out, float* workspace, int precision, void* stream) {
    if (batch == 0) return 0;
    CriticSpec s;
    if (int rc = plain_spec("ssn_critic_forward", params, dims, nlayers, hide_cell_type, precision, s)) return rc;
    return critic_net_forward(s, x, cond, batch, out, workspace, (hipStream_t)stream);
}
int ssn_critic_loss_grad(const float* params, const int* dims, int nlayers, const float* xg, const float* cg,
                         const float* xd, const float* cd, const float* xp, const float* cp, int ng, int nd, int np,
                         float lmd, int hide_cell_type, float* grads, float* stats, float* dvals, float* workspace,
                         int precision, void* stream) {
    CriticSpec s;
    if (int rc = plain_spec("ssn_critic_loss_grad", params, dims, nlayers, hide_cell_type, precision, s)) return rc;
    return critic_net_loss_grad(s, xg, cg, xd, cd, xp, cp, ng, nd, np, lmd, grads, stats, dvals, workspace, (hipStream_t)stream,
                                nullptr, nullptr);
}
int ssn_critic_input_grad(const float* params, const int* dims, int nlayers, const float* x, const float* cond, int batch,
                          int hide_cell_type, float scale, float* gx, float* stats, float* workspace, int precision,
                          void* stream) {
    if (batch == 0) return 0;
    CriticSpec s;
    if (int rc = plain_spec("ssn_critic_input_grad", params, dims, nlayers, hide_cell_type, precision, s)) return rc;
    return critic_net_input_grad(s, x, cond, batch, scale, gx, stats, workspace, (hipStream_t)stream);
}
// -- leaky
int ssn_critic_forward_leaky(const float* params, const int* dims, int nlayers, const float* x, const float* cond, int batch,
                             int hide_cell_type, float leak, float* out, float* workspace, int precision, void* stream) {
    if (batch == 0) return 0;
    CriticSpec s;
    if (int rc = leaky_spec("ssn_critic_forward_leaky", params, dims, nlayers, leak, hide_cell_type, precision, s)) return rc;
    return critic_net_forward(s, x, cond, batch, out, workspace, (hipStream_t)stream);
}
int ssn_critic_loss_grad_leaky(const float* params, const int* dims, int nlayers, const float* xg, const float* cg,
                               const float* xd, const float* cd, const float* xp, const float* cp, int ng, int nd, int np,
                               float lmd, int hide_cell_type, float leak, float* grads, float* stats, float* dvals,
                               float* workspace, int precision, void* stream) {
    CriticSpec s;
    if (int rc = leaky_spec("ssn_critic_loss_grad_leaky", params, dims, nlayers, leak, hide_cell_type, precision, s)) return rc;
    return critic_net_loss_grad(s, xg, cg, xd, cd, xp, cp, ng, nd, np, lmd, grads, stats, dvals, workspace, (hipStream_t)stream,
                                nullptr, nullptr);
}
int ssn_critic_input_grad_leaky(const float* params, const int* dims, int nlayers, const float* x, const float* cond, int batch,
                                int hide_cell_type, float leak, float scale, float* gx, float* stats, float* workspace,
                                int precision, void* stream) {
    if (batch == 0) return 0;
    CriticSpec s;
    if (int rc = leaky_spec("ssn_critic_input_grad_leaky", params, dims, nlayers, leak, hide_cell_type, precision, s)) return rc;
    return critic_net_input_grad(s, x, cond, batch, scale, gx, stats, workspace, (hipStream_t)stream);
}
// -- norm
int ssn_critic_forward_norm(const float* params, const int* dims, const int* layer_norm, int nlayers, const float* x,
                            const float* cond, int batch, int hide_cell_type, float* out, float* workspace, int precision,
                            void* stream) {
    CriticSpec s;
    if (int rc = norm_spec("ssn_critic_forward_norm", params, dims, layer_norm, nlayers, 0.f, hide_cell_type, precision, s)) return rc;
    if (batch == 0) return 0;
    return critic_net_forward(s, x, cond, batch, out, workspace, (hipStream_t)stream);
}
int ssn_critic_loss_grad_norm(const float* params, const int* dims, const int* layer_norm, int nlayers, const float* xg,
                              const float* cg, const float* xd, const float* cd, const float* xp, const float* cp, int ng,
                              int nd, int np, float lmd, int hide_cell_type, float* grads, float* stats, float* dvals,
                              float* workspace, int precision, void* stream) {
    CriticSpec s;
    if (int rc = norm_spec("ssn_critic_loss_grad_norm", params, dims, layer_norm, nlayers, 0.f, hide_cell_type, precision, s)) return rc;
    return critic_net_loss_grad(s, xg, cg, xd, cd, xp, cp, ng, nd, np, lmd, grads, stats, dvals, workspace, (hipStream_t)stream,
                                nullptr, nullptr);
}
int ssn_critic_input_grad_norm(const float* params, const int* dims, const int* layer_norm, int nlayers, const float* x,
                               const float* cond, int batch, int hide_cell_type, float scale, float* gx, float* stats,
                               float* workspace, int precision, void* stream) {
    CriticSpec s;
    if (int rc = norm_spec("ssn_critic_input_grad_norm", params, dims, layer_norm, nlayers, 0.f, hide_cell_type, precision, s)) return rc;
    if (batch == 0) return 0;
    return critic_net_input_grad(s, x, cond, batch, scale, gx, stats, workspace, (hipStream_t)stream);
}
// layer_norm NULL or all zero = plain layers, leak as in the _leaky entry points (plain layers only).
int ssn_critic_accuracy(const float* params, const int* dims, const int* layer_norm, int nlayers, float leak, const float* xg,
                        const float* cg, const float* xd, const float* cd, int ng, int nd, int hide_cell_type, float* acc,
                        float* dvals, float* workspace, int precision, void* stream) {
    CriticSpec s;
    if (int rc = norm_spec("ssn_critic_accuracy", params, dims, layer_norm, nlayers, leak, hide_cell_type, precision, s)) return rc;
    return critic_accuracy(s, xg, cg, xd, cd, ng, nd, acc, dvals, workspace, stream);
}
// -- act
int ssn_critic_forward_act(const float* params, const int* dims, const int* layer_flags, int nlayers, int act, const float* x,
                           const float* cond, int batch, int hide_cell_type, float* out, float* workspace, int precision,
                           void* stream) {
    CriticSpec s;
    if (int rc = act_spec("ssn_critic_forward_act", params, dims, layer_flags, nlayers, act, hide_cell_type, precision, s)) return rc;
    if (batch == 0) return 0;
    return critic_net_forward(s, x, cond, batch, out, workspace, (hipStream_t)stream);
}
int ssn_critic_loss_grad_act(const float* params, const int* dims, const int* layer_flags, int nlayers, int act, const float* xg,
                             const float* cg, const float* xd, const float* cd, const float* xp, const float* cp, int ng,
                             int nd, int np, float lmd, int hide_cell_type, float* grads, float* stats, float* dvals,
                             float* workspace, int precision, void* stream) {
    CriticSpec s;
    if (int rc = act_spec("ssn_critic_loss_grad_act", params, dims, layer_flags, nlayers, act, hide_cell_type, precision, s)) return rc;
    return critic_net_loss_grad(s, xg, cg, xd, cd, xp, cp, ng, nd, np, lmd, grads, stats, dvals, workspace, (hipStream_t)stream,
                                nullptr, nullptr);
}
int ssn_critic_input_grad_act(const float* params, const int* dims, const int* layer_flags, int nlayers, int act, const float* x,
                              const float* cond, int batch, int hide_cell_type, float scale, float* gx, float* stats,
                              float* workspace, int precision, void* stream) {
    CriticSpec s;
    if (int rc = act_spec("ssn_critic_input_grad_act", params, dims, layer_flags, nlayers, act, hide_cell_type, precision, s)) return rc;
    if (batch == 0) return 0;
    return critic_net_input_grad(s, x, cond, batch, scale, gx, stats, workspace, (hipStream_t)stream);
}
int ssn_critic_accuracy_act(const float* params, const int* dims, const int* layer_flags, int nlayers, int act, const float* xg,
                            const float* cg, const float* xd, const float* cd, int ng, int nd, int hide_cell_type, float* acc,
                            float* dvals, float* workspace, int precision, void* stream) {
    CriticSpec s;
    if (int rc = act_spec("ssn_critic_accuracy_act", params, dims, layer_flags, nlayers, act, hide_cell_type, precision, s)) return rc;
    return critic_accuracy(s, xg, cg, xd, cd, ng, nd, acc, dvals, workspace, stream);
}
// -- the optimizer and the one-call step
int ssn_optimizer_step(float* p, const float* g, float* s1, float* s2, long n, const ssn_opt_params* o, void* stream) {
    return optimizer_step_full(p, g, s1, s2, n, o, nullptr, 0.0, nullptr, nullptr, nullptr, nullptr, stream);
}
int ssn_interpolate_f32(const float* eps, const float* xd, const float* xg, float* xp, int rows, int cols, void* stream) {
    if (rows < 0 || cols < 0 || ((long)rows * cols > 0 && (!eps || !xd || !xg || !xp))) return refuse("ssn_interpolate", kInvalid);
    SSN_TRY(ssn::launch_interpolate(eps, xd, xg, xp, rows, cols, (hipStream_t)stream));
    return 0;
}
int ssn_critic_step_run(const ssn_critic_step* a, void* stream) { return critic_step_impl(a, nullptr, 0.0, stream); }
int ssn_critic_step_gated_run(const ssn_critic_step* a, double rate_penalty_bound, void* stream) {
    if (!a || !a->pens64 || !(rate_penalty_bound > 0.0))
        return refuse("ssn_critic_step_gated_run", "needs pens64 and a positive bound");
    return critic_step_impl(a, a->pens64 + 1, rate_penalty_bound, stream);
}

// ---- feed-forward model, moment matching ------------------------------------------------------------------------------------
int ssn_ff_forward_sparse_f32(const float* RF_w, const int* conn_idx, const float* conn_str, int ncon, const float* TH_sam,
                              const float* stim, float* out, float* q, float* den, const ssn_ff_params* p, void* stream) {
    if (!ff_params_ok(p) || ncon < 0 || (q == nullptr) != (den == nullptr) ||
        (p->nsam > 0 && (!RF_w || !TH_sam || !stim || !out || (ncon > 0 && (!conn_idx || !conn_str)))))
        return refuse("ssn_ff_forward_sparse", kInvalid);
    ssn::FFArgs a = ff_args(*p);
    a.RF_w = RF_w; a.TH_sam = TH_sam; a.stim = stim; a.out = out; a.q = q; a.den = den;
    ssn::FFLattice lat;
    const bool lattice = ff_lattice(stim, p->ni, lat, stream);
    SSN_TRY(ssn::launch_ff_forward_sparse(a, lattice ? &lat : nullptr, conn_idx, conn_str, ncon, (hipStream_t)stream));
    return 0;
}
int ssn_ff_backward_sparse_f32(const float* RF_w, const int* conn_idx, const float* conn_str, int ncon, const float* stim, const float* q,
                               const float* den, const float* gq, float* dsig, const ssn_ff_params* p, void* stream) {
    if (!ff_params_ok(p) || ncon < 0 || !q || !den || !gq || !dsig ||
        (p->nsam > 0 && (!RF_w || !stim || (ncon > 0 && (!conn_idx || !conn_str)))))
        return refuse("ssn_ff_backward_sparse", kInvalid);
    ssn::FFArgs a = ff_args(*p);
    a.RF_w = RF_w; a.stim = stim; a.q = const_cast<float*>(q); a.den = const_cast<float*>(den);
    SSN_TRY(ssn::launch_ff_backward_sparse(a, conn_idx, conn_str, ncon, gq, dsig, (hipStream_t)stream));
    return 0;
}
int ssn_ff_forward_f32(const float* RF_w, const float* FF_con, const float* FF_str, const float* TH_sam,
                       const float* stim, float* out, float* q, float* den, const ssn_ff_params* p, void* stream) {
    if (!ff_params_ok(p) || (q == nullptr) != (den == nullptr)) return refuse("ssn_ff_forward", kInvalid);
    if (int rc = ff_dense_alignment("ssn_ff_forward", *p, RF_w, FF_con, FF_str)) return rc;
    ssn::FFArgs a = ff_args(*p);
    a.RF_w = RF_w; a.FF_con = FF_con; a.FF_str = FF_str; a.TH_sam = TH_sam; a.stim = stim; a.out = out; a.q = q; a.den = den;
    ssn::FFLattice lat;
    const bool lattice = ff_lattice(stim, p->ni, lat, stream);
    SSN_TRY(ssn::launch_ff_forward(a, lattice ? &lat : nullptr, (hipStream_t)stream));
    return 0;
}
int ssn_ff_backward_f32(const float* RF_w, const float* FF_con, const float* FF_str, const float* stim, const float* q,
                        const float* den, const float* gq, float* dsig, const ssn_ff_params* p, void* stream) {
    if (!ff_params_ok(p) || !q || !den || !gq || !dsig) return refuse("ssn_ff_backward", kInvalid);
    if (int rc = ff_dense_alignment("ssn_ff_backward", *p, RF_w, FF_con, FF_str)) return rc;
    ssn::FFArgs a = ff_args(*p);
    a.RF_w = RF_w; a.FF_con = FF_con; a.FF_str = FF_str; a.stim = stim;
    a.q = const_cast<float*>(q); a.den = const_cast<float*>(den);
    SSN_TRY(ssn::launch_ff_backward(a, gq, dsig, (hipStream_t)stream));
    return 0;
}
int ssn_moment_sums_f32(const float* x, int B, int D, double* sums, void* stream) {
    if (B < 0 || D < 0 || (D > 0 && (!x || !sums))) return refuse("ssn_moment_sums", kInvalid);
    SSN_TRY(ssn::launch_moment_sums(x, B, D, sums, (hipStream_t)stream));
    return 0;
}
int ssn_moment_loss_grad_f32(const float* x, const double* sums, double global_batch, const double* data_moments,
                             const double* weights, int B, int D, float* gx, double* out, void* stream) {
    if (B < 0 || D < 0 || !(global_batch > 0) || !out || (D > 0 && (!x || !sums || !data_moments || !weights || !gx)))
        return refuse("ssn_moment_loss_grad", kInvalid);
    SSN_TRY(ssn::launch_moment_loss_grad(x, sums, global_batch, data_moments, weights, B, D, gx, out, (hipStream_t)stream));
    return 0;
}

// ---- steady-state gradient ------------------------------------------------------------------------------------------------------
int ssn_build_dw_f32(const float* z, const float* J, const float* D, const float* S, int which, float* dW, int B, int N,
                     void* stream) { return build_dw_impl<float>(z, J, D, S, which, dW, B, N, stream); }
int ssn_build_dw_f64(const double* z, const double* J, const double* D, const double* S, int which, double* dW, int B,
                     int N, void* stream) { return build_dw_impl<double>(z, J, D, S, which, dW, B, N, stream); }
int ssn_ss_grad_system_f32(const float* R, const float* W, const float* dW, int dw_per_draw, const float* I,
                           int i_per_draw, int nz, int nb, int M, const ssn_solver_params* p, float* A, float* rhs,
                           void* stream) {
    return ss_system_impl<float>(R, W, dW, dw_per_draw, I, i_per_draw, nz, nb, M, p, A, rhs, stream);
}
int ssn_ss_grad_system_f64(const double* R, const double* W, const double* dW, int dw_per_draw, const double* I,
                           int i_per_draw, int nz, int nb, int M, const ssn_solver_params* p, double* A, double* rhs,
                           void* stream) {
    return ss_system_impl<double>(R, W, dW, dw_per_draw, I, i_per_draw, nz, nb, M, p, A, rhs, stream);
}
int ssn_lu_solve_f32(float* A, float* rhs, int* info, int nsys, int M, int nrhs, void* stream) {
    return lu_solve_impl<float>(A, rhs, info, nsys, M, nrhs, stream);
}
int ssn_lu_solve_f64(double* A, double* rhs, int* info, int nsys, int M, int nrhs, void* stream) {
    return lu_solve_impl<double>(A, rhs, info, nsys, M, nrhs, stream);
}

// ---- ensembles ------------------------------------------------------------------------------------------------------------------
long ssn_ens_record_doubles(int D, int P) { return (D < 0 || P < 0) ? -1 : 4L + 2L * D + 2L * P; }
int ssn_ens_moments_f32(const float* x, int K, int B, int D, double* sums, const double* data_moments, const double* weights,
                        float* gx, double* rec, int rstride, void* stream) {
    if (K < 0 || B <= 0 || D < 0 || rstride < ssn_ens_record_doubles(D, 0) ||
        (K > 0 && D > 0 && (!x || !sums || !data_moments || !weights || !gx || !rec)))
        return refuse("ssn_ens_moments", kInvalid);
    SSN_TRY(ssn::launch_ens_moments(x, K, B, D, sums, data_moments, weights, gx, rec, rstride, (hipStream_t)stream));
    return 0;
}
int ssn_ens_jds_grad_f32(const float* gW, const float* z, const float* p16, double* out, int K, int B, int N, void* stream) {
    if (K < 0 || B < 0 || N < 1 || (K > 0 && B > 0 && (!gW || !z || !p16 || !out))) return refuse("ssn_ens_jds_grad", kInvalid);
    SSN_TRY(ssn::launch_ens_jds_grad(gW, z, p16, out, K, B, N, (hipStream_t)stream));
    return 0;
}
int ssn_ens_gen_grads_f32(const ssn_ens_grads* a, void* stream) {
    if (a && a->D == 0)                        // (L0 would be 0 / 0: a loss without moments hands its own L0 in)
        return refuse("ssn_ens_gen_grads",
                      "D must be at least 1 (a loss that is not a function of moments takes ssn_ens_gen_grads_l0_f32)");
    if (!a || a->K < 0 || a->B <= 0 || a->nv < 0 || a->nv > 2 || a->NB <= 0 || a->M <= 0 || (a->M & 1) || a->D < 0 ||
        a->rstride < ssn_ens_record_doubles(a->D, a->nv + 12) ||
        (a->K > 0 && (!a->part || !a->dyn_row || !a->rate_row || !a->data_moments || !a->weights || !a->costs || !a->grads ||
                      !a->rec || (a->nv > 0 && (!a->g_ext || !a->ext_base || !a->zin)))))
        return refuse("ssn_ens_gen_grads", kInvalid);
    return ens_gen_grads_launch(a, nullptr, stream);
}
int ssn_ens_gen_grads_l0_f32(const ssn_ens_grads* a, const double* l0, void* stream) {
    if (!a || a->K < 0 || a->B <= 0 || a->nv < 0 || a->nv > 2 || a->NB <= 0 || a->M <= 0 || (a->M & 1) || a->D != 0 ||
        a->data_moments || a->weights || a->rstride < ssn_ens_record_doubles(0, a->nv + 12) ||
        (a->K > 0 && (!l0 || !a->part || !a->dyn_row || !a->rate_row || !a->costs || !a->grads || !a->rec ||
                      (a->nv > 0 && (!a->g_ext || !a->ext_base || !a->zin)))))
        return refuse("ssn_ens_gen_grads_l0", "invalid argument (D must be 0, data_moments and weights null)");
    return ens_gen_grads_launch(a, l0, stream);
}
int ssn_ens_apply_f32(const ssn_ens_apply* a, void* stream) {
    if (!a || a->K < 0 || a->P <= 0 || a->kind < 0 || a->kind > 2 || a->rec_off < 0 || a->rstride < a->rec_off + 2 * a->P ||
        (a->K > 0 && (!a->hyp || !a->clip_lo || !a->clip_hi || !a->p || !a->g || !a->rec || (a->kind > 0 && !a->s1) ||
                      (a->kind == 1 && !a->s2))))
        return refuse("ssn_ens_apply", kInvalid);
    ssn::EnsApplyArgs g{};
    g.K = a->K; g.P = a->P; g.kind = a->kind; g.beta1 = a->beta1; g.beta2 = a->beta2; g.eps = a->eps; g.rho = a->rho;
    g.hyp = a->hyp; g.clip_lo = a->clip_lo; g.clip_hi = a->clip_hi; g.p = a->p; g.s1 = a->s1; g.s2 = a->s2; g.g = a->g;
    g.rec = a->rec; g.rstride = a->rstride; g.rec_off = a->rec_off;
    SSN_TRY(ssn::launch_ens_apply(g, (hipStream_t)stream));
    return 0;
}
int ssn_ens_stimulus_hetero_f32(const float* bw, const float* con, float smoothness, const float* zin, const float* v, float* ext,
                                int K, int B, int NB, int N, void* stream) {
    if (K < 0 || B < 0 || NB < 0 || N < 1 || !(smoothness > 0.f) || ((long)K * B * NB > 0 && (!bw || !con || !zin || !v || !ext)))
        return refuse("ssn_ens_stimulus_hetero", kInvalid);
    SSN_TRY(ssn::launch_ens_stimulus_hetero(bw, con, smoothness, zin, v, ext, K, B, NB, N, (hipStream_t)stream));
    return 0;
}

// ---- scorer and sliced Wasserstein ----------------------------------------------------------------------------------------------
int ssn_tc_features_f32(const float* tc, float* feat, long rows, int NC, int NB, int Q, void* stream) {
    if (rows < 0 || NC < 0 || NB < 1 || Q < 0 || (rows * NC * Q > 0 && (!tc || !feat))) return refuse("ssn_tc_features_f32", kInvalid);
    SSN_TRY(ssn::launch_tc_features(tc, feat, rows, NC, NB, Q, (hipStream_t)stream));
    return 0;
}
int ssn_ks_columns_f32(const float* x, const float* truth_sorted, const int* m, int S, int B, int C, int T, int* n,
                       long long* num, void* stream) {
    return ks_columns("ssn_ks_columns_f32", false, x, truth_sorted, m, S, B, C, T, n, num, nullptr, stream);
}
int ssn_ks_w1_columns_f32(const float* x, const float* truth_sorted, const int* m, int S, int B, int C, int T, int* n,
                          long long* num, double* wnum, void* stream) {
    return ks_columns("ssn_ks_w1_columns_f32", true, x, truth_sorted, m, S, B, C, T, n, num, wnum, stream);
}
int ssn_project_rows_f32(const float* x, long rows, int ldx, int C, const float* theta, int L, float* out, void* stream) {
    if (L > SSN_W1_MAX_DIRECTIONS) return refuse("ssn_project_rows_f32", kTooManyDirections);
    if (rows < 0 || C < 0 || L < 0 || ldx < C || (rows * L > 0 && (!out || (C > 0 && (!x || !theta)))))
        return refuse("ssn_project_rows_f32", kInvalid);
    SSN_TRY(ssn::launch_project_rows(x, rows, ldx, C, theta, L, out, (hipStream_t)stream));
    return 0;
}
int ssn_swd_match_f32(const float* px, const float* py, int B, int L, int power, float* coef, double* loss_l, void* stream) {
    if (B > SSN_SWD_MAX_BATCH) return refuse("ssn_swd_match_f32", "more than 4096 rows (keys and values are sorted in 48 KiB of LDS)");
    if (L > SSN_W1_MAX_DIRECTIONS) return refuse("ssn_swd_match_f32", kTooManyDirections);
    if (B < 0 || L < 0 || (power != 1 && power != 2) || ((long)B * L > 0 && (!px || !py || !coef || !loss_l)))
        return refuse("ssn_swd_match_f32", kInvalid);
    SSN_TRY(ssn::launch_swd_match(px, py, B, L, power, coef, loss_l, (hipStream_t)stream));
    return 0;
}
int ssn_swd_backproject_f32(const float* coef, const float* theta, int B, int L, int D, float* gx, void* stream) {
    if (L > SSN_W1_MAX_DIRECTIONS) return refuse("ssn_swd_backproject_f32", kTooManyDirections);
    if (B < 0 || L < 0 || D < 0 || ((long)B * D > 0 && (!gx || (L > 0 && (!coef || !theta)))))
        return refuse("ssn_swd_backproject_f32", kInvalid);
    SSN_TRY(ssn::launch_swd_backproject(coef, theta, B, L, D, gx, (hipStream_t)stream));
    return 0;
}
int ssn_ens_swd_project_f32(const float* x, const float* y, const float* theta, int K, int B, int L, int D, float* px, float* py,
                            void* stream) {
    if (int err = ens_swd_limits("ssn_ens_swd_project_f32", K, B, L)) return err;
    if (K < 0 || B < 0 || L < 0 || D < 0 || ((long)K * B * L > 0 && (!px || !py || (D > 0 && (!x || !y || !theta)))))
        return refuse("ssn_ens_swd_project_f32", kInvalid);
    SSN_TRY(ssn::launch_ens_swd_project(x, y, theta, K, B, L, D, px, py, (hipStream_t)stream));
    return 0;
}
int ssn_ens_swd_match_f32(const float* px, const float* py, const int* power, int K, int B, int L, int form, float* coef,
                          double* loss_l, double* l0, void* stream) {
    const char* const fn = "ssn_ens_swd_match_f32";
    if (int err = ens_swd_limits(fn, K, B, L)) return err;
    if (K < 0 || B < 0 || L < 0 || (K > 0 && !power)) return refuse(fn, kInvalid);
    ssn::SwdPowerBits bits{};
    for (int k = 0; k < K; ++k) {
        if (power[k] != 1 && power[k] != 2) return refuse(fn, "a power other than 1 or 2");
        if (power[k] == 2) bits.w[k >> 5] |= 1u << (k & 31);
    }
    if (form != SSN_SWD_FORM_AUTO && form != SSN_SWD_FORM_GENERAL && form != SSN_SWD_FORM_WAVE) return refuse(fn, "unknown form");
    if (form == SSN_SWD_FORM_WAVE && B > SSN_SWD_WAVE_MAX_BATCH) return refuse(fn, "the wave form takes at most 64 rows per member");
    if ((long)K * B * L > 0 && (!px || !py || !coef || !loss_l || !l0)) return refuse(fn, "invalid argument (null pointer)");
    SSN_TRY(ssn::launch_ens_swd_match(px, py, bits, K, B, L, form, coef, loss_l, l0, (hipStream_t)stream));
    return 0;
}
int ssn_ens_swd_backproject_f32(const float* coef, const float* theta, int K, int B, int L, int D, float* gx, void* stream) {
    if (int err = ens_swd_limits("ssn_ens_swd_backproject_f32", K, B, L)) return err;
    if (K < 0 || B < 0 || L < 0 || D < 0 || ((long)K * B * D > 0 && (!gx || (L > 0 && (!coef || !theta)))))
        return refuse("ssn_ens_swd_backproject_f32", kInvalid);
    if (L == 0) {                                             // (as the single-run entry: no direction, zeros)
        if ((long)K * B * D > 0) SSN_TRY(hipMemsetAsync(gx, 0, (size_t)K * B * D * sizeof(float), (hipStream_t)stream));
        return 0;
    }
    SSN_TRY(ssn::launch_ens_swd_backproject(coef, theta, K, B, L, D, gx, (hipStream_t)stream));
    return 0;
}
int ssn_fp_select_max_candidates(void) { return ssn::fp_select_max_candidates(); }
int ssn_fp_select_f64(const int* codes, const double* x, int A, int R, int NB, int M, const int* probes, int nprobe, const int* set_of,
                      int cand0, int NZ, int* verdict, double* out, int* accepted, int* used, int* rejections, int* draw_index,
                      void* stream) {
    return fp_select_impl<double>("ssn_fp_select_f64", codes, x, A, R, NB, M, probes, nprobe, set_of, cand0, NZ, verdict, out, accepted,
                                  used, rejections, draw_index, stream);
}
int ssn_fp_select_f32(const int* codes, const float* x, int A, int R, int NB, int M, const int* probes, int nprobe, const int* set_of,
                      int cand0, int NZ, int* verdict, float* out, int* accepted, int* used, int* rejections, int* draw_index,
                      void* stream) {
    return fp_select_impl<float>("ssn_fp_select_f32", codes, x, A, R, NB, M, probes, nprobe, set_of, cand0, NZ, verdict, out, accepted,
                                 used, rejections, draw_index, stream);
}

// ---- MT19937 / Philox -----------------------------------------------------------------------------------------------------------
int ssn_mt19937_jump_poly(unsigned long long nblocks, unsigned long long* bits) {
    if (!bits) return refuse("ssn_mt19937_jump_poly", "null output");
    if (ssn::mt19937_jump_poly(nblocks, bits) != 0)
        return refuse_as(hipErrorUnknown, "ssn_mt19937_jump_poly",
                         "the characteristic polynomial did not come out with degree 19937");
    return 0;
}
int ssn_mt19937_random_sample_f32(unsigned int* key, int* pos, unsigned long long total, unsigned long long skip,
                                  unsigned long long count, float* out, void* stream) {
    return mt_sample<float>(key, pos, total, skip, count, out, stream);
}
int ssn_mt19937_random_sample_f64(unsigned int* key, int* pos, unsigned long long total, unsigned long long skip,
                                  unsigned long long count, double* out, void* stream) {
    return mt_sample<double>(key, pos, total, skip, count, out, stream);
}
int ssn_mt19937_random_sample_begin_f32(const unsigned int* key, int pos, unsigned long long total, unsigned long long skip,
                                        unsigned long long count, float* out, void* stream, int* ticket) {
    return mt_sample_begin<float>(key, pos, total, skip, count, out, stream, ticket);
}
int ssn_mt19937_random_sample_begin_f64(const unsigned int* key, int pos, unsigned long long total, unsigned long long skip,
                                        unsigned long long count, double* out, void* stream, int* ticket) {
    return mt_sample_begin<double>(key, pos, total, skip, count, out, stream, ticket);
}
int ssn_mt19937_random_sample_tail_begin_f32(const unsigned int* key, int pos, unsigned long long total, unsigned long long skip,
                                             unsigned long long count, float* out, int tail_kind, unsigned long long tail_total,
                                             unsigned long long tail_skip, unsigned long long tail_count, float* tail_out, void* stream,
                                             int* ticket) {
    const char* const fn = "ssn_mt19937_random_sample_tail_begin";
    if (!key || !ticket) return refuse(fn, "null state / ticket");
    *ticket = -1;                              // (also on the refusal below)
    if (tail_kind != 1 && tail_kind != 2) return refuse(fn, "tail_kind must be 1 (choice(2, n) * 2 - 1) or 2 (rand(n) * 2 - 1)");
    const ssn::MtTail tail = mt_tail(tail_kind, tail_total, tail_skip, tail_count, tail_out);
    return mt_begin(key, pos, total, skip, count, out, 4, stream, ticket, nullptr, nullptr, 0, &tail);
}
int ssn_build_w_mt19937_begin_f32(const unsigned int* key, int pos, int B_total, int b0, int nb, const float* J, const float* D,
                                  const float* S, float* W, float* z, int N, void* stream, int* ticket) {
    if (!key || !ticket || !J || !D || !S || !W || N < 1 || B_total < 0 || b0 < 0 || nb < 0 || b0 + nb > B_total)
        return refuse("ssn_build_w_mt19937_begin", kInvalid);
    float jds[12];
    pack_jds(J, D, S, jds);
    const unsigned long long mm = 4ull * N * N;
    return mt_begin(key, pos, mm * B_total, mm * b0, mm * nb, z, 4, stream, ticket, nb ? W : nullptr, jds, N);
}
int ssn_build_w_mt19937_tail_begin_f32(const unsigned int* key, int pos, int B_total, int b0, int nb, const float* J, const float* D,
                                       const float* S, float* W, float* z, int N, int tail_kind, float* zin, void* stream, int* ticket) {
    if (!key || !ticket || !J || !D || !S || (nb && (!W || !zin)) || N < 1 || B_total < 0 || b0 < 0 || nb < 0 || b0 + nb > B_total
        || (tail_kind != 1 && tail_kind != 2))
        return refuse("ssn_build_w_mt19937_tail_begin", kInvalid);
    float jds[12];
    pack_jds(J, D, S, jds);
    const unsigned long long mm = 4ull * N * N, m = 2ull * N;
    const ssn::MtTail tail = mt_tail(tail_kind, m * B_total, m * b0, m * nb, zin);
    return mt_begin(key, pos, mm * B_total, mm * b0, mm * nb, z, 4, stream, ticket, nb ? W : nullptr, jds, N, &tail);
}
int ssn_mt19937_plan(int pos, unsigned long long total, unsigned long long skip, unsigned long long count, long* out) {
    if (!out || !ssn::mt19937_plan(pos, total, skip, count, out)) return refuse("ssn_mt19937_plan", kInvalid);
    return 0;
}
int ssn_mt19937_plan_tail(int pos, unsigned long long total, unsigned long long skip, unsigned long long count, int tail_kind,
                          unsigned long long tail_total, unsigned long long tail_skip, unsigned long long tail_count, long* out) {
    const ssn::MtTail tail = mt_tail(tail_kind, tail_total, tail_skip, tail_count, nullptr);
    if (!out || !ssn::mt19937_plan(pos, total, skip, count, out, &tail)) return refuse("ssn_mt19937_plan_tail", kInvalid);
    return 0;
}
int ssn_mt19937_random_sample_finish(int ticket, unsigned int* key, int* pos) {
    if (!key || !pos) return refuse("ssn_mt19937_random_sample_finish", "null state");
    SSN_TRY(ssn::mt19937_finish(ticket, key, pos));
    return 0;
}
int ssn_philox_amp_f32(unsigned long long seed, unsigned long long offset, const float* v, float* zin, float* amp, unsigned long long n,
                       int M, int bernoulli, void* stream) {
    return philox_amp_impl<float>(seed, offset, v, zin, amp, n, M, bernoulli, stream);
}
int ssn_philox_amp_f64(unsigned long long seed, unsigned long long offset, const double* v, double* zin, double* amp,
                       unsigned long long n, int M, int bernoulli, void* stream) {
    return philox_amp_impl<double>(seed, offset, v, zin, amp, n, M, bernoulli, stream);
}
int ssn_philox_uniform_f32(unsigned long long seed, unsigned long long offset, float* out, unsigned long long n, void* stream) {
    return philox_uniform_impl<float>(seed, offset, out, n, stream);
}
int ssn_philox_uniform_f64(unsigned long long seed, unsigned long long offset, double* out, unsigned long long n, void* stream) {
    return philox_uniform_impl<double>(seed, offset, out, n, stream);
}

}  // extern "C"
