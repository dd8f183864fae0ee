// Shared host-side helpers for libfoamyade_hip.so (product code; never includes anything from oracle/).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/foamyade_hip.h"

namespace fy {

// Run-time switches: environment variables, read here and nowhere else, when an object is created.  None changes a
// result (amg_passes: the preconditioner, so the path to the converged solution).  Deployment options and test aids only -- an A/B timing experiment is a build variant (tools/build_variant.sh), never a shipped switch.
struct Options {
    // deployment
    std::string tree_cache_dir;  // FOAMYADE_TREE_CACHE_DIR      ranks of one node share the k-d build through this directory ("" = off)
    int rebin_interval;          // FOAMYADE_REBIN_INTERVAL      counting sort of the particles every this many steps (default 32; locality only)
    int strip_blocks;            // FOAMYADE_STRIP_BLOCKS=n       blocks per strip of the FV cell sweeps (0: off; unset, -1: ~8 rows of cells)
    bool halo_overlap;           // FOAMYADE_HALO_OVERLAP=0       every slab exchange is followed by its consumer (serial schedule; identical results); default 1
    int ipc_slot_mb;             // FOAMYADE_IPC_SLOT_MB         peer-store communicator: MiB per neighbour slot (0: unset)
    long long ipc_timeout_ms;    // FOAMYADE_IPC_TIMEOUT_MS      peer-store communicator: bound of a device-side wait for a peer (0: unset)
    bool wire_trace;             // FOAMYADE_WIRE_TRACE          drop-in leg: per-step trace of the wire's copies on the device clock (stderr)
    bool explicit_tree;          // FOAMYADE_EXPLICIT_TREE=1     32-byte explicit tree nodes even on a lattice block (what a general mesh gets)
    // test aids: the path that a test holds the default against
    bool no_locate_lists;        // FOAMYADE_NO_LOCATE_LISTS=1   the plain tree walk places every particle (what a general mesh gets)
    int locate_stack;            // FOAMYADE_LOCATE_STACK=n      explicit tree: the walk's LDS stack depth (0: the full depth; unset, -1: measured per step)
    bool locate_wide;            // FOAMYADE_LOCATE_WIDE=1       explicit tree: the 16-byte stack entries of 2^25 cells and more on any tree
    bool no_deep_vcycle;         // FOAMYADE_NO_DEEP_VCYCLE=1    slab multigrid: one exchange per sweep instead of one per level and cycle
    long long mg_replicate_below; // FOAMYADE_MG_REPLICATE_BELOW=n  slab multigrid: levels of <= n global cells are replicated (0, unset: kMgReplicateBelow)
    int amg_passes;              // FOAMYADE_AMG_PASSES=1..3     general-mesh multigrid: pairwise matching passes per level (unset: 3), so that a small case carries many levels
    bool localcomm_stream;       // FOAMYADE_LOCALCOMM_STREAM=1  in-process slab groups: collectives as event waits on the ranks' streams
    bool no_fused_corrector;     // FOAMYADE_NO_FUSED_CORRECTOR=1  the corrector as five sweeps instead of the two fused ones
    bool faces_from_arrays;      // FOAMYADE_FACES_FROM_ARRAYS=1   the fused sweeps stream rAUf / alphacf from their face arrays instead of re-forming them
    bool no_tiled_stress;        // FOAMYADE_NO_TILED_STRESS=1   explicit stress term: the tensor through memory (two sweeps) instead of the LDS-tiled sweep
    bool no_pairs;               // FOAMYADE_NO_PAIRS=1         pressure solver: one cell per thread in every sweep instead of two
    bool no_tail_cache;          // FOAMYADE_NO_TAIL_CACHE=1     multigrid tail: the first level from global memory instead of LDS
    int ipc_slot_kb;             // FOAMYADE_IPC_SLOT_KB         peer-store communicator: KiB per neighbour slot, overrides ipc_slot_mb (0: unset)
};
Options options();

// thread-local last-error text behind fy_last_error()
std::string& last_error();
int fail(int code, const char* fmt, ...);
// The kernel layer's switches, as the latest options() call read them (a process-wide snapshot: the launchers are not handed an object)
bool pairs_disabled();           // no_pairs
bool tail_cache_disabled();      // no_tail_cache
bool locate_wide_forced();       // locate_wide

#define FY_HIP(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess)                                                                             \
            return ::fy::fail(FY_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

#define FY_TRY(expr)                 \
    do {                             \
        int _rc = (expr);            \
        if (_rc != FY_OK) return _rc; \
    } while (0)

// Owning device allocation.  All product state lives in HBM; there is no host fallback.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    // grow-only (keeps the allocation across steps; sized for the largest batch seen)
    int reserve(size_t count) {
        if (count <= n) return FY_OK;
        release();
        size_t cap = count + count / 8 + 64;
        hipError_t e = hipMalloc((void**)&p, cap * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            return fail(FY_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", cap * sizeof(T), hipGetErrorString(e));
        }
        n = cap;
        return FY_OK;
    }
    int alloc_exact(size_t count) {
        release();
        if (count == 0) return FY_OK;
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            return fail(FY_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
        }
        n = count;
        return FY_OK;
    }
};

// Owning PINNED host allocation (hipHostMalloc): the staging side of every host<->device copy on the drop-in path.  Copies from or to
// pageable memory are staged by the runtime through its own small pinned buffers and block the caller; from pinned memory they run
// at PCIe rate, asynchronously, on whatever stream they are put on.
template <class T>
struct HostBuf {
    T* p = nullptr;
    size_t n = 0;
    HostBuf() = default;
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
    ~HostBuf() { release(); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
    T* data() { return p; }
    T& operator[](size_t i) { return p[i]; }
    int reserve(size_t count) {          // grow-only, contents not kept
        if (count <= n) return FY_OK;
        release();
        const size_t cap = count + count / 8 + 64;
        hipError_t e = hipHostMalloc((void**)&p, cap * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(FY_ERR_HIP, "hipHostMalloc(%zu bytes) failed: %s", cap * sizeof(T), hipGetErrorString(e));
        }
        n = cap;
        return FY_OK;
    }
};

// Read-back of a folded reduction through MAPPED pinned host memory (both solvers' reduce_read): the fold (launch_reduce_finalize) writes its results straight into `host`
// through the device alias `dev` and stores a sequence number behind each in one of eight arrival flags; the host spins on the flags -- in-order stream: everything
// enqueued before the fold has completed by then -- so a read-back costs neither a device-to-host blit nor a stream synchronisation.  init() never fails: without mapped
// memory (!mapped()) the owner folds on the device and copies, without flags (!flagged()) it synchronises the stream before it reads `host`.
struct MappedReadback {
    static constexpr int kFlags = 8;
    double *host = nullptr, *dev = nullptr;    // `ndoubles` doubles: the first kFlags are wait()'s landing zone, the rest the owner's (the block solver's deferred slots)
    unsigned long long *flag = nullptr, *flag_dev = nullptr;
    unsigned long long seq = 0;                // what the latest fold stores into its flags
    MappedReadback() = default;
    MappedReadback(const MappedReadback&) = delete;
    MappedReadback& operator=(const MappedReadback&) = delete;
    ~MappedReadback() { if (host) (void)hipHostFree(host); if (flag) (void)hipHostFree(flag); }
    void init(size_t ndoubles) {
        if (hipHostMalloc((void**)&host, ndoubles * sizeof(double), hipHostMallocMapped) != hipSuccess) host = nullptr;
        if (host && hipHostGetDevicePointer((void**)&dev, host, 0) != hipSuccess) { (void)hipHostFree(host); host = nullptr; }
        if (!host) return;
        if (hipHostMalloc((void**)&flag, kFlags * sizeof(unsigned long long), hipHostMallocMapped) != hipSuccess) flag = nullptr;
        if (flag && hipHostGetDevicePointer((void**)&flag_dev, flag, 0) != hipSuccess) { (void)hipHostFree(flag); flag = nullptr; }
        if (flag) for (int q = 0; q < kFlags; ++q) flag[q] = 0;
    }
    bool mapped() const { return host != nullptr; }
    bool flagged(int nslots) const { return flag && nslots <= kFlags; }
    double* slot(int i) { return host + i; }                   // (and dev + i on the device)
    // the fold was launched on `stream` with ++seq: wait for its `nslots` flags and take the results.  idle(): what the host does meanwhile, every 1024 spins
    template <class Idle>
    int wait(hipStream_t stream, int nslots, double* out, Idle&& idle) {
        for (int q = 0; q < nslots; ++q) {
            unsigned long spins = 0;
            while (__atomic_load_n(&flag[q], __ATOMIC_ACQUIRE) != seq) {
                if ((++spins & 0x3ffu) == 0) FY_TRY(idle());
                if ((spins & 0xfffu) == 0) {                        // every 4096 polls: is the stream still alive?
                    const hipError_t e = hipStreamQuery(stream);
                    if (e == hipSuccess) { if (__atomic_load_n(&flag[q], __ATOMIC_ACQUIRE) == seq) break; return fail(FY_ERR_HIP, "reduction flag never arrived"); }
                    if (e != hipErrorNotReady) return fail(FY_ERR_HIP, "stream failed while waiting for a reduction: %s", hipGetErrorString(e));
                }
            }
            out[q] = host[q];
        }
        return FY_OK;
    }
    int wait(hipStream_t stream, int nslots, double* out) { return wait(stream, nslots, out, [] { return FY_OK; }); }
};

struct EventTimer {
    hipEvent_t a = nullptr, b = nullptr;
    bool armed = false;
    int init() {
        FY_HIP(hipEventCreate(&a));
        FY_HIP(hipEventCreate(&b));
        return FY_OK;
    }
    void destroy() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        a = b = nullptr;
    }
    void start(hipStream_t s) { (void)hipEventRecord(a, s); armed = true; }
    void stop(hipStream_t s) { (void)hipEventRecord(b, s); }
    double ms() {
        if (!armed) return 0.0;
        float t = 0.f;
        (void)hipEventSynchronize(b);
        (void)hipEventElapsedTime(&t, a, b);
        armed = false;
        return (double)t;
    }
};

// consecutive phases on one stream share their boundary events: N + 1 records for N phases (an event record between two kernels idles
// the stream for several microseconds, so every pair that can be saved is)
struct PhaseMarks {
    static constexpr int kMax = 8;
    hipEvent_t ev[kMax] = {};
    bool set_[kMax] = {};
    int init() { for (auto& e : ev) FY_HIP(hipEventCreate(&e)); return FY_OK; }
    void destroy() { for (auto& e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; } }
    void clear() { for (auto& b : set_) b = false; }
    void mark(int i, hipStream_t s) { (void)hipEventRecord(ev[i], s); set_[i] = true; }
    double ms(int i, int j) {
        if (!set_[i] || !set_[j]) return 0.0;
        float t = 0.f;
        (void)hipEventSynchronize(ev[j]);
        (void)hipEventElapsedTime(&t, ev[i], ev[j]);
        return (double)t;
    }
};

// accumulating per-kernel clock: one HIP event pair per launch, recorded on the launch stream, harvested once per step
struct KernelClock {
    std::vector<hipEvent_t> a, b;
    size_t used = 0;
    double total_ms = 0.0;
    int64_t launches = 0;
    bool on = false;
    // An event record between two kernels costs the stream 5 - 10 us of idle GPU (kernel trace: 10.9 us between two level-0 sweeps with
    // the clock on, 0 without).  The clock therefore SAMPLES: the first `per_collect` launches after each collect() are timed -- every
    // launch of a category does the same work -- so what it measures does not slow down what it measures by more than that.
    size_t per_collect = 1;
    bool open_ = false;
    void begin(hipStream_t s) {
        open_ = false;
        if (!on || used >= per_collect) return;
        if (used == a.size()) { hipEvent_t x, y; (void)hipEventCreate(&x); (void)hipEventCreate(&y); a.push_back(x); b.push_back(y); }
        (void)hipEventRecord(a[used], s);
        open_ = true;
    }
    void end(hipStream_t s) {
        if (!open_) return;
        (void)hipEventRecord(b[used], s);
        ++used;
        open_ = false;
    }
    void collect() {       // call after the stream has been synchronised
        for (size_t i = 0; i < used; ++i) { float t = 0.f; (void)hipEventElapsedTime(&t, a[i], b[i]); total_ms += t; }
        launches += (int64_t)used;
        used = 0;
    }
    void reset() { used = 0; total_ms = 0.0; launches = 0; }
    void destroy() { for (auto e : a) (void)hipEventDestroy(e); for (auto e : b) (void)hipEventDestroy(e); a.clear(); b.clear(); }
};

inline unsigned div_up(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

// setDeltaT.H [OF-6] (pimpleFoamYade.C:64): the next deltaT from the Courant number of the current flux at the old one
inline double next_delta_t(double dt, double courant_max, double max_co, double max_delta_t) {
    const double maxDeltaTFact = max_co / (courant_max + 1e-15);
    const double deltaTFact = std::min(std::min(maxDeltaTFact, 1.0 + 0.1 * maxDeltaTFact), 1.2);
    return std::min(deltaTFact * dt, max_delta_t);
}

// lduMatrix::solver's L1 residual control per component of a three-component Jacobi solve (both solve_vec3): h = {sum |b - A x| x 3, the normalisation sums x 3} of pass
// `pass`; the first pass fixes the normalisation and the initial residuals.  Converged when every component is below tol, or below rel_tol times its initial residual
inline bool vec3_converged(int pass, const double (&h)[6], double tol, double rel_tol, double (&norm)[3], double (&res0)[3]) {
    if (pass == 0) for (int q = 0; q < 3; ++q) { norm[q] = h[3 + q] + 1e-20; res0[q] = h[q] / norm[q]; }
    bool conv = true;
    for (int q = 0; q < 3; ++q) { const double res = h[q] / norm[q]; conv = conv && (res < tol || (rel_tol > 0 && res < rel_tol * res0[q])); }
    return conv;
}

// nutWallFunction::yPlusLam [OF-6 nutWallFunctionFvPatchScalarField.C]: ten fixed-point sweeps of y+ = ln(E y+) / kappa from 11 (both solvers' wall functions)
inline double wall_yplus_lam(double kappa, double E) {
    double ypl = 11.0;
    for (int it = 0; it < 10; ++it) ypl = std::log(std::max(E * ypl, 1.0)) / kappa;
    return ypl;
}

}  // namespace fy
