// Device-side helpers that more than one kernel source needs (fv_kernels.hip in both its builds, fv_linalg_kernels.hip, ldu_kernels.hip,
// ldu_amg.hip, the particle_*.hip sources).  Everything here is inlined into its caller: including this header adds no symbol to an object.
// Launch plumbing only (block order, reductions, the launch check); the physics that fv_kernels.hip (both builds) and ldu_kernels.hip share is in fv_closures.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace fy {
namespace {

// XCD-aware block order (guide T1): block b runs on XCD b % 8; give every XCD one contiguous z-slab of the grid so that the
// y/z-neighbour re-reads of a stencil hit that XCD's own L2.  Pure speed: any mapping is correct.
__device__ __forceinline__ int swz_block(int bid, int nblk) {
    if (nblk % 8) return bid;
    return (bid % 8) * (nblk / 8) + bid / 8;
}

// ------------------------------------------------------------------------------------------------ block reductions (256 threads)
// one partial per block and slot: slot q's partials start at q * stride, the block's own is number lb.  The defaults are the launch's
// own (block index, grid size); a sweep whose blocks run in another order, or over a window of the range, passes its logical values.
// I = the type the index partials[q * stride + lb] is formed in: the general-mesh kernels (ldu_kernels.hip) hand over blockIdx.x and
// gridDim.x as they are, unsigned, which is the arithmetic they were compiled and measured with
template <int N, class I = int>
__device__ __forceinline__ void block_reduce_store(double (&v)[N], const int (&is_max)[N], double* partials, I lb = -1, I stride = 0) {
    if (lb < 0) lb = (I)blockIdx.x;
    if (stride <= 0) stride = (I)gridDim.x;                // partials of slot q start at q * (blocks of the WHOLE sweep)
    __shared__ double sh[4][N];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        double x = v[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double y = __shfl_down(x, o, 64);
            x = is_max[q] ? fmax(x, y) : x + y;
        }
        if (lane == 0) sh[wv][q] = x;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const int q = threadIdx.x;
        double x = sh[0][q];
        for (int w = 1; w < 4; ++w) x = is_max[q] ? fmax(x, sh[w][q]) : x + sh[w][q];
        partials[(size_t)q * stride + lb] = x;
    }
}

}  // namespace
}  // namespace fy

// Reducing kernels: one thread per cell (like the plain stencil kernels -- a 1024-block grid-stride loop reached only ~3 TB/s where
// the one-thread-per-cell smoother reaches 5.4), XCD-aware block order, one partial per block; k_reduce_finalize folds the
// red_blocks(n) partials of a slot in a fixed order, so results are reproducible from run to run.
#define FY_RED_LOOP(t, n) const int t = swz_block(blockIdx.x, gridDim.x) * 256 + (int)threadIdx.x; if (t < (n))

// after a launcher's hipLaunchKernelGGL calls (inside namespace fy, in a function that returns an FY_* code)
#define FY_LAUNCH_CHECK()                                                                                     \
    do {                                                                                                      \
        hipError_t _e = hipGetLastError();                                                                    \
        if (_e != hipSuccess) return fail(FY_ERR_HIP, "kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

namespace fy {
namespace {

// The launcher most kernels have: one thread per item, nothing to do for none, the launch check.  `at` is the caller's stream; it also takes down
// where the launcher stands, so that a failed launch is reported with the launcher's file and line as FY_LAUNCH_CHECK reports it.
struct LaunchAt {
    hipStream_t s; const char* file; int line;
    LaunchAt(hipStream_t s_, const char* f = __builtin_FILE(), int l = __builtin_LINE()) : s(s_), file(f), line(l) {}
};
template <class Kernel, class... Args>
int launch_n(LaunchAt at, Kernel kernel, int64_t n, int block, Args... args) {
    if (n <= 0) return FY_OK;
    hipLaunchKernelGGL(kernel, dim3(div_up(n, block)), dim3(block), 0, at.s, args...);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FY_ERR_HIP, "kernel launch failed: %s (%s:%d)", hipGetErrorString(e), at.file, at.line);
    return FY_OK;
}

}  // namespace
}  // namespace fy
