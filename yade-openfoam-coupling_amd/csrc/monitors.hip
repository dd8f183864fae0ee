// The geometry-free kernels of fy::Monitors (monitors.hpp): k_monitor_cells, the one sweep over the cells for all volume objects, and k_monitor_finalize, the fold of
// the block partials into a row of every object's ring.  (The face kernels are the solvers': k_monitor_faces in fv_kernels.hip, k_ldu_monitor_faces in ldu_kernels.hip.)
// Built with -ffp-contract=off like every kernel here: each product and each sum below is one IEEE operation, which is what the tests' bound counts.  FP64, no atomics:
// a partial is a fixed tree over the block's lanes, a value a fixed tree over the partials, so a sample has the same bits from run to run.
#include "monitors.hpp"

#include "device_util.hpp"

namespace fy {

namespace {

// A block of 256 lanes takes a tile of 256 kMonCellsPerLane cells, lane t the cells t, t + 256, ... of it (coalesced).  The cells' volumes and weights are read once and
// kept in registers, then every source component once; a lane adds its cells' terms in ascending order, and each component leaves the block as its five partials.  The
// wave and LDS fold costs some sixty cross-lane moves per component whatever the tile holds, which is why a lane takes several cells.  The loop's trip count and the
// table are uniform (kernel arguments), so the barriers inside mon_block_reduce_store are reached by every lane.
__global__ __launch_bounds__(256) void k_monitor_cells(const MonCellTable t, int n, double* __restrict__ partials) {
    const int c0 = blockIdx.x * (256 * kMonCellsPerLane) + threadIdx.x;
    double m[kMonCellsPerLane], w[kMonCellsPerLane];
#pragma unroll
    for (int u = 0; u < kMonCellsPerLane; ++u) {
        const int c = c0 + u * 256;
        m[u] = 0.0; w[u] = 0.0;
        if (c < n) {
            m[u] = t.V ? t.V[c] : t.V0;
            if (t.w) w[u] = t.w[c] * m[u];
        }
    }
    for (int j = 0; j < t.n; ++j) {
        const MonCellSrc s = t.s[j];
        double v[kMonKinds];
        mon_terms(false, 0.0, 0.0, 0.0, v);
#pragma unroll
        for (int u = 0; u < kMonCellsPerLane; ++u) {
            const int c = c0 + u * 256;
            if (c < n) {
                const double x = s.p ? s.p[(size_t)c * s.stride + s.off] : 1.0;
                v[MK_SUM] = v[MK_SUM] + x;
                v[MK_MSUM] = v[MK_MSUM] + x * m[u];
                v[MK_WSUM] = v[MK_WSUM] + w[u] * x;
                v[MK_MIN] = fmin(v[MK_MIN], x);
                v[MK_MAX] = fmax(v[MK_MAX], x);
            }
        }
        mon_block_reduce_store(v, partials, j * kMonKinds, (int)gridDim.x, (int)blockIdx.x);
    }
}

// the partials of one slot folded by the workgroup in a fixed order: 256 lanes stride over them, a shuffle tree per wave, the four waves in LDS.  op 0 sum | 1 min | 2 max
__device__ __forceinline__ double mon_fold(const double* __restrict__ p, int nblk, int op, double (&sh)[4]) {
    double x = op == 1 ? INFINITY : op == 2 ? -INFINITY : 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) {
        const double y = p[b];
        x = op == 1 ? fmin(x, y) : op == 2 ? fmax(x, y) : x + y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double y = __shfl_down(x, o, 64);
        x = op == 1 ? fmin(x, y) : op == 2 ? fmax(x, y) : x + y;
    }
    __syncthreads();                                     // (the previous fold's readers are done with sh)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    double r = sh[0];
    for (int w = 1; w < 4; ++w) r = op == 1 ? fmin(r, sh[w]) : op == 2 ? fmax(r, sh[w]) : r + sh[w];
    return r;
}

// one workgroup per value: numerator, denominator (where the operation has one), the division, the store into the object's ring; the workgroup of an object's first
// value also stores the row's time.  Objects that are not due this step (MonRings::due) leave at once
__global__ __launch_bounds__(256) void k_monitor_finalize(const MonOut* __restrict__ outs, const double* __restrict__ pc, int nblk_c, const double* __restrict__ pf, int nblk_f,
                                                          const MonRings r, double time) {
    __shared__ double sh[4];
    const MonOut e = outs[blockIdx.x];
    if (!(r.due >> e.object & 1u)) return;
    const double* p = e.src ? pf : pc;
    const int nblk = e.src ? nblk_f : nblk_c;
    double v = mon_fold(p + (size_t)e.num * nblk, nblk, e.op, sh);
    if (e.den >= 0) v = v / mon_fold(p + (size_t)e.den * nblk, nblk, 0, sh);
    if (threadIdx.x == 0) {
        double* row = r.ring[e.object] + (size_t)r.row[e.object] * r.width[e.object];
        row[1 + e.col] = v;
        if (e.col == 0) row[0] = time;
    }
}

}  // namespace

int launch_monitor_cells(hipStream_t s, const MonCellTable& t, int n_cells, double* partials) {
    if (n_cells <= 0 || t.n <= 0) return FY_OK;
    hipLaunchKernelGGL(k_monitor_cells, dim3(mon_cell_blocks(n_cells)), dim3(256), 0, s, t, n_cells, partials);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_monitor_finalize(hipStream_t s, const MonOut* outs, int n_outs, const double* pc, int nblk_c, const double* pf, int nblk_f, const MonRings& r, double time) {
    if (n_outs <= 0) return FY_OK;
    hipLaunchKernelGGL(k_monitor_finalize, dim3(n_outs), dim3(256), 0, s, outs, pc, nblk_c, pf, nblk_f, r, time);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

}  // namespace fy
