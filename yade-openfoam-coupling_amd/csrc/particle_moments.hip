// Particle half, the solid-phase statistics (the other sources: particle_bin.hip).
#include "particle_kernels.hpp"

#include "common.hpp"
#include "device_util.hpp"
#include "scatter_table.hpp"
#include "stencil_ring.hpp"

namespace fy {
namespace {

// ------------------------------------------------------------------------------------------------ solid-phase statistics (fy_solver_set_solid_statistics)
// Not in the reference.  Per cell c, over every located particle of every batch of the step and every slot of its stencil with weight w, eight sums (SolidMoments):
//   s0 = sum w          s1 = sum w Vp       s2..s4 = sum (w Vp) v        s5 = sum (w Vp) |v|^2       s6 = sum w d^2       s7 = sum (w Vp) Tp
// with d = 2 r, Vp = pi d^3 / 6 as the deposit forms it (particle_locate.hip: pVol) and |v|^2 = (vx vx + vy vy) + vz vz.  The scatter has the force pass's
// (workgroup, cell) pattern, so it is k_heat_coeff_gaussian's once more: the LDS table, flush_table into the momentum back-scatter's tile buckets, a one-writer tile
// reduce that leaves the demand counters at zero, global FP64 atomics where there are no tiles or no room.  A bucket entry carries four sums, so the kernel is
// launched twice: HALF 0 scatters {s0 | s1, s5, s6}, HALF 1 {s7 | s2, s3, s4} -- each as flush_table's (dst0[c] | dstN[3 c + 0..2]) of its own half of SolidMoments.
// k_solid_stats_cells then forms the fields per cell; every bracket below is one IEEE operation.
struct MomentTerms { double c0, c1, c2, c3; };
template <int HALF>
__device__ __forceinline__ MomentTerms moment_terms(double w, double dia, double vx, double vy, double vz, double tp) {
    const double pVol = M_PI * cube3(dia) / 6.0;
    const double wv = w * pVol;
    if (HALF == 0) return MomentTerms{w, wv, wv * ((vx * vx + vy * vy) + vz * vz), w * (dia * dia)};
    return MomentTerms{wv * tp, wv * vx, wv * vy, wv * vz};
}

// the force pass's workgroup and table size (particle_force.hip: kForceThreads, kForceLog2; particle_heat.hip: kHeatThreads, kHeatLog2), so that a workgroup's entries
// per tile are what the momentum back-scatter's bucket capacities of this step were sized for
constexpr int kMomThreads = 512, kMomLog2 = 10;
template <int HALF>
__global__ __launch_bounds__(kMomThreads) void k_moments_gaussian(ParticleSoA p, int64_t n, CellWindow cw, const double* __restrict__ Tp, double tp_uniform,
                                                                  double* __restrict__ dst0, double* __restrict__ dst3, TileBuckets tb) {
    constexpr int kSlots = 1 << kMomLog2;
    __shared__ uint32_t keys[kSlots];
    __shared__ double vals[kSlots * 4];
    __shared__ TileMapLds tmap;
    table_clear<kSlots, kMomThreads, 4>(keys, vals);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kMomThreads + threadIdx.x;
    if (i < n) {
        const StencilSpan sp = stencil_span(p.chain_len[i]);  // oldest first, the force pass's order
        const int k = sp.k, first = sp.first;
        if (k > 0) {
            const double dia = 2 * p.rad[i];
            const double vx = p.vx[i], vy = p.vy[i], vz = p.vz[i];
            const double tp = HALF == 0 ? 0.0 : (Tp ? Tp[p.orig[i]] : tp_uniform);
            for (int t = 0; t < k; ++t) {
                const size_t slot = stencil_slot(p, i, first + t);
                const int64_t cl = (int64_t)p.ids[slot] - cw.base;
                if (cl < 0 || cl >= cw.n_field) continue;
                const int32_t c = (int32_t)cl;
                const MomentTerms m = moment_terms<HALF>(p.w[slot], dia, vx, vy, vz, tp);
                const int h = agg_slot<kMomLog2>(keys, (uint32_t)c);
                if (h >= 0) {
                    lds_add_f64(&vals[agg_at<kSlots>(h, 0)], m.c0); lds_add_f64(&vals[agg_at<kSlots>(h, 1)], m.c1);
                    lds_add_f64(&vals[agg_at<kSlots>(h, 2)], m.c2); lds_add_f64(&vals[agg_at<kSlots>(h, 3)], m.c3);
                } else {                                          // table crowded: nothing is dropped
                    atomic_add_f64(&dst0[c], m.c0);
                    atomic_add_f64(&dst3[3 * (size_t)c + 0], m.c1); atomic_add_f64(&dst3[3 * (size_t)c + 1], m.c2); atomic_add_f64(&dst3[3 * (size_t)c + 2], m.c3);
                }
            }
        }
    }
    __syncthreads();
    flush_table<kSlots, kMomThreads, 4>(keys, vals, tmap, tb, dst0, dst3, nullptr);
}

// one workgroup per tile, the tile's only writer: the bucket's four sums per entry into (dst0 | dst3); the tile's demand counter goes back to zero (the buckets are the
// momentum back-scatter's, which counts its own demand from zero in the next step).  k_heat_tile_reduce with four sums
__global__ __launch_bounds__(256) void k_moments_tile_reduce(TileBuckets tb, double* __restrict__ dst0, double* __restrict__ dst3) {
    __shared__ double acc[kTileCells * 4];
    const uint32_t tile = blockIdx.x;
    uint32_t cnt = tb.fill[tile];
    const uint32_t cap = tb.cap[tile];
    if (cnt > cap) cnt = cap;
    __syncthreads();                                        // (every thread has read the counter)
    if (threadIdx.x == 0) tb.fill[tile] = 0;
    if (cnt == 0) return;
    tile_bucket_sum<4>(tb, tile, cnt, acc);
    const TilePos tp = tile_pos(tb.tg, tile);
    for (int l = threadIdx.x; l < kTileCells; l += 256) {
        const TileCell tc = tile_cell(tp, l);
        if (!tc.inside(tb.tg)) continue;
        const double a0 = acc[agg_at<kTileCells>(l, 0)], a1 = acc[agg_at<kTileCells>(l, 1)], a2 = acc[agg_at<kTileCells>(l, 2)], a3 = acc[agg_at<kTileCells>(l, 3)];
        if (a0 == 0.0 && a1 == 0.0 && a2 == 0.0 && a3 == 0.0) continue;
        const size_t c = tc.index(tb.tg);
        dst0[c] += a0;
        double* d = dst3 + 3 * c;
        const double d0 = d[0] + a1, d1 = d[1] + a2, d2 = d[2] + a3;
        d[0] = d0; d[1] = d1; d[2] = d2;
    }
}

// point-force mode: the containing cell (k_point_force's incell, -1: not found), w = 1
__global__ __launch_bounds__(256) void k_moments_point(const double* __restrict__ rec, int64_t n, const int32_t* __restrict__ incell, CellWindow cw,
                                                       const double* __restrict__ Tp, double tp_uniform, SolidMoments m) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t cl = incell[i] < 0 ? -1 : (int64_t)incell[i] - cw.base;
    if (cl < 0 || cl >= cw.n_field) return;
    const double* r = rec + 10 * i;
    const double dia = 2 * r[9];
    const MomentTerms a = moment_terms<0>(1.0, dia, r[3], r[4], r[5], 0.0);
    const MomentTerms b = moment_terms<1>(1.0, dia, r[3], r[4], r[5], Tp ? Tp[i] : tp_uniform);
    atomic_add_f64(&m.a0[cl], a.c0);
    atomic_add_f64(&m.a3[3 * (size_t)cl + 0], a.c1); atomic_add_f64(&m.a3[3 * (size_t)cl + 1], a.c2); atomic_add_f64(&m.a3[3 * (size_t)cl + 2], a.c3);
    atomic_add_f64(&m.b0[cl], b.c0);
    atomic_add_f64(&m.b3[3 * (size_t)cl + 0], b.c1); atomic_add_f64(&m.b3[3 * (size_t)cl + 1], b.c2); atomic_add_f64(&m.b3[3 * (size_t)cl + 2], b.c3);
}

// the fields of one cell from its eight sums and its volume
__global__ __launch_bounds__(256) void k_solid_stats_cells(int64_t n, SolidMoments m, const double* __restrict__ vol, SolidFields f) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const double s1 = m.a3[3 * c + 0];
    double nP = 0.0, sf = 0.0, ux = 0.0, uy = 0.0, uz = 0.0, gT = 0.0, d32 = 0.0, tP = 0.0;
    if (s1 != 0.0) {
        const double V = vol[c];
        const double s0 = m.a0[c], s5 = m.a3[3 * c + 1], s6 = m.a3[3 * c + 2];
        nP = s0 / V;
        sf = s1 / V;
        ux = m.b3[3 * c + 0] / s1; uy = m.b3[3 * c + 1] / s1; uz = m.b3[3 * c + 2] / s1;
        const double th = ((s5 / s1) - ((ux * ux + uy * uy) + uz * uz)) / 3;
        gT = th > 0.0 ? th : 0.0;
        d32 = ((6.0 / M_PI) * s1) / s6;
        tP = m.b0[c] / s1;
    }
    f.nParticle[c] = nP; f.solidFraction[c] = sf;
    f.uSolid[3 * c + 0] = ux; f.uSolid[3 * c + 1] = uy; f.uSolid[3 * c + 2] = uz;
    f.granularTemperature[c] = gT; f.dSauter[c] = d32;
    if (f.TParticle) f.TParticle[c] = tP;
}

// "solidMoments" [n][8] for the field read-out: s0 .. s7 of a cell side by side
__global__ __launch_bounds__(256) void k_moments_interleave(int64_t n, SolidMoments m, double* __restrict__ out) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    double* o = out + 8 * c;
    o[0] = m.a0[c]; o[1] = m.a3[3 * c + 0];
    o[2] = m.b3[3 * c + 0]; o[3] = m.b3[3 * c + 1]; o[4] = m.b3[3 * c + 2];
    o[5] = m.a3[3 * c + 1]; o[6] = m.a3[3 * c + 2]; o[7] = m.b0[c];
}

}  // namespace

int launch_moments_gaussian(hipStream_t s, ParticleSoA p, int64_t n, CellWindow cw, const double* Tp, double tp_uniform, SolidMoments m, TileBuckets tb) {
    if (n <= 0) return FY_OK;
    FY_TRY(launch_n(s, k_moments_gaussian<0>, n, kMomThreads, p, n, cw, Tp, tp_uniform, m.a0, m.a3, tb));
    if (tb.cell) { hipLaunchKernelGGL(k_moments_tile_reduce, dim3((unsigned)tb.tg.n_tiles()), dim3(256), 0, s, tb, m.a0, m.a3); FY_LAUNCH_CHECK(); }
    FY_TRY(launch_n(s, k_moments_gaussian<1>, n, kMomThreads, p, n, cw, Tp, tp_uniform, m.b0, m.b3, tb));
    if (tb.cell) { hipLaunchKernelGGL(k_moments_tile_reduce, dim3((unsigned)tb.tg.n_tiles()), dim3(256), 0, s, tb, m.b0, m.b3); FY_LAUNCH_CHECK(); }
    return FY_OK;
}

int launch_moments_point(hipStream_t s, const double* rec, int64_t n, const int32_t* incell, CellWindow cw, const double* Tp, double tp_uniform, SolidMoments m) {
    return launch_n(s, k_moments_point, n, 256, rec, n, incell, cw, Tp, tp_uniform, m);
}

int launch_solid_stats_cells(hipStream_t s, int64_t n_cells, SolidMoments m, const double* vol, SolidFields f) {
    return launch_n(s, k_solid_stats_cells, n_cells, 256, n_cells, m, vol, f);
}

int launch_moments_interleave(hipStream_t s, int64_t n_cells, SolidMoments m, double* out) {
    return launch_n(s, k_moments_interleave, n_cells, 256, n_cells, m, out);
}

}  // namespace fy
