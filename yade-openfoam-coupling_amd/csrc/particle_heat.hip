// Particle half, the heat exchange (the five sources: particle_bin.hip).
#include "particle_kernels.hpp"

#include "common.hpp"
#include "device_util.hpp"
#include "scatter_table.hpp"
#include "stencil_ring.hpp"

namespace fy {
namespace {

// ------------------------------------------------------------------------------------------------ particle-fluid heat exchange (fy_thermal_desc)
// Not in the reference.  Pass A (k_heat_coeff_*): per particle the Nusselt number from the stencil the force pass used -- eps = sum w alpha_c and u_f = sum w U_c from
// the SAME cell records, Re = small + |u_f - v_p| d / nu --, hA = Nu kappa pi d kept per particle (wire order), and the scatter Sp_c += w hA, Su_c += w hA Tp.
// Pass B (k_heat_flux_*), after the fluid's T equation was solved with Sp implicit: q = hA (sum w T_c - Tp).  With sum_c w = 1 the particles receive exactly what the
// cells lose.  The scatter has the force pass's (workgroup, cell) pattern -- same workgroup size, same table -- so it goes through the same LDS table and, where the
// momentum back-scatter's bucket capacities are at hand, through the tile buckets (two of an entry's four value slots); what finds no room goes out as global atomics.
// kOwn (fy_thermal_desc.particle_cp > 0): the library integrates Tp, backward Euler for the particle-fluid pair with no extra solve.  With m c = rho_p c_pp (4/3) pi r^3
// and r_p = dt hA / (m c), pass A scatters and keeps hA' = hA / (1 + r_p) in hA's place; pass B forms q = hA' (sum w T_c - Tp) and writes Tp += dt q / (m c) in place --
// eliminating the new Tp, m c (Tp' - Tp) = dt hA (T_f' - Tp').  A particle nobody located keeps its Tp.  kOwn = false is the code as it was: the caller owns Tp.
__device__ __forceinline__ double nusselt(const HeatParams& hp, double eps, double Re) {
    if (hp.law == FY_NUSSELT_GUNN) {
        const double Res = eps * Re;
        return (7.0 - 10.0 * eps + 5.0 * (eps * eps)) * (1.0 + 0.7 * pow(Res, 0.2) * hp.pr13) + (1.33 - 2.4 * eps + 1.2 * (eps * eps)) * pow(Res, 0.7) * hp.pr13;
    }
    return 2.0 + 0.6 * sqrt(Re) * hp.pr13;
}

// m_p c_pp of a particle of radius r
__device__ __forceinline__ double heat_capacity(double rho_cpp, double r) { return rho_cpp * (((4.0 / 3.0) * M_PI) * ((r * r) * r)); }
// hA' = hA / (1 + dt hA / (m c))
__device__ __forceinline__ double damped_hA(const HeatParams& hp, double hA, double r) { return hA / (1.0 + (hp.dt * hA) / heat_capacity(hp.rho_cpp, r)); }
// pass B's Tp argument: read-only where the caller owns the temperatures, updated in place where the library does
template <bool kOwn> struct TpArg { typedef const double* __restrict__ type; };
template <> struct TpArg<true> { typedef double* type; };

// one workgroup per tile, the tile's only writer: the bucket's two sums per entry into Sp / Su; the tile's demand counter goes back to zero (the buckets are the
// momentum back-scatter's, which counts its own demand from zero in the next step)
__global__ __launch_bounds__(256) void k_heat_tile_reduce(TileBuckets tb, double* __restrict__ Sp, double* __restrict__ Su) {
    __shared__ double acc[kTileCells * 2];
    const uint32_t tile = blockIdx.x;
    uint32_t cnt = tb.fill[tile];
    const uint32_t cap = tb.cap[tile];
    if (cnt > cap) cnt = cap;
    __syncthreads();                                        // (every thread has read the counter)
    if (threadIdx.x == 0) tb.fill[tile] = 0;
    if (cnt == 0) return;
    tile_bucket_sum<2>(tb, tile, cnt, acc);
    const TilePos tp = tile_pos(tb.tg, tile);
    for (int l = threadIdx.x; l < kTileCells; l += 256) {
        const TileCell tc = tile_cell(tp, l);
        if (!tc.inside(tb.tg)) continue;
        const double a0 = acc[agg_at<kTileCells>(l, 0)], a1 = acc[agg_at<kTileCells>(l, 1)];
        if (a0 == 0.0 && a1 == 0.0) continue;
        const size_t c = tc.index(tb.tg);
        Sp[c] += a0; Su[c] += a1;
    }
}

// the force pass's workgroup and table size (particle_force.hip: kForceThreads, kForceLog2), so that a workgroup's entries per tile are what the momentum
// back-scatter's bucket capacities were sized for
constexpr int kHeatThreads = 512, kHeatLog2 = 10;
template <bool kOwn>
__global__ __launch_bounds__(kHeatThreads) void k_heat_coeff_gaussian(ParticleSoA p, int64_t n, HeatParams hp, CellWindow cw, const double* __restrict__ R,
                                                                      const double* __restrict__ Tp, double* __restrict__ hA_out, double* __restrict__ Sp,
                                                                      double* __restrict__ Su, TileBuckets tb) {
    constexpr int kSlots = 1 << kHeatLog2;
    __shared__ uint32_t keys[kSlots];
    __shared__ double vals[kSlots * 2];
    __shared__ TileMapLds tmap;
    table_clear<kSlots, kHeatThreads, 2>(keys, vals);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kHeatThreads + threadIdx.x;
    if (i < n) {
        const StencilSpan sp = stencil_span(p.chain_len[i]);  // oldest first, the force pass's order
        const int k = sp.k, first = sp.first;
        const int32_t orig = p.orig[i];
        if (k == 0) {
            hA_out[orig] = 0.0;                               // nobody located it: no deposit, q = 0
        } else {
            double eps = 0.0, ux = 0.0, uy = 0.0, uz = 0.0;
            for (int t = 0; t < k; ++t) {
                const size_t slot = stencil_slot(p, i, first + t);
                const int64_t cl = (int64_t)p.ids[slot] - cw.base;
                if (cl < 0 || cl >= cw.n_field) continue;
                const double w = p.w[slot];
                const double2* r = reinterpret_cast<const double2*>(R + kRecDoubles * (size_t)cl);
                const double2 r0 = r[0], r1 = r[1];
                ux += (r0.x * w); uy += (r0.y * w); uz += (r1.x * w);
                eps += (r1.y * w);
            }
            const double dia = 2 * p.rad[i];
            const double rx = ux - p.vx[i], ry = uy - p.vy[i], rz = uz - p.vz[i];
            const double Re = hp.small + ((sqrt(rx * rx + ry * ry + rz * rz) * dia) / hp.nu);
            double hA = ((nusselt(hp, eps, Re) * hp.kappa) * M_PI) * dia;
            if (kOwn) hA = damped_hA(hp, hA, p.rad[i]);
            const double tp = Tp ? Tp[orig] : hp.tp_uniform;
            hA_out[orig] = hA;
            for (int t = 0; t < k; ++t) {
                const size_t slot = stencil_slot(p, i, first + t);
                const int64_t cl = (int64_t)p.ids[slot] - cw.base;
                if (cl < 0 || cl >= cw.n_field) continue;
                const int32_t c = (int32_t)cl;
                const double c0 = p.w[slot] * hA, c1 = c0 * tp;
                const int h = agg_slot<kHeatLog2>(keys, (uint32_t)c);
                if (h >= 0) { lds_add_f64(&vals[agg_at<kSlots>(h, 0)], c0); lds_add_f64(&vals[agg_at<kSlots>(h, 1)], c1); }
                else { atomic_add_f64(&Sp[c], c0); atomic_add_f64(&Su[c], c1); }
            }
        }
    }
    __syncthreads();
    flush_table<kSlots, kHeatThreads, 2>(keys, vals, tmap, tb, Sp, Su, nullptr);
}

template <bool kOwn>
__global__ __launch_bounds__(256) void k_heat_flux_gaussian(ParticleSoA p, int64_t n, CellWindow cw, const double* __restrict__ T, double tp_uniform,
                                                            typename TpArg<kOwn>::type Tp, const double* __restrict__ hA, double* __restrict__ q_out, HeatParams hp) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const StencilSpan sp = stencil_span(p.chain_len[i]);
    const int k = sp.k, first = sp.first;
    const int32_t orig = p.orig[i];
    double tf = 0.0;
    for (int t = 0; t < k; ++t) {
        const size_t slot = stencil_slot(p, i, first + t);
        const int64_t cl = (int64_t)p.ids[slot] - cw.base;
        if (cl < 0 || cl >= cw.n_field) continue;
        tf += (T[cl] * p.w[slot]);
    }
    if constexpr (!kOwn) {
        q_out[orig] = k == 0 ? 0.0 : hA[orig] * (tf - (Tp ? Tp[orig] : tp_uniform));
    } else {
        if (k == 0) { q_out[orig] = 0.0; return; }           // keeps its Tp
        const double tp = Tp[orig];
        const double q = hA[orig] * (tf - tp);
        q_out[orig] = q;
        Tp[orig] = tp + (hp.dt * q) / heat_capacity(hp.rho_cpp, p.rad[i]);
    }
}

// point-force mode: the containing cell (k_point_force's incell, -1: not found), w = 1, eps = 1, the cell's U
template <bool kOwn>
__global__ __launch_bounds__(256) void k_heat_coeff_point(const double* __restrict__ rec, int64_t n, const int32_t* __restrict__ incell, HeatParams hp, CellWindow cw,
                                                          const double* __restrict__ U, const double* __restrict__ Tp, double* __restrict__ hA_out,
                                                          double* __restrict__ Sp, double* __restrict__ Su) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t cl = incell[i] < 0 ? -1 : (int64_t)incell[i] - cw.base;
    if (cl < 0 || cl >= cw.n_field) { hA_out[i] = 0.0; return; }
    const double* r = rec + 10 * i;
    const double* u = U + 3 * (size_t)cl;
    const double dia = 2 * r[9];
    const double rx = u[0] - r[3], ry = u[1] - r[4], rz = u[2] - r[5];
    const double Re = hp.small + ((sqrt(rx * rx + ry * ry + rz * rz) * dia) / hp.nu);
    double hA = ((nusselt(hp, 1.0, Re) * hp.kappa) * M_PI) * dia;
    if (kOwn) hA = damped_hA(hp, hA, r[9]);
    hA_out[i] = hA;
    atomic_add_f64(&Sp[cl], hA);
    atomic_add_f64(&Su[cl], hA * (Tp ? Tp[i] : hp.tp_uniform));
}

template <bool kOwn>
__global__ __launch_bounds__(256) void k_heat_flux_point(int64_t n, const int32_t* __restrict__ incell, CellWindow cw, const double* __restrict__ T, double tp_uniform,
                                                         typename TpArg<kOwn>::type Tp, const double* __restrict__ hA, double* __restrict__ q_out, const double* __restrict__ rec,
                                                         HeatParams hp) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t cl = incell[i] < 0 ? -1 : (int64_t)incell[i] - cw.base;
    if constexpr (!kOwn) {
        q_out[i] = (cl < 0 || cl >= cw.n_field) ? 0.0 : hA[i] * (T[cl] - (Tp ? Tp[i] : tp_uniform));
    } else {
        if (cl < 0 || cl >= cw.n_field) { q_out[i] = 0.0; return; }      // keeps its Tp
        const double tp = Tp[i];
        const double q = hA[i] * (T[cl] - tp);
        q_out[i] = q;
        Tp[i] = tp + (hp.dt * q) / heat_capacity(hp.rho_cpp, rec[10 * i + 9]);
    }
}

}  // namespace

int launch_heat_coeff_gaussian(hipStream_t s, ParticleSoA p, int64_t n, HeatParams hp, CellWindow cw, const double* R, const double* Tp, double* hA, double* Sp, double* Su,
                               TileBuckets tb) {
    if (n <= 0) return FY_OK;
    if (hp.rho_cpp > 0) FY_TRY(launch_n(s, k_heat_coeff_gaussian<true>, n, kHeatThreads, p, n, hp, cw, R, Tp, hA, Sp, Su, tb));
    else FY_TRY(launch_n(s, k_heat_coeff_gaussian<false>, n, kHeatThreads, p, n, hp, cw, R, Tp, hA, Sp, Su, tb));
    if (tb.cell) {                           // (the solver always hands buckets over; without them the flush above went out as atomics)
        hipLaunchKernelGGL(k_heat_tile_reduce, dim3((unsigned)tb.tg.n_tiles()), dim3(256), 0, s, tb, Sp, Su);
        FY_LAUNCH_CHECK();
    }
    return FY_OK;
}

int launch_heat_flux_gaussian(hipStream_t s, ParticleSoA p, int64_t n, CellWindow cw, const double* T, HeatParams hp, double* Tp, const double* hA, double* q) {
    if (hp.rho_cpp > 0) return launch_n(s, k_heat_flux_gaussian<true>, n, 256, p, n, cw, T, hp.tp_uniform, Tp, hA, q, hp);
    return launch_n(s, k_heat_flux_gaussian<false>, n, 256, p, n, cw, T, hp.tp_uniform, (const double*)Tp, hA, q, hp);
}

int launch_heat_coeff_point(hipStream_t s, const double* rec, int64_t n, const int32_t* incell, HeatParams hp, CellWindow cw, const double* U, const double* Tp, double* hA,
                            double* Sp, double* Su) {
    if (hp.rho_cpp > 0) return launch_n(s, k_heat_coeff_point<true>, n, 256, rec, n, incell, hp, cw, U, Tp, hA, Sp, Su);
    return launch_n(s, k_heat_coeff_point<false>, n, 256, rec, n, incell, hp, cw, U, Tp, hA, Sp, Su);
}

int launch_heat_flux_point(hipStream_t s, const double* rec, int64_t n, const int32_t* incell, CellWindow cw, const double* T, HeatParams hp, double* Tp, const double* hA, double* q) {
    if (hp.rho_cpp > 0) return launch_n(s, k_heat_flux_point<true>, n, 256, n, incell, cw, T, hp.tp_uniform, Tp, hA, q, rec, hp);
    return launch_n(s, k_heat_flux_point<false>, n, 256, n, incell, cw, T, hp.tp_uniform, (const double*)Tp, hA, q, rec, hp);
}

}  // namespace fy

