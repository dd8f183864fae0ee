// Particle half, between the scatters and the cells (the five sources: particle_bin.hip): the tile buckets' capacities, their reduction into the cell
// arrays, and what finishes a cell once its sums are complete -- setCellVolFraction and the fold of the momentum sources -- in the reduction or on its own.
#include "particle_kernels.hpp"

#include "common.hpp"
#include "device_util.hpp"
#include "scatter_table.hpp"

namespace fy {
namespace {

// k_tile_caps: block b serves bucket set b.  cap[t] = demand x 1.25 + 128, offsets by an exclusive scan, clamped to the pool; demand reset
__global__ __launch_bounds__(1024) void k_tile_caps(TileBuckets s0, TileBuckets s1, unsigned int* __restrict__ also_zero) {
    if (also_zero && blockIdx.x == 0 && threadIdx.x == 0) { also_zero[1] = also_zero[0]; also_zero[0] = 0u; }      // (slot 1 keeps the last pass's count for the diagnostics)
    const TileBuckets tb = blockIdx.x == 0 ? s0 : s1;
    if (!tb.cell) return;
    const int n_tiles = tb.tg.n_tiles();
    __shared__ uint32_t wave_tot[16];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int base = 0; base < n_tiles; base += 1024) {
        const int t = base + (int)threadIdx.x;
        uint32_t want = 0;
        if (t < n_tiles) {
            const uint32_t need = tb.fill[t];
            want = need ? ((need + (need >> 2) + 128u + 7u) & ~7u) : 0u;      // a tile nobody wrote to last step keeps no room (its first entries go out as atomics)
            tb.fill[t] = 0;
        }
        uint32_t inc = want;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(inc, d, 64);
            if (lane >= d) inc += y;
        }
        if (lane == 63) wave_tot[wv] = inc;
        __syncthreads();
        uint32_t woff = carry;
        for (int q = 0; q < wv; ++q) woff += wave_tot[q];
        uint32_t start = woff + inc - want;
        if (t < n_tiles) {
            // the pool is finite: a tile that no longer fits gets what is left (its excess goes out as atomics)
            if (start > tb.pool) start = tb.pool;
            const uint32_t room = tb.pool - start;
            tb.off[t] = start;
            tb.cap[t] = want < room ? want : room;
        }
        __syncthreads();
        if (threadIdx.x == 1023) carry = woff + inc;
        __syncthreads();
    }
}

// One workgroup per tile of 8 x 8 x 8 cells: the tile's bucket is summed into a dense LDS accumulator (ds_add_f64: ~37 x the global
// atomics' rate), then the tile goes to the cell arrays with plain read-modify-writes -- this workgroup is the tile's only writer.
// FINISH 0: that is all (z-slabs: the reverse-halo sums of the neighbours come in before the cells are finished).
// FINISH 1 (single domain, void-fraction deposit): the cell's sums are complete here, so setCellVolFraction (k_finalize_cells) happens in the
//          same pass -- no round trip of the accumulators through memory, no second sweep over the touched flags.
// FINISH 2 (single domain, momentum-source back-scatter): likewise k_fold_sources (uSourceDrag += D, uSource += uParticle D).
// Same operations on the same operands in the same order as the separate kernels: identical bits.  With FINISH != 0 every tile runs,
// also one whose bucket is empty (its cells may have been reached by the fallback atomics).
// FINISH 3 / 4 (z-slabs): FINISH 1 / 2 for the tiles of the z-layers [fin.tk_lo, fin.tk_hi) -- planes that receive nothing from a neighbour's reverse halo,
//          whose cells' sums are therefore complete here -- and FINISH 0 for the others, in ONE launch: the finish of the interior no longer costs a
//          pass of its own over the accumulators (k_finalize_cells / k_fold_sources keep the few planes at the slab's ends).
struct TileFinish { const double* vol; double* alpha; double* uParticle; double* R; const double* uParticleC; double* uSourceDrag; int tk_lo, tk_hi; };
template <int FINISH>
__global__ __launch_bounds__(256) void k_tile_reduce(TileBuckets tb, double* __restrict__ dst0, double* __restrict__ dst3, unsigned char* __restrict__ touched, TileFinish fin) {
    __shared__ double acc[kTileCells * 4];
    const uint32_t tile = blockIdx.x;
    uint32_t cnt = tb.fill[tile];
    const uint32_t cap = tb.cap[tile];
    if (cnt > cap) cnt = cap;
    // (block-uniform; a compile-time constant for FINISH 0 .. 2)
    const int tkz = (int)(tile / (uint32_t)(tb.tg.ntx * tb.tg.nty));
    const int mode = FINISH >= 3 ? ((tkz >= fin.tk_lo && tkz < fin.tk_hi) ? FINISH - 2 : 0) : FINISH;
    if (mode == 0 && cnt == 0) return;
    if (cnt) tile_bucket_sum<4>(tb, tile, cnt, acc);
    const TilePos tp = tile_pos(tb.tg, tile);
    for (int l = threadIdx.x; l < kTileCells; l += 256) {
        const TileCell tc = tile_cell(tp, l);
        if (!tc.inside(tb.tg)) continue;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        if (cnt) { a0 = acc[agg_at<kTileCells>(l, 0)]; a1 = acc[agg_at<kTileCells>(l, 1)]; a2 = acc[agg_at<kTileCells>(l, 2)]; a3 = acc[agg_at<kTileCells>(l, 3)]; }
        const bool any = !(a0 == 0.0 && a1 == 0.0 && a2 == 0.0 && a3 == 0.0);
        const size_t c = tc.index(tb.tg);
        if (mode == 0) {
            if (!any) continue;
            dst0[c] += a0;
            double* d = dst3 + 3 * c;
            const double d0 = d[0] + a1, d1 = d[1] + a2, d2 = d[2] + a3;
            d[0] = d0; d[1] = d1; d[2] = d2;
            if (touched) touched[c] = 1;
        } else if (mode == 1) {
            // the accumulators hold what the fallback atomics left (touched says so); they go back to zero, the cell is finished
            const bool t = touched[c] != 0;
            if (!any && !t) continue;
            double pv = a0, u0 = a1, u1 = a2, u2 = a3;
            if (t) {
                double* d = dst3 + 3 * c;
                if (any) { pv = dst0[c] + a0; u0 = d[0] + a1; u1 = d[1] + a2; u2 = d[2] + a3; }
                else { pv = dst0[c]; u0 = d[0]; u1 = d[1]; u2 = d[2]; }
                dst0[c] = 0.0; d[0] = 0.0; d[1] = 0.0; d[2] = 0.0;
                touched[c] = 0;
            }
            const double V = fin.vol[c];                      // setCellVolFraction FoamYade.C:318-328
            const double pvolC = 1.0 - (pv / V);
            const double al = ((pvolC > 0.10) ? pvolC : 0.10);
            fin.alpha[c] = al;
            if (fin.R) fin.R[8 * c + 3] = al;
            double* o = fin.uParticle + 3 * c;
            o[0] = u0 / V; o[1] = u1 / V; o[2] = u2 / V;
        } else {
            const double D0 = dst0[c];                        // what the fallback atomics added to the drag accumulator (usually nothing)
            double D = D0;
            double* sp = dst3 + 3 * c;
            if (!any && D0 == 0.0) continue;
            double s0 = sp[0], s1 = sp[1], s2 = sp[2];
            if (any) { D += a0; s0 += a1; s1 += a2; s2 += a3; }
            if (D0 != 0.0) dst0[c] = 0.0;                     // the accumulator is empty again either way
            if (D != 0.0) {                                   // k_fold_sources, FoamYade.C:385-386
                fin.uSourceDrag[c] += D;
                const double* up = fin.uParticleC + 3 * c;
                s0 = s0 + (up[0] * D); s1 = s1 + (up[1] * D); s2 = s2 + (up[2] * D);
            }
            sp[0] = s0; sp[1] = s1; sp[2] = s2;
        }
    }
}

// setCellVolFraction FoamYade.C:318-328: assignment on the cells this batch touched; accumulators reset for the next batch
__global__ __launch_bounds__(256) void k_finalize_cells(int32_t n_cells, const double* __restrict__ vol, double* __restrict__ pvol_acc,
                                                        double* __restrict__ up_acc, unsigned char* __restrict__ touched,
                                                        double* __restrict__ alpha, double* __restrict__ uParticle, double* __restrict__ R) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cells) return;
    if (!touched[c]) return;
    touched[c] = 0;
    const double V = vol[c];
    const double pvolC = 1.0 - (pvol_acc[c] / V);
    const double a = ((pvolC > 0.10) ? pvolC : 0.10);
    alpha[c] = a;
    if (R) R[8 * (size_t)c + 3] = a;       // the force pass reads alpha out of the packed cell record (k_pack_cells)
    double* up = up_acc + 3 * (size_t)c;
    double* o = uParticle + 3 * (size_t)c;
    o[0] = up[0] / V; o[1] = up[1] / V; o[2] = up[2] / V;
    pvol_acc[c] = 0.0; up[0] = 0.0; up[1] = 0.0; up[2] = 0.0;
}

// after all pairs of a batch: uSourceDrag += D, uSource += uParticle * D (FoamYade.C:385-386), D reset for the next batch
__global__ __launch_bounds__(256) void k_fold_sources(int64_t n_field, double* __restrict__ drag_acc, const double* __restrict__ uParticle,
                                                      double* __restrict__ uSourceDrag, double* __restrict__ uSource) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_field) return;
    const double D = drag_acc[c];
    if (D == 0.0) return;
    drag_acc[c] = 0.0;
    uSourceDrag[c] += D;
    const double* up = uParticle + 3 * (size_t)c;
    double* s = uSource + 3 * (size_t)c;
    const double s0 = s[0] + (up[0] * D), s1 = s[1] + (up[1] * D), s2 = s[2] + (up[2] * D);
    s[0] = s0; s[1] = s1; s[2] = s2;
}

}  // namespace

int launch_finalize_cells(hipStream_t s, int32_t n_cells, const double* vol, double* pvol_acc, double* up_acc,
                          unsigned char* touched, double* alpha, double* uParticle, double* R) {
    hipLaunchKernelGGL(k_finalize_cells, dim3(div_up(n_cells, 256)), dim3(256), 0, s, n_cells, vol, pvol_acc, up_acc, touched, alpha, uParticle, R);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_fold_sources(hipStream_t s, int64_t n_field, double* drag_acc, const double* uParticle, double* uSourceDrag, double* uSource) {
    return launch_n(s, k_fold_sources, n_field, 256, n_field, drag_acc, uParticle, uSourceDrag, uSource);
}

int launch_tile_caps(hipStream_t s, TileBuckets a, TileBuckets b, unsigned int* also_zero) {
    if (!a.cell && !b.cell) return also_zero ? fail(FY_ERR_INVALID, "launch_tile_caps: nothing to launch for the counter") : FY_OK;
    hipLaunchKernelGGL(k_tile_caps, dim3(2), dim3(1024), 0, s, a, b, also_zero);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_tile_reduce(hipStream_t s, TileBuckets tb, double* dst0, double* dst3, unsigned char* touched) {
    if (!tb.cell) return FY_OK;
    hipLaunchKernelGGL(k_tile_reduce<0>, dim3((unsigned)tb.tg.n_tiles()), dim3(256), 0, s, tb, dst0, dst3, touched, TileFinish{});
    FY_LAUNCH_CHECK();
    return FY_OK;
}

// the reductions that also finish cells run over every tile: without buckets there is nothing to run over
template <int FINISH>
static int tile_reduce_finish(hipStream_t s, const char* who, TileBuckets tb, double* dst0, double* dst3, unsigned char* touched, TileFinish fin) {
    if (!tb.cell) return fail(FY_ERR_INVALID, "%s without tile buckets", who);
    hipLaunchKernelGGL(k_tile_reduce<FINISH>, dim3((unsigned)tb.tg.n_tiles()), dim3(256), 0, s, tb, dst0, dst3, touched, fin);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_tile_reduce_finalize(hipStream_t s, TileBuckets tb, double* pvol_acc, double* up_acc, unsigned char* touched, const double* vol, double* alpha,
                                double* uParticle, double* R) {
    return tile_reduce_finish<1>(s, "launch_tile_reduce_finalize", tb, pvol_acc, up_acc, touched, TileFinish{vol, alpha, uParticle, R, nullptr, nullptr, 0, 0});
}
int launch_tile_reduce_fold(hipStream_t s, TileBuckets tb, double* drag_acc, double* uSource, const double* uParticle, double* uSourceDrag) {
    return tile_reduce_finish<2>(s, "launch_tile_reduce_fold", tb, drag_acc, uSource, nullptr, TileFinish{nullptr, nullptr, nullptr, nullptr, uParticle, uSourceDrag, 0, 0});
}
// z-slabs: the tiles of the z-layers [tk_lo, tk_hi) are finished in the reduction (setCellVolFraction resp. the fold of the sources), the others only summed
int launch_tile_reduce_finalize_layers(hipStream_t s, TileBuckets tb, double* pvol_acc, double* up_acc, unsigned char* touched, const double* vol, double* alpha,
                                       double* uParticle, double* R, int tk_lo, int tk_hi) {
    return tile_reduce_finish<3>(s, "launch_tile_reduce_finalize_layers", tb, pvol_acc, up_acc, touched, TileFinish{vol, alpha, uParticle, R, nullptr, nullptr, tk_lo, tk_hi});
}
int launch_tile_reduce_fold_layers(hipStream_t s, TileBuckets tb, double* drag_acc, double* uSource, const double* uParticle, double* uSourceDrag, int tk_lo, int tk_hi) {
    return tile_reduce_finish<4>(s, "launch_tile_reduce_fold_layers", tb, drag_acc, uSource, nullptr, TileFinish{nullptr, nullptr, nullptr, nullptr, uParticle, uSourceDrag, tk_lo, tk_hi});
}

}  // namespace fy
