// Particle half of the hot path as hand-written HIP for gfx950 (MI355X, wave64), in five sources behind one host interface (particle_kernels.hpp):
//   particle_bin.hip      (this file) bin_count / scan / bin_scatter: AoS wire records -> spatially binned SoA (locality only; results independent), the
//                         placement's ordering by chain length, record traffic (fibre repack, z-slab migration), the stencils' read-back
//   particle_locate.hip   locate_deposit: meshTree::nnearestCellsRange (meshTree.C:148-238) as a flat per-lane DFS over the preorder tree with an LDS stack, or as a
//                         scan of candidate lists, fused with calcInterpWeightGaussian (FoamYade.C:293-316) and buildCellPartList's deposition (FoamYade.C:261-290)
//   particle_tiles.hip    the scatters' tile buckets -> cell arrays; finalize_cells: setCellVolFraction (FoamYade.C:318-328); fold_sources
//   particle_force.hip    force_gaussian: hydroDragForce + archimedesForce + source back-scatter (FoamYade.C:354-389,415-435);
//                         point_force: findCell + stokesDragForce + stokesDragTorque (FoamYade.C:248-253,437-453)
//   particle_heat.hip     particle-fluid heat exchange (not in the reference)
// Device functions reach more than one of them through scatter_table.hpp (the LDS aggregation table and its flush) and stencil_ring.hpp.
// All arithmetic is FP64 in the reference's operation order; the files are compiled with -ffp-contract=off so that the distance comparisons that steer the
// tree walk are bit-identical to the CPU reference (index work must be exact).  Everything here is HBM/L2-latency bound: no MFMA (no dense contraction).
#include "particle_kernels.hpp"

#include "common.hpp"
#include "device_util.hpp"
#include "stencil_ring.hpp"

namespace fy {
namespace {

// Block order: plain round-robin.  An XCD-aware remap (guide T1: block b runs on XCD b % 8, give each XCD a contiguous run of the
// binned particle order) was measured on MI355X and LOSES for the particle kernels: locate+deposit 14.5 -> 16.1 ms, force 10.0 ->
// 10.8 ms at 10 M particles, because the FP64 atomics of a spatially compact run pile onto few memory channels.

// ------------------------------------------------------------------------------------------------ binning
__device__ __forceinline__ uint32_t bin_key(const BinGrid& g, double x, double y, double z) {
    int bx = (int)floor((x - g.ox) * g.inv_h);
    int by = (int)floor((y - g.oy) * g.inv_h);
    int bz = (int)floor((z - g.oz) * g.inv_h);
    bx = min(max(bx, 0), g.nbx - 1);
    by = min(max(by, 0), g.nby - 1);
    bz = min(max(bz, 0), g.nbz - 1);
    const uint32_t brick = ((uint32_t)(bz >> 2) * g.by4 + (uint32_t)(by >> 2)) * g.bx4 + (uint32_t)(bx >> 2);
    const uint32_t local = ((uint32_t)(bz & 3) << 4) | ((uint32_t)(by & 3) << 2) | (uint32_t)(bx & 3);
    return brick * 64u + local;
}

__global__ __launch_bounds__(256) void k_bin_count(const double* __restrict__ rec, int64_t n, BinGrid g,
                                                   uint32_t* __restrict__ key, uint32_t* __restrict__ rank,
                                                   uint32_t* __restrict__ hist) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* r = rec + 10 * i;
    const uint32_t k = bin_key(g, r[0], r[1], r[2]);
    key[i] = k;
    rank[i] = atomicAdd(&hist[k], 1u);
}

// exclusive scan of 2048-element tiles; tile totals go to block_sums (scanned in place by k_scan_sums)
__global__ __launch_bounds__(256) void k_scan_tiles(uint32_t* __restrict__ data, uint32_t n, uint32_t* __restrict__ block_sums) {
    __shared__ uint32_t wave_tot[4];
    const uint32_t base = blockIdx.x * 2048u + threadIdx.x * 8u;
    uint32_t v[8];
    uint32_t t = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t x = (base + j < n) ? data[base + j] : 0u;
        v[j] = t;
        t += x;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = t;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(inc, d, 64);
        if (lane >= d) inc += y;
    }
    if (lane == 63) wave_tot[wv] = inc;
    __syncthreads();
    uint32_t woff = 0;
    for (int q = 0; q < wv; ++q) woff += wave_tot[q];
    const uint32_t excl = woff + inc - t;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (base + j < n) data[base + j] = excl + v[j];
    if (threadIdx.x == 255) block_sums[blockIdx.x] = woff + inc;
}

__global__ __launch_bounds__(1024) void k_scan_sums(uint32_t* __restrict__ sums, uint32_t nb) {
    __shared__ uint32_t wave_tot[16];
    const uint32_t per = (nb + 1023u) / 1024u;
    const uint32_t lo = threadIdx.x * per;
    uint32_t t = 0;
    for (uint32_t j = 0; j < per; ++j)
        if (lo + j < nb) t += sums[lo + j];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = t;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(inc, d, 64);
        if (lane >= d) inc += y;
    }
    if (lane == 63) wave_tot[wv] = inc;
    __syncthreads();
    uint32_t woff = 0;
    for (int q = 0; q < wv; ++q) woff += wave_tot[q];
    uint32_t run = woff + inc - t;
    for (uint32_t j = 0; j < per; ++j)
        if (lo + j < nb) {
            const uint32_t x = sums[lo + j];
            sums[lo + j] = run;
            run += x;
        }
}

// Counting-sort placement in two steps: the scatter writes ONLY the 4-byte source index to the sorted position (random 4-B
// writes), then a gather pass reads whole 80-byte records at random and writes the SoA arrays coalesced.  Scattering the seven
// doubles directly (10 M x 8 random 8-byte writes) measured 1.28 ms at 10 M particles; random reads are far cheaper than random writes.
__global__ __launch_bounds__(256) void k_bin_scatter(int64_t n, const uint32_t* __restrict__ key, const uint32_t* __restrict__ rank,
                                                     const uint32_t* __restrict__ start, const uint32_t* __restrict__ tile_off,
                                                     int32_t* __restrict__ orig) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = key[i];
    const size_t d = (size_t)start[k] + tile_off[k >> 11] + rank[i];
    orig[d] = (int32_t)i;
}

// The chain length of a particle barely changes from one coupling step to the next (at rest: not at all), and the force pass's three loops
// over a stencil run to the LONGEST chain of a wave: with a wave's lanes holding a 0 .. 14 mix around the mean of 5.46 that is ~9.5
// iterations, with chains of one length (two at a class boundary) ~5.6.  So when the placement is recomputed, every run of 512 slots (one
// workgroup of the locate and of the force pass: the same particles, the same cells in reach) is put in order of the chain lengths of the
// step before -- stable, so the cell order survives inside a class.  k_chain_by_wire files the lengths under the wire index first (the
// placement they were computed in is about to be overwritten).  Costs two small launches per rebin_interval steps.
constexpr int kOrderClasses = 3 * (kMaxK + 1);
__global__ __launch_bounds__(256) void k_chain_by_wire(const int32_t* __restrict__ orig, const int32_t* __restrict__ chain_len,
                                                       const unsigned char* __restrict__ scan_class, int64_t n, unsigned char* __restrict__ kwire) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = chain_len[i];
    const int k = c < 0 ? 0 : (c > kMaxK ? kMaxK : c);
    const int sc = scan_class ? (int)scan_class[i] : 0;
    kwire[orig[i]] = (unsigned char)(3 * k + sc);        // chain length first, then how far the list scan ran (measured: +0.5 - 1 % of the particle phase over the length alone; the other way round is no better)
}
constexpr int kRun = kOrderRun;      // the locate's workgroup (1024 loses 4 % of the step to locality, 256 is no better)
__global__ __launch_bounds__(kRun) void k_order_blocks_by_chain(int32_t* __restrict__ orig, const unsigned char* __restrict__ kwire, int64_t n) {
    __shared__ uint32_t cnt[kOrderClasses][kRun / 64];             // [class][wave]
    const int64_t i = (int64_t)blockIdx.x * kRun + threadIdx.x;
    const bool have = i < n;
    const int32_t w = have ? orig[i] : 0;
    const int k = have ? (int)kwire[w] : -1;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t rank = 0;
    for (int c = 0; c < kOrderClasses; ++c) {
        const unsigned long long m = __ballot(k == c);
        if (k == c) rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) cnt[c][wv] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (!have) return;
    uint32_t before = 0;
    for (int c = 0; c < k; ++c) for (int q = 0; q < kRun / 64; ++q) before += cnt[c][q];
    for (int q = 0; q < wv; ++q) before += cnt[k][q];
    orig[(int64_t)blockIdx.x * kRun + before + rank] = w;
}

__global__ __launch_bounds__(256) void k_bin_gather(const double* __restrict__ rec, int64_t n, ParticleSoA p) {
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= n) return;
    const double* r = rec + 10 * (size_t)p.orig[d];
    p.px[d] = r[0]; p.py[d] = r[1]; p.pz[d] = r[2];
    p.vx[d] = r[3]; p.vy[d] = r[4]; p.vz[d] = r[5];
    p.rad[d] = r[9];
}

// ---- particle migration between z-slabs: records whose containing cell now lies in a neighbour's planes are packed for
// that neighbour, the others compacted; 11 doubles per particle = the wire record + its tag (an int64 carried as a bit pattern)
__global__ __launch_bounds__(256) void k_migrate_pack(const double* __restrict__ rec, const int64_t* __restrict__ tags, int64_t n, SlabOwn own,
                                                      unsigned int* __restrict__ counters, double* __restrict__ stay, double* __restrict__ up,
                                                      double* __restrict__ down) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* r = rec + 10 * i;
    const double z = r[2];
    int kz = (int)floor((z - own.oz) / own.dx);
    kz = min(max(kz, 0), own.nzglob - 1);
    const int dest = !(z == z) ? 0 : (kz >= own.k1 ? 1 : (kz < own.k0 ? 2 : 0));      // NaN stays (and is never located)
    double* out = dest == 0 ? stay : (dest == 1 ? up : down);
    const unsigned int pos = atomicAdd(&counters[dest], 1u);
    double* o = out + 11 * (size_t)pos;
    for (int q = 0; q < 10; ++q) o[q] = r[q];
    o[10] = __longlong_as_double(tags ? (long long)tags[i] : (long long)-1);
}

__global__ __launch_bounds__(256) void k_migrate_unpack(const double* __restrict__ packed, int64_t n, double* __restrict__ rec, int64_t* __restrict__ tags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* r = packed + 11 * i;
    for (int q = 0; q < 10; ++q) rec[10 * i + q] = r[q];
    if (tags) tags[i] = (int64_t)__double_as_longlong(r[10]);
}

// found flags in wire order (FoamYade.C:141,204,222): 1 if the particle has a stencil, -1 otherwise.  Only the parallel-Yade
// protocol and the tests read them, so they are formed on demand instead of as 10 M scattered 4-byte stores in every force pass.
__global__ __launch_bounds__(256) void k_found_from_chain(ParticleSoA p, int64_t n, int32_t* __restrict__ found_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) found_out[p.orig[i]] = p.chain_len[i] > 0 ? 1 : -1;
}

// sorted chain-order stencil storage -> [n][16] ascending-d2 rows in wire order (parity tests only)
__global__ __launch_bounds__(256) void k_unpack_stencils(ParticleSoA p, int64_t n, int32_t* __restrict__ k_out, int32_t* __restrict__ ids,
                                                         double* __restrict__ w, int32_t* __restrict__ chain_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const StencilSpan sp = stencil_span(p.chain_len[i]);
    const int chain = sp.chain, k = sp.k;
    const size_t orig = (size_t)p.orig[i];
    k_out[orig] = chain;       // the reference's container also grows past 12 (meshTree.H:74-77)
    chain_out[orig] = chain;
    for (int t = 0; t < kMaxK; ++t) {
        if (t < k) {
            const size_t slot = stencil_slot(p, i, chain - 1 - t);      // last push first
            ids[orig * kMaxK + t] = p.ids[slot];
            w[orig * kMaxK + t] = p.w[slot];
        } else {
            ids[orig * kMaxK + t] = -1;
            w[orig * kMaxK + t] = 0.0;
        }
    }
}

// reverse-halo accumulation: y += x, and flag the cells that received something (stands in for the neighbour's touched flags)
__global__ __launch_bounds__(256) void k_add_mark(double* __restrict__ y, const double* __restrict__ x, size_t n, unsigned char* __restrict__ mark) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    y[i] += v;
    if (mark && v != 0.0) mark[i] = 1;
}

__global__ __launch_bounds__(256) void k_fill_f64(double* __restrict__ p, size_t n, double v) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

}  // namespace

// Fibre coupling (`fibreCpl`, FoamYade.H:102): Yade sends 15 doubles per particle (FoamYade.C:131-136,161-165) and the position is read
// with that stride (FoamYade.C:194-198), but velocity, spin and radius are still taken from `buf[np*10 + 3..9]` of the SAME buffer
// (FoamYade.C:211-221).  The reference ships it that way; the narrow records the kernels consume are gathered with exactly that indexing.
__global__ void k_fibre_repack(const double* __restrict__ wide, double* __restrict__ rec, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) rec[10 * i + q] = wide[15 * i + q];
#pragma unroll
    for (int q = 3; q < 10; ++q) rec[10 * i + q] = wide[10 * i + q];
}

int launch_bin_count(hipStream_t s, const double* rec, int64_t n, BinGrid g, uint32_t* key, uint32_t* rank, uint32_t* hist) {
    return launch_n(s, k_bin_count, n, 256, rec, n, g, key, rank, hist);
}

int launch_exclusive_scan_u32(hipStream_t s, uint32_t* data, uint32_t n, uint32_t* block_sums) {
    if (n == 0) return FY_OK;
    const uint32_t nb = (n + 2047u) / 2048u;
    hipLaunchKernelGGL(k_scan_tiles, dim3(nb), dim3(256), 0, s, data, n, block_sums);
    FY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, s, block_sums, nb);
    FY_LAUNCH_CHECK();
    return FY_OK;   // the tile offsets stay separate: consumers add block_sums[i >> 11]
}

int launch_bin_scatter(hipStream_t s, const double* rec, int64_t n, const uint32_t* key, const uint32_t* rank,
                       const uint32_t* start, const uint32_t* tile_off, ParticleSoA p, bool gather) {
    FY_TRY(launch_n(s, k_bin_scatter, n, 256, n, key, rank, start, tile_off, p.orig));
    return gather ? launch_bin_gather(s, rec, n, p) : FY_OK;
}

int launch_chain_by_wire(hipStream_t s, const int32_t* orig, const int32_t* chain_len, const unsigned char* scan_class, int64_t n, unsigned char* kwire) {
    return launch_n(s, k_chain_by_wire, n, 256, orig, chain_len, scan_class, n, kwire);
}
int launch_order_blocks_by_chain(hipStream_t s, int32_t* orig, const unsigned char* kwire, int64_t n) {
    return launch_n(s, k_order_blocks_by_chain, n, kRun, orig, kwire, n);
}

int launch_bin_gather(hipStream_t s, const double* rec, int64_t n, ParticleSoA p) { return launch_n(s, k_bin_gather, n, 256, rec, n, p); }

int launch_fibre_repack(hipStream_t s, const double* wide, double* rec, int64_t n) { return launch_n(s, k_fibre_repack, n, 256, wide, rec, n); }

int launch_migrate_pack(hipStream_t s, const double* rec, const int64_t* tags, int64_t n, SlabOwn own, unsigned int* counters, double* stay, double* up, double* down) {
    return launch_n(s, k_migrate_pack, n, 256, rec, tags, n, own, counters, stay, up, down);
}

int launch_migrate_unpack(hipStream_t s, const double* packed, int64_t n, double* rec, int64_t* tags) {
    return launch_n(s, k_migrate_unpack, n, 256, packed, n, rec, tags);
}

int launch_found_from_chain(hipStream_t s, ParticleSoA p, int64_t n, int32_t* found) { return launch_n(s, k_found_from_chain, n, 256, p, n, found); }

int launch_unpack_stencils(hipStream_t s, ParticleSoA p, int64_t n, int32_t* k, int32_t* ids, double* w, int32_t* chain) {
    return launch_n(s, k_unpack_stencils, n, 256, p, n, k, ids, w, chain);
}

int launch_add_mark(hipStream_t s, double* y, const double* x, size_t n, unsigned char* mark) { return launch_n(s, k_add_mark, (int64_t)n, 256, y, x, n, mark); }

int launch_fill_f64(hipStream_t s, double* p, size_t n, double v) { return launch_n(s, k_fill_f64, (int64_t)n, 256, p, n, v); }

}  // namespace fy
