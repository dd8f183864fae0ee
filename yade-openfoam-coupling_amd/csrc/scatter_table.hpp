// The scatters' per-workgroup LDS aggregation table and its flush into the cell tiles' buckets, stated once for every particle kernel source that
// scatters (particle_locate.hip: the void-fraction deposit; particle_force.hip: the momentum back-scatter; particle_heat.hip: Sp / Su; particle_tiles.hip:
// the buckets' reduction).  Device only; everything here is inlined into its caller: including this header adds no symbol to an object.
#pragma once
#include <hip/hip_runtime.h>

#include "particle_kernels.hpp"

namespace fy {
namespace {

__device__ __forceinline__ void atomic_add_f64(double* p, double v) {
    // global_atomic_add_f64, no return value, device (agent) scope.  (Workgroup-scope atomics were measured: no faster.)
    unsafeAtomicAdd(p, v);
}

// ------------------------------------------------------------------------------------------------ LDS aggregation of scatters
// Binned particles that share a workgroup also share most of their stencil cells (measured on the C3 cloud: 8.4 (particle, cell)
// pairs per distinct cell in a 256-particle block, 12 in a 1024-particle block).  FP64 global atomics are what bounds the scatter
// phases (force kernel: 10.0 ms with, 2.1 ms without them at 10 M particles), so every workgroup first sums its contributions
// per cell in an LDS hash table (ds_add_f64) and only the per-cell totals go out as global_atomic_add_f64.
constexpr uint32_t kAggEmpty = 0xffffffffu;

template <int LOG2SLOTS>
__device__ __forceinline__ int agg_slot(uint32_t* keys, uint32_t cell) {
    uint32_t h = (cell * 2654435761u) >> (32 - LOG2SLOTS);
#pragma unroll 1
    for (int pr = 0; pr < 24; ++pr) {
        const uint32_t old = atomicCAS(&keys[h], kAggEmpty, cell);
        if (old == kAggEmpty || old == cell) return (int)h;
        h = (h + 1) & ((1u << LOG2SLOTS) - 1u);
    }
    return -1;      // table crowded: caller falls back to a direct global atomic
}

__device__ __forceinline__ void lds_add_f64(double* p, double v) { unsafeAtomicAdd(p, v); }   // ds_add_f64

// Where component j of table slot h lives.  Component-major (round 4): an 8-byte LDS access is banked by (byte address / 4) mod 32 within
// groups of 16 lanes, so slot-major storage (4 h + j: a 32-byte stride) lets the random slots of a group reach only 4 of the 16 bank pairs
// for a given j -- at least 4-way conflicts by construction; component-major (j N + h) spreads them over all 16.
// Measured (profiles/r04_lds_table_layout.txt): the micro-benchmark's random-slot ds_add_f64 rate doubles (1.4 -> 2.9 lanes per clock per CU),
// k_force_gaussian loses a quarter of its conflict cycles and a third of its LDS wait cycles but only 0.03 ms -- what is left are the
// 16 random slots of a lane group on 16 bank pairs (~3 deep), same-cell adds (an atomic cannot broadcast) and the 4-byte CAS probes.
template <int NSLOTS> __device__ __forceinline__ int agg_at(int h, int j) { return j * NSLOTS + h; }

// an empty table of NSLOTS entries with NC sums each; the caller synchronises before the first agg_slot
template <int NSLOTS, int NTHREADS, int NC>
__device__ __forceinline__ void table_clear(uint32_t (&keys)[NSLOTS], double (&vals)[NSLOTS * NC]) {
    static_assert(NC == 2 || NC == 4, "sums per table entry");
    for (int q = threadIdx.x; q < NSLOTS; q += NTHREADS) {
        keys[q] = kAggEmpty;
        vals[q] = 0.0; vals[q + NSLOTS] = 0.0;
        if constexpr (NC == 4) { vals[q + 2 * NSLOTS] = 0.0; vals[q + 3 * NSLOTS] = 0.0; }
    }
}

// ------------------------------------------------------------------------------------------------ tile buckets (see particle_kernels.hpp)
// storage cell index -> (tile, cell inside the tile)
__device__ __forceinline__ void tile_of(const TileGrid& tg, uint32_t cl, uint32_t* tile, uint32_t* local) {
    const uint32_t i = cl % (uint32_t)tg.nx, r = cl / (uint32_t)tg.nx;
    const uint32_t j = r % (uint32_t)tg.ny, k = r / (uint32_t)tg.ny;
    *tile = (i >> 3) + (uint32_t)tg.ntx * ((j >> 3) + (uint32_t)tg.nty * (k >> 3));
    *local = (i & 7u) | ((j & 7u) << 3) | ((k & 7u) << 6);
}
// and back: the tile's position in the grid of tiles (once per workgroup), then (tile, cell inside the tile) -> storage cell index; false: the tile is
// cut by the block's edge and this cell lies beyond it
struct TilePos { int ti, tj, tk; };
__device__ __forceinline__ TilePos tile_pos(const TileGrid& tg, uint32_t tile) {
    return TilePos{(int)(tile % (uint32_t)tg.ntx), (int)((tile / (uint32_t)tg.ntx) % (uint32_t)tg.nty), (int)(tile / (uint32_t)(tg.ntx * tg.nty))};
}
struct TileCell {
    int i, j, k;
    __device__ __forceinline__ bool inside(const TileGrid& tg) const { return !(i >= tg.nx || j >= tg.ny || k >= tg.nzs); }
    __device__ __forceinline__ size_t index(const TileGrid& tg) const { return (size_t)i + (size_t)tg.nx * ((size_t)j + (size_t)tg.ny * (size_t)k); }
};
__device__ __forceinline__ TileCell tile_cell(const TilePos& t, int l) { return TileCell{t.ti * 8 + (l & 7), t.tj * 8 + ((l >> 3) & 7), t.tk * 8 + (l >> 6)}; }

// A workgroup's aggregation table -> the tiles' buckets.  Per table entry: which tile, and the entry's rank among this workgroup's
// entries for that tile (a 128-slot LDS map: a workgroup's stencils reach a few dozen tiles); one returning global atomic per
// (workgroup, tile) claims the run; plain stores.  What finds no room (bucket full, map full, or no buckets at all) is added with
// global atomics.  Every thread of the workgroup calls this (it synchronises).
// NC sums per entry: 4 -- component 0 -> dst0[c], components 1 .. 3 -> dstN[3 c + 0 .. 2], touched[c] = 1 (nullable) where the atomics went;
//                    2 -- component 0 -> dst0[c], component 1 -> dstN[c] (two of a bucket entry's four value slots; `touched` is not looked at).
constexpr int kTileMap = 128;
struct TileMapLds { uint32_t tile[kTileMap], cnt[kTileMap], base[kTileMap]; };

template <int NSLOTS, int NTHREADS, int NC>
__device__ __forceinline__ void flush_table(const uint32_t* keys, const double* vals, TileMapLds& m, const TileBuckets& tb, double* __restrict__ dst0,
                                            double* __restrict__ dstN, unsigned char* __restrict__ touched) {
    static_assert(NSLOTS % NTHREADS == 0, "table slots per thread");
    static_assert(NC == 2 || NC == 4, "sums per table entry");
    constexpr int R = NSLOTS / NTHREADS;
    uint32_t pr[R];                                         // map slot << 16 | rank; 0xffffffff: empty table slot; 0xfffffffe: no room in the map
#pragma unroll
    for (int r = 0; r < R; ++r) pr[r] = keys[threadIdx.x + r * NTHREADS] == kAggEmpty ? 0xffffffffu : 0xfffffffeu;
    if (tb.cell) {                                          // (uniform)
        for (int q = threadIdx.x; q < kTileMap; q += NTHREADS) { m.tile[q] = kAggEmpty; m.cnt[q] = 0; }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (pr[r] == 0xffffffffu) continue;
            uint32_t tile, local;
            tile_of(tb.tg, keys[threadIdx.x + r * NTHREADS], &tile, &local);
            uint32_t h = (tile * 2654435761u) >> 25;        // 7 bits
#pragma unroll 1
            for (int probe = 0; probe < kTileMap; ++probe) {
                const uint32_t old = atomicCAS(&m.tile[h], kAggEmpty, tile);
                if (old == kAggEmpty || old == tile) { pr[r] = (h << 16) | atomicAdd(&m.cnt[h], 1u); break; }
                h = (h + 1) & (kTileMap - 1);
            }
        }
        __syncthreads();
        if (threadIdx.x < kTileMap && m.tile[threadIdx.x] != kAggEmpty)
            m.base[threadIdx.x] = atomicAdd(&tb.fill[m.tile[threadIdx.x]], m.cnt[threadIdx.x]);
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (pr[r] == 0xffffffffu) continue;
        const int q = threadIdx.x + r * NTHREADS;
        const uint32_t c = keys[q];
        double v[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) v[j] = vals[agg_at<NSLOTS>(q, j)];
        bool placed = false;
        if (pr[r] != 0xfffffffeu) {
            const uint32_t slot = pr[r] >> 16, rank = pr[r] & 0xffffu;
            const uint32_t tile = m.tile[slot], pos = m.base[slot] + rank;
            if (pos < tb.cap[tile]) {
                uint32_t t2, local;
                tile_of(tb.tg, c, &t2, &local);
                const size_t at = (size_t)tb.off[tile] + pos;
                tb.cell[at] = local;
                double2* o = reinterpret_cast<double2*>(tb.val + 4 * at);
                o[0] = make_double2(v[0], v[1]);
                if constexpr (NC == 4) o[1] = make_double2(v[2], v[3]);
                placed = true;
            }
        }
        if (!placed) {
            atomic_add_f64(&dst0[c], v[0]);
            if constexpr (NC == 4) {
                atomic_add_f64(&dstN[3 * (size_t)c + 0], v[1]);
                atomic_add_f64(&dstN[3 * (size_t)c + 1], v[2]);
                atomic_add_f64(&dstN[3 * (size_t)c + 2], v[3]);
                if (touched) touched[c] = 1;
            } else {
                atomic_add_f64(&dstN[c], v[1]);
            }
        }
    }
}

// One workgroup (256 threads) per tile: the first cnt entries of the tile's bucket summed into a dense LDS accumulator of kTileCells x NC
// (ds_add_f64: ~37 x the global atomics' rate), component j of tile cell l at agg_at<kTileCells>(l, j).  Every thread calls this (it synchronises).
template <int NC>
__device__ __forceinline__ void tile_bucket_sum(const TileBuckets& tb, uint32_t tile, uint32_t cnt, double (&acc)[kTileCells * NC]) {
    static_assert(NC == 2 || NC == 4, "sums per bucket entry");
    for (int q = threadIdx.x; q < kTileCells * NC; q += 256) acc[q] = 0.0;
    __syncthreads();
    const size_t off = tb.off[tile];
    for (uint32_t j = threadIdx.x; j < cnt; j += 256) {
        const uint32_t l = tb.cell[off + j];
        const double2* v = reinterpret_cast<const double2*>(tb.val + 4 * (off + j));
        const double2 v0 = v[0];
        if constexpr (NC == 4) {
            const double2 v1 = v[1];
            lds_add_f64(&acc[agg_at<kTileCells>(l, 0)], v0.x); lds_add_f64(&acc[agg_at<kTileCells>(l, 1)], v0.y);
            lds_add_f64(&acc[agg_at<kTileCells>(l, 2)], v1.x); lds_add_f64(&acc[agg_at<kTileCells>(l, 3)], v1.y);
        } else {
            lds_add_f64(&acc[agg_at<kTileCells>(l, 0)], v0.x); lds_add_f64(&acc[agg_at<kTileCells>(l, 1)], v0.y);
        }
    }
    __syncthreads();
}

}  // namespace
}  // namespace fy
