// Particle half, second phase (the five sources: particle_bin.hip): where a particle's stencil comes from -- the k-d walk, the per-(cell, octant) candidate
// lists that stand in for it on a lattice -- and the Gaussian weights and the void-fraction deposit that are fused with it.
#include "particle_kernels.hpp"

#include <algorithm>

#include "common.hpp"
#include "device_util.hpp"
#include "scatter_table.hpp"
#include "stencil_ring.hpp"

namespace fy {
namespace {

constexpr int kWave = 64;

// ------------------------------------------------------------------------------------------------ locate + deposit
// One lane per particle, one wave per 64-particle chunk of the binned order.  Per-lane DFS stack lives in LDS as
// [level][lane] uint4 = {offset, size | axis<<30, df2 (2 dwords)}: 16 B * 64 lanes = one 1 KiB row per level, and the bank of an
// entry depends on the lane only, so lanes at different levels never conflict.
// Node fetch.  Explicit: 32-byte {x,y,z,id} records (any mesh).  Implicit: for a uniform hex block whose centres were verified
// at create time to equal origin + (i + 0.5) * dx bit for bit, a node is just the packed (i,j,k) of its cell -- 4 bytes, 16 nodes
// per 64-byte line instead of 2 -- and the centre is recomputed with the same two IEEE operations (contraction is off).
// The divergent bottom-of-tree loads are what bound this kernel (one L1 tag lookup per distinct line per instruction), so
// trading ~12 FP64 ALU ops for 8x fewer lines is the MI355X-shaped choice.
struct NodeVal { double x, y, z; int32_t id; };

template <bool IMPLICIT>
__device__ __forceinline__ NodeVal fetch_node(const KdNode* __restrict__ tree, const uint32_t* __restrict__ packed, const ImplicitGeom& ig, uint32_t o) {
    NodeVal v;
    if constexpr (IMPLICIT) {
        const uint32_t q = packed[o];
        const int i = (int)(q & 1023u), j = (int)((q >> 10) & 1023u), k = (int)(q >> 20);     // 10 + 10 + 12 bits
        v.x = ig.ox + ((double)i + 0.5) * ig.dx;
        v.y = ig.oy + ((double)j + 0.5) * ig.dx;
        v.z = ig.oz + ((double)k + 0.5) * ig.dx;
        v.id = i + ig.nx * (j + ig.ny * k);
    } else {
        // the 32-byte node as two 16-byte loads: the compiler's own split of the struct copy is 16 + 8 + 4, three passes of the address unit over one line -- the explicit walk of
        // 10 M particles through 4.1 M nodes 4.45 -> 3.80 ms.  (One line access per visit -- neighbouring lanes fetching both their nodes together, a half each, and swapping
        // halves by DPP -- was built too: same chains, 7 % SLOWER.  Past two accesses the walk is bound by the latency of its slowest lane's fetch, not by the address unit.)
        const uint4* q = reinterpret_cast<const uint4*>(tree + o);
        const uint4 lo = q[0], hi = q[1];
        v.x = __hiloint2double((int)lo.y, (int)lo.x); v.y = __hiloint2double((int)lo.w, (int)lo.z); v.z = __hiloint2double((int)hi.y, (int)hi.x); v.id = (int32_t)hi.z;
    }
    return v;
}

// Persistent lanes: a wave owns kLocPPB consecutive particles of the binned order and every lane pulls its next particle
// from the wave's range as soon as its walk ends (ballot + prefix count), so lanes do not idle while the slowest walk of a
// 64-particle chunk finishes (measured before this change: 36 % VALU lane utilisation, SQ_THREAD_CYCLES_VALU / 64 / SQ_ACTIVE_INST_VALU).
// One loop iteration = at most one pop and one node visit per lane; the Gaussian weights are formed later, at full width,
// by k_deposit -- here the squared distance of every chain member is parked in its weight slot.
constexpr int kLocPPB = 1024;
#ifndef FY_LOC_REFILL
#define FY_LOC_REFILL 12
#endif
constexpr int kLocRefill = FY_LOC_REFILL;    // refill once this many lanes are idle

// DFS stack entry.  Implicit nodes: 8 B -- the far side's df2 is
// NOT stored; the entry carries the parent's 10-bit lattice index along the split axis and df2 = (o + (idx + 0.5) dx - q)^2 is
// recomputed at pop time with the same IEEE operations, bit for bit.  Halving the entry doubles the waves a CU can hold
// (LDS: levels x 64 lanes x entry), and this kernel is latency bound.
//   implicit entry: bits 0..24 far offset | 25..49 far size | 50..51 axis of the far child | 52..63 parent index on the split axis
//   (offsets and sizes < 2^25 = 33.5 M nodes, lattice index < 4096: covers the 32.8 M-cell C5 block and 1280-plane weak-scaling boxes)
template <bool IMPLICIT, bool WIDE> struct StackEntry { typedef unsigned long long type; };
// explicit nodes, 8 B: offset | size << 25 | axis << 50 | t << 52, t = a 12-bit LOWER bound of df2 in units of maxdist / 4095 (round 6; 16 B with the exact df2 before).  A far side is
// visited when the bound is below `best`: a superset of what the exact test admits, and what it adds cannot change a chain -- every centre behind the plane has d >= df2 >= best in
// floating point too (the candidate lists' note below).  Half the LDS per wave: 13 -> 24 waves per CU, the walk of 10 M particles through 4.1 M nodes 3.76 -> 3.30 ms.
// WIDE (trees of 2^25 nodes and more): the 16-byte entry {offset, size | axis << 30, df2}.
template <> struct StackEntry<false, true> { typedef uint4 type; };

// Per-cell traversal start.  For a query q inside cell (ci,cj,ck) the top of the reference's walk is fully determined:
//  (a) an ancestor whose centre is farther than sqrt(maxdist) from every point of the cell can improve `best` but can never enter
//      the chain (meshTree.C:185-192 only queues d < maxdist), and any `best` >= maxdist it leaves behind is indistinguishable, for
//      the chain, from best = +inf: nodes it would have rejected are >= maxdist away and are not queued either;
//  (b) when the ancestor's lattice index on its split axis differs from the cell's by >= 2, the near side is the side holding the
//      cell (no exact comparison involved) and the far side is >= 1.5 dx away; by the time the reference comes back to it the near
//      subtree has been searched, best <= |q - own cell centre|^2 <= 0.75 dx^2 < 2.25 dx^2, so `df2 < best` (meshTree.C:225) fails.
// While both hold the walk just descends; the first node where one fails is where k_locate starts, with an empty stack.
// 160^3: 8.8 levels skipped on average, 47.1 -> 38.4 visits and 21.9 -> 14.6 stack entries per particle, chains bit-identical.
__global__ __launch_bounds__(256) void k_build_locate_start(const uint32_t* __restrict__ packed, ImplicitGeom ig, int32_t n_cells, double md_cells,
                                                            unsigned long long* __restrict__ start) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cells) return;
    const int cc[3] = {c % ig.nx, (c / ig.nx) % ig.ny, c / (ig.nx * ig.ny)};
    uint32_t o = 0, nn = (uint32_t)n_cells, axis = 0;
    while (nn > 0) {
        const uint32_t pk = packed[o];
        const int nd[3] = {(int)(pk & 1023u), (int)((pk >> 10) & 1023u), (int)(pk >> 20)};
        double g2 = 0.0;                                  // squared gap between the node centre and the (slightly inflated) cell box, in dx
        for (int a = 0; a < 3; ++a) {
            const double gap = fabs((double)(nd[a] - cc[a])) - 0.5 - 1e-6;
            if (gap > 0) g2 += gap * gap;
        }
        const int ds = nd[axis] - cc[axis];
        if (!(g2 >= md_cells) || (ds < 2 && ds > -2)) break;
        const uint32_t nl = nn >> 1, nr = nn - nl - 1u;
        if (ds > 0) { o = o + 1u; nn = nl; } else { o = o + 1u + nl; nn = nr; }
        axis = (axis == 2u ? 0u : axis + 1u);
    }
    if (nn == 0) { o = 0; axis = 0; nn = (uint32_t)n_cells; }   // cannot happen (a leaf's own cell fails (a)); fall back to the root
    start[c] = (unsigned long long)o | ((unsigned long long)nn << 25) | ((unsigned long long)axis << 50);
}

// ------------------------------------------------------------------------------------------------ candidate lists
// What the walk below produces is, exactly, the sequence of strict running minima of d(node, q) over the tree's nodes in near-first
// DFS order, kept where d < maxdist (meshTree.C:192-196): a far side is skipped only when df2 >= best (meshTree.C:225), every node
// behind it has d >= df2 in floating point too (the squared axis term is one of d's three non-negative addends and rounding is
// monotone), so a skipped subtree holds no improvement.  On the lattice that order is a function of (cell, octant) alone: the side
// taken at an ancestor whose lattice index on its split axis differs from the query cell's is decided by the cell, and where the
// index is the same the ancestor's coordinate IS the cell centre's (same expression, same bits), so the side is the octant bit
// `!(q - centre < 0)`.  Hence, per (cell, octant), ONE list of the nodes that can be a running minimum for some q of that octant, in
// DFS order; a particle evaluates d for ~7 listed nodes with the reference's operations instead of walking ~38 tree nodes with a
// stack.  k_build_locate_lists simulates the walk over the octant box B:
//   * a node enters the list unless it is outside the range for every q in B, or an earlier listed node Y is closer for every q in B
//     (d(Y,q) - d(X,q) is linear in q: its maximum over B is a sum of per-axis endpoint values).  A node left out this way never
//     lowers the running minimum below what Y already did and is never pushed, so the scan's `best` and chain are the walk's;
//   * a far side is skipped when it is out of range for all of B or some listed Y has d(Y,q) <= (q_a - plane)^2 on all of B -- a
//     superset of what the reference visits for any single q; extra nodes have d >= best and change nothing.
// All comparisons carry a margin (kListMargin, lattice units^2) far above the rounding of d (<= 1e-9 for |coordinate| / dx <= 1e6,
// enforced by the caller), and B is the half cell shrunk by kListEps at the faces: particles closer than 2 kListEps dx to a cell face
// (where floor() and the nearest centre may disagree by an ulp), outside the block, or in an octant whose list overflowed, are
// handed to the plain walk (k_locate with a work list).  The root is listed with a no-emit flag (it sets `best` but is never pushed,
// meshTree.C:156).  Verified against the walk on every golden case and by tools/proto/locate_lists.cpp (host prototype).
constexpr int kListLen = kLocateListLen;              // 24 codes per (cell, octant): 48 B = three 16-byte loads
constexpr double kListEps = 4e-6, kListMargin = 1e-8;
constexpr uint32_t kListEnd = 0xffffu, kListOverflow = 0xfffeu, kListNoEmit = 0x1000u;

__device__ __forceinline__ double ax_min2(double lo, double hi, double x) { const double g = x < lo ? lo - x : (x > hi ? x - hi : 0.0); return g * g; }
__device__ __forceinline__ double ax_max2(double lo, double hi, double x) { const double g = fmax(fabs(lo - x), fabs(hi - x)); return g * g; }

__global__ __launch_bounds__(256) void k_build_locate_lists(const uint32_t* __restrict__ packed, ImplicitGeom ig, int32_t n_cells, double md,
                                                            unsigned short* __restrict__ lists, int32_t cell0, int32_t n_listed) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;       // list number: (cell - cell0) * 8 + octant, cells [cell0, cell0 + n_listed)
    if (t >= (size_t)n_listed * 8) return;
    const int cell = cell0 + (int)(t >> 3), oct = (int)(t & 7);
    const int c[3] = {cell % ig.nx, (cell / ig.nx) % ig.ny, cell / (ig.nx * ig.ny)};
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        if ((oct >> a) & 1) { lo[a] = c[a] - kListEps; hi[a] = c[a] + 0.5 - kListEps; }
        else { lo[a] = c[a] - 0.5 + kListEps; hi[a] = c[a] + kListEps; }
    }
    unsigned long long st[28];                       // offset | size << 25 | axis << 50 | parent index on its split axis << 52
    uint32_t kept[kListLen];
    int nk = 0, sp = 0;
    bool overflow = false;
    uint32_t o = 0, nn = (uint32_t)n_cells, axis = 0;
    for (;;) {
        if (nn == 0) {
            if (sp == 0) break;
            const unsigned long long e = st[--sp];
            const uint32_t ea = (uint32_t)((e >> 50) & 3ull), pa = (ea == 0 ? 2u : ea - 1u);
            const int P = (int)(e >> 52);
            bool prune = ax_min2(lo[pa], hi[pa], (double)P) >= md + kListMargin;
            for (int y = 0; y < nk && !prune; ++y) {
                const int Y[3] = {(int)(kept[y] & 1023u), (int)((kept[y] >> 10) & 1023u), (int)(kept[y] >> 20)};
                double sdiff = 0.0;                  // max over B of d(Y,q) - (q_pa - P)^2
                for (int b = 0; b < 3; ++b) {
                    if (b == (int)pa) { const double k = (double)(P - Y[b]); sdiff += fmax(k * (2 * lo[b] - P - Y[b]), k * (2 * hi[b] - P - Y[b])); }
                    else sdiff += ax_max2(lo[b], hi[b], (double)Y[b]);
                }
                prune = sdiff <= -kListMargin;
            }
            if (!prune) { o = (uint32_t)(e & 0x1ffffffull); nn = (uint32_t)((e >> 25) & 0x1ffffffull); axis = ea; }
            continue;
        }
        const uint32_t pk = packed[o];
        const int X[3] = {(int)(pk & 1023u), (int)((pk >> 10) & 1023u), (int)(pk >> 20)};
        double dmin = 0.0;
        for (int a = 0; a < 3; ++a) dmin += ax_min2(lo[a], hi[a], (double)X[a]);
        if (dmin < md + kListMargin) {
            bool dom = false;
            for (int y = 0; y < nk && !dom; ++y) {
                const int Y[3] = {(int)(kept[y] & 1023u), (int)((kept[y] >> 10) & 1023u), (int)(kept[y] >> 20)};
                double sdiff = 0.0;                  // max over B of d(Y,q) - d(X,q); per axis (q-Y)^2 - (q-X)^2 = (X-Y)(2q - X - Y)
                for (int a = 0; a < 3; ++a) {
                    const double k = (double)(X[a] - Y[a]);
                    sdiff += fmax(k * (2 * lo[a] - X[a] - Y[a]), k * (2 * hi[a] - X[a] - Y[a]));
                }
                dom = sdiff <= -kListMargin;
            }
            if (!dom) {
                if (nk < kListLen) {
                    const int di = X[0] - c[0] + 8, dj = X[1] - c[1] + 8, dk = X[2] - c[2] + 8;
                    if ((unsigned)di > 15u || (unsigned)dj > 15u || (unsigned)dk > 15u) overflow = true;      // cannot happen for a range < 7.5 cells
                    kept[nk] = pk;
                    lists[t * kListLen + nk] = (unsigned short)((uint32_t)di | ((uint32_t)dj << 4) | ((uint32_t)dk << 8) | (o == 0 ? kListNoEmit : 0u));
                    ++nk;
                } else {
                    overflow = true;
                }
            }
        }
        const bool left_near = X[axis] != c[axis] ? c[axis] < X[axis] : !((oct >> axis) & 1);
        const uint32_t nl = nn >> 1, nr = nn - nl - 1u;
        uint32_t near_o, near_n, far_o, far_n;
        if (left_near) { near_o = o + 1u; near_n = nl; far_o = o + 1u + nl; far_n = nr; }
        else           { near_o = o + 1u + nl; near_n = nr; far_o = o + 1u; far_n = nl; }
        const unsigned long long P = (unsigned long long)X[axis];
        axis = (axis == 2u ? 0u : axis + 1u);
        if (far_n > 0 && sp < 28) st[sp++] = (unsigned long long)far_o | ((unsigned long long)far_n << 25) | ((unsigned long long)axis << 50) | (P << 52);
        else if (far_n > 0) overflow = true;
        o = near_o; nn = near_n;
    }
    if (nk < kListLen) lists[t * kListLen + nk] = (unsigned short)kListEnd;
    if (overflow) lists[t * kListLen] = (unsigned short)kListOverflow;
}

// What k_deposit does for one particle, straight after its walk and with plain global atomics: the candidate lists' leftovers are a few
// hundred particles (within 8e-6 dx of a cell face), for which a second, latency-bound launch with its own aggregation table cost more
// than the walk itself.  pvol_acc == nullptr: the walk only parks the squared distances (k_deposit follows).
struct WalkDeposit { GaussParams gp; CellWindow cw; double* pvol_acc; double* up_acc; unsigned char* touched; };
__device__ __attribute__((noinline)) void walk_deposit(const ParticleSoA& p, int64_t i, int chain, const WalkDeposit& wd) {
    const int k = stencil_span(chain).k;                              // last push first below: ascending d2
    if (k <= 0) return;
    const double dia = 2 * p.rad[i];                                  // FoamYade.C:219
    const double pVol = M_PI * cube3(dia) / 6.0;                      // FoamYade.H:36 (as k_locate_deposit forms it)
    const double vx = p.vx[i], vy = p.vy[i], vz = p.vz[i];
    double allwt = 0.0;                                               // calcInterpWeightGaussian FoamYade.C:301-314, ascending-d2 order
#pragma unroll 1
    for (int t = 0; t < k; ++t) {
        const size_t slot = stencil_slot(p, i, chain - 1 - t);
        const double wt = gauss_wu(wd.gp, p.w[slot]);
        p.w[slot] = wt;
        allwt += wt;
    }
    const double rallwt_ = 1.0 / allwt;
#pragma unroll 1
    for (int t = 0; t < k; ++t) {
        const size_t slot = stencil_slot(p, i, chain - 1 - t);
        const double weight = p.w[slot] * rallwt_;                    // FoamYade.C:312-314
        p.w[slot] = weight;
        const int64_t cl = (int64_t)p.ids[slot] - wd.cw.base;         // storage index (slab window)
        if (cl < 0 || cl >= wd.cw.n_field) continue;
        atomic_add_f64(&wd.pvol_acc[cl], pVol * weight);              // buildCellPartList FoamYade.C:265-288
        atomic_add_f64(&wd.up_acc[3 * (size_t)cl + 0], (weight * vx) * pVol);
        atomic_add_f64(&wd.up_acc[3 * (size_t)cl + 1], (weight * vy) * pVol);
        atomic_add_f64(&wd.up_acc[3 * (size_t)cl + 2], (weight * vz) * pVol);
        wd.touched[cl] = 1;
    }
}

// WD: the walk also deposits for the particle it has placed (the leftovers of the candidate lists); without it the instance carries neither the 16 weights' scratch (192 B per
// lane) nor their registers: the explicit walk 97 -> 42 VGPRs
template <bool IMPLICIT, bool WD, bool WIDE = false>
__global__ __launch_bounds__(kWave) void k_locate(const KdNode* __restrict__ tree, const uint32_t* __restrict__ packed, ImplicitGeom ig,
                                                  int32_t n_cells, ParticleSoA p, int64_t n, double maxdist,
                                                  const unsigned long long* __restrict__ start, SlabOwn own,
                                                  const int32_t* __restrict__ work, const unsigned int* __restrict__ work_n, WalkDeposit wd,
                                                  int stack_cap, int32_t* __restrict__ ovf_list, unsigned int* __restrict__ ovf_count, unsigned int* __restrict__ depth_hwm) {
    // ovf_list != null: the LDS stack holds stack_cap entries per lane only (more waves per CU: the kernel is latency bound); a walk that would need more is given up and its
    // particle filed in ovf_list for a second launch with the full depth -- every particle is walked from its start by exactly one of the two, so the chains are the same
    static_assert(!(IMPLICIT && WIDE), "implicit entries are 8 bytes");
    typedef typename StackEntry<IMPLICIT, WIDE>::type entry_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char stack_raw[];
    entry_t* stack = reinterpret_cast<entry_t*>(stack_raw);
#define STK(sp_) stack[(sp_) * kWave + lane]
    const int lane = threadIdx.x;
    // work list (k_locate_lists' leftovers): the waves share its entries evenly; otherwise a wave owns kLocPPB consecutive particles
    int64_t per = (n + gridDim.x - 1) / gridDim.x, base = (int64_t)blockIdx.x * per;      // (kLocPPB for a large cloud; fewer per wave when the cloud is small: locate_grid)
    if (work) { n = (int64_t)*work_n; per = (n + gridDim.x - 1) / gridDim.x; base = (int64_t)blockIdx.x * per; }
    const int64_t end = (base + per < n) ? base + per : n;
    int64_t next = base;                               // wave-uniform cursor into [base, end)
    const NodeVal root = fetch_node<IMPLICIT>(tree, packed, ig, 0u);
    const double hdx = 0.5 * ig.dx;

    bool active = false;
    int64_t i = 0;
    double qx = 0, qy = 0, qz = 0, best = 0;
    int chain = 0, sp = 0, spmax = 0;
    uint32_t o = 0, nn = 0, axis = 0;
    for (;;) {
        // ---- hand new particles to idle lanes (batched: the refill code is wave-wide, so wait until it pays)
        const unsigned long long idle = __ballot(!active);
        const int n_idle = __popcll(idle);
        if (next < end && (n_idle >= kLocRefill || n_idle == kWave)) {
            const int rank = __popcll(idle & ((1ull << lane) - 1ull));
            const int64_t cand = next + rank;
            if (!active && cand < end) {
                i = work ? (int64_t)work[cand] : cand;
                qx = p.px[i]; qy = p.py[i]; qz = p.pz[i];
                // meshTree.C:156: dist = distance(root->p, px); the root itself can never enter the queue (x < x is false)
                const double a = qx - root.x, b = qy - root.y, c = qz - root.z;
                best = a * a;
                best += b * b;
                best += c * c;
                // Round 4: the walk starts from best = min(|q - root|^2, maxdist).  The chain is the same: a centre is queued iff it is nearer than maxdist AND than every
                // centre visited before it (meshTree.C:192-196), and centres at or beyond maxdist -- the only ones a smaller starting bound hides, in the subtrees whose
                // split plane is at least sqrt(maxdist) away -- can neither be queued nor outbid one that is.  What changes is the stack: the far sides of the top levels,
                // pushed while `best` is still the distance to some far ancestor and dropped again at their pop, are not pushed at all
                best = fmin(best, maxdist);
                chain = 0; sp = 0; spmax = 0; o = 0; nn = (uint32_t)n_cells; axis = 0;
                if constexpr (IMPLICIT) {
                    if (start) {                                 // skip the levels the query's cell determines (k_build_locate_start)
                        const double fx = floor((qx - ig.ox) / ig.dx), fy_ = floor((qy - ig.oy) / ig.dx), fz = floor((qz - ig.oz) / ig.dx);
                        if (fx >= 0 && fx < ig.nx && fy_ >= 0 && fy_ < ig.ny && fz >= 0 && fz < ig.nz) {
                            const unsigned long long e = start[(size_t)fx + (size_t)ig.nx * ((size_t)fy_ + (size_t)ig.ny * (size_t)fz)];
                            o = (uint32_t)(e & 0x1ffffffull); nn = (uint32_t)((e >> 25) & 0x1ffffffull); axis = (uint32_t)((e >> 50) & 3ull);
                            if (o != 0) best = maxdist;          // no ancestor was within maxdist: same chain as any best >= maxdist, and no far side beyond it is stacked
                        }
                    }
                }
                active = true;
                if (own.active) {                                // another slab's particle: not located here (k = 0)
                    int kz = (int)floor((qz - own.oz) / own.dx);
                    kz = min(max(kz, 0), own.nzglob - 1);
                    if (!(qz == qz) || !own_planes(own, p.orig[i], kz, qx, qy, qz)) { p.chain_len[i] = 0; active = false; }
                }
            }
            next += n_idle;
        } else if (n_idle == kWave) {
            break;                                       // nothing running, nothing left
        }
        if (active) {
            if (nn == 0) {
                // up to two pops per iteration: most popped far sides fail df2 < best and would waste the visit slot
                for (int attempt = 0; attempt < 2; ++attempt) {
                    if (nn != 0) break;
                    if (sp == 0) {
                        if (active) {                                          // walk finished; k = min(chain, 16)
                            p.chain_len[i] = chain; active = false;
                            if constexpr (WD) walk_deposit(p, i, chain, wd);
                            if (depth_hwm && (i & 63) == 0) atomicAdd(&depth_hwm[min(spmax, kLocDepthBins - 1)], 1u);      // (one walk in 64: a histogram of the stack depths)
                        }
                        break;
                    }
                    --sp;
                    const entry_t e = STK(sp);
                    double df2;
                    uint32_t eo, en, ea;
                    if constexpr (IMPLICIT) {
                        eo = (uint32_t)(e & 0x1ffffffull); en = (uint32_t)((e >> 25) & 0x1ffffffull); ea = (uint32_t)((e >> 50) & 3ull);
                        const int idx = (int)(e >> 52);
                        const uint32_t pa = (ea == 0 ? 2u : ea - 1u);               // the parent's split axis
                        const double org = (pa == 0 ? ig.ox : (pa == 1 ? ig.oy : ig.oz));
                        const double qq = (pa == 0 ? qx : (pa == 1 ? qy : qz));
                        const double df = (org + (double)(2 * idx + 1) * hdx) - qq;
                        df2 = df * df;
                    } else if constexpr (WIDE) {
                        eo = e.x; en = e.y & 0x3fffffffu; ea = e.y >> 30;
                        df2 = __hiloint2double((int)e.w, (int)e.z);
                    } else {
                        eo = (uint32_t)(e & 0x1ffffffull); en = (uint32_t)((e >> 25) & 0x1ffffffull); ea = (uint32_t)((e >> 50) & 3ull);
                        df2 = (double)(uint32_t)(e >> 52) * (maxdist * (1.0 / 4095.0));      // the lower bound
                    }
                    if (df2 < best) { o = eo; nn = en; axis = ea; }                  // meshTree.C:225, evaluated when the near subtree has returned
                }
            }
            if (active && nn != 0) {
                uint32_t pk = 0;
                NodeVal nd;
                if constexpr (IMPLICIT) {
                    pk = packed[o];
                    const int ci = (int)(pk & 1023u), cj = (int)((pk >> 10) & 1023u), ck = (int)(pk >> 20);
                    // (2i + 1) * (dx / 2) is the same real number as (i + 0.5) * dx and both factors are exact, so the rounded
                    // product is the same double: one FP64 add less per axis
                    nd.x = ig.ox + (double)(2 * ci + 1) * hdx;
                    nd.y = ig.oy + (double)(2 * cj + 1) * hdx;
                    nd.z = ig.oz + (double)(2 * ck + 1) * hdx;
                    nd.id = ci + ig.nx * (cj + ig.ny * ck);
                } else {
                    nd = fetch_node<false>(tree, packed, ig, o);
                }
                const double a = qx - nd.x, b = qy - nd.y, c = qz - nd.z;
                const double aa = a * a, bb = b * b, cc = c * c;
                double d = aa;                       // meshTree.C:54-64: dist += ds*ds over x, y, z
                d += bb;
                d += cc;
                if (d < best) {                      // meshTree.C:192 (and the re-push on return is a no-op: same id)
                    best = d;
                    if (d < maxdist) {               // meshTree.C:195
                        const size_t slot = stencil_slot(p, i, chain);
                        p.ids[slot] = nd.id;
                        p.w[slot] = d;               // squared distance parked here until k_deposit forms the weights
                        ++chain;
                    }
                }
                // meshTree.C:200: df = node[axis] - q[axis] = -(q[axis] - node[axis]) exactly, so df*df is the squared term already
                // formed for the distance and df > 0 <=> (q - node)[axis] < 0 -- same bits, three subtractions and a multiply fewer
                const double mdf = (axis == 0 ? a : (axis == 1 ? b : c));
                const double df2 = mdf * mdf;        // == aa / bb / cc of that axis, one multiply instead of a second three-way select
                const uint32_t nl = nn >> 1, nr = nn - nl - 1;
                uint32_t near_o, near_n, far_o, far_n;
                if (mdf < 0.0) { near_o = o + 1; near_n = nl; far_o = o + 1 + nl; far_n = nr; }     // meshTree.C:206-208
                else          { near_o = o + 1 + nl; near_n = nr; far_o = o + 1; far_n = nl; }      // meshTree.C:209-212
                const uint32_t paxis = axis;
                axis = (axis == 2 ? 0 : axis + 1);
                // best only decreases, so a far side that already fails df2 < best can never pass later
                const bool push = far_n > 0 && df2 < best;
                const bool ovf = push && ovf_list && sp >= stack_cap;
                if (ovf_list) {                          // (kernel-uniform) the lanes that give up file their particles with ONE atomic per wave and iteration
                    const unsigned long long m = __ballot(ovf);
                    if (m) {
                        const int leader = __ffsll((long long)m) - 1;
                        unsigned int at = 0;
                        if (lane == leader) at = atomicAdd(ovf_count, (unsigned int)__popcll(m));
                        at = __shfl(at, leader, kWave);
                        if (ovf) { ovf_list[at + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)i; active = false; }
                    }
                }
                if (push && !ovf) {
                    if constexpr (IMPLICIT) {
                        const unsigned long long idx = (paxis == 0 ? (pk & 1023u) : (paxis == 1 ? ((pk >> 10) & 1023u) : (pk >> 20)));
                        STK(sp) = (unsigned long long)far_o | ((unsigned long long)far_n << 25) | ((unsigned long long)axis << 50) | (idx << 52);
                    } else if constexpr (WIDE) {
                        uint4 e;
                        e.x = far_o; e.y = far_n | (axis << 30);
                        e.z = (uint32_t)__double2loint(df2); e.w = (uint32_t)__double2hiint(df2);
                        STK(sp) = e;
                    } else {
                        const int t = max((int)(df2 * (4095.0 / maxdist)) - 1, 0);          // df2 < best <= maxdist: t <= 4094; one unit of slack against the rounding of the product
                        STK(sp) = (unsigned long long)far_o | ((unsigned long long)far_n << 25) | ((unsigned long long)axis << 50) | ((unsigned long long)t << 52);
                    }
                    ++sp;
                    spmax = max(spmax, sp);
                }
                o = near_o; nn = near_n;
            }
        }
    }
#undef STK
}

// ------------------------------------------------------------------------------------------------ nearest cell
// meshTree::nearestCell (meshTree.C:66-135): plain nearest-neighbour descent of the same tree -- near side first, far side iff
// df^2 < best, strict improvements only, so among equidistant centres the first one in depth-first order wins.  The reference never calls
// it; it is the natural findCell stand-in on meshes where the nearest centre is the containing cell.  One lane per
// query, explicit stack in scratch (tree depth <= 25); far sides that cannot pass `df2 < best` any more are dropped at push time.
template <bool IMPLICIT>
__global__ __launch_bounds__(256) void k_nearest_cell(const KdNode* __restrict__ tree, const uint32_t* __restrict__ packed, ImplicitGeom ig, int32_t n_cells,
                                                      const double* __restrict__ pos, int64_t n, int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double qx = pos[3 * i], qy = pos[3 * i + 1], qz = pos[3 * i + 2];
    uint32_t st_o[28], st_n[28];
    double st_d[28];
    unsigned char st_a[28];
    int sp = 0;
    const NodeVal root = fetch_node<IMPLICIT>(tree, packed, ig, 0u);
    double best;
    {
        const double a = qx - root.x, b = qy - root.y, c = qz - root.z;
        best = a * a; best += b * b; best += c * c;                 // meshTree.C:71: dist = distance(root->p, v)
    }
    int32_t best_id = root.id;
    uint32_t o = 0, nn = (uint32_t)n_cells, axis = 0;
    for (;;) {
        if (nn == 0) {
            if (sp == 0) break;
            --sp;
            if (!(st_d[sp] < best)) continue;                       // meshTree.C:121, evaluated when the near subtree has returned
            o = st_o[sp]; nn = st_n[sp]; axis = st_a[sp];
        }
        const NodeVal nd = fetch_node<IMPLICIT>(tree, packed, ig, o);
        const double a = qx - nd.x, b = qy - nd.y, c = qz - nd.z;
        double d = a * a;                                           // meshTree.C:54-64
        d += b * b;
        d += c * c;
        if (d < best) { best = d; best_id = nd.id; }                // meshTree.C:90-93 (and the comparisons on return: same node, same distance)
        const double mdf = axis == 0 ? a : (axis == 1 ? b : c);     // -(node[axis] - q[axis])
        const double df2 = mdf * mdf;
        const uint32_t nl = nn >> 1, nr = nn - nl - 1;
        uint32_t near_o, near_n, far_o, far_n;
        if (mdf < 0.0) { near_o = o + 1; near_n = nl; far_o = o + 1 + nl; far_n = nr; }     // df > 0: left first (meshTree.C:104-110)
        else          { near_o = o + 1 + nl; near_n = nr; far_o = o + 1; far_n = nl; }
        axis = (axis == 2 ? 0 : axis + 1);
        if (far_n > 0 && df2 < best && sp < 28) { st_o[sp] = far_o; st_n[sp] = far_n; st_d[sp] = df2; st_a[sp] = (unsigned char)axis; ++sp; }
        o = near_o; nn = near_n;
    }
    out[i] = best_id;
}

// register budget of k_locate_deposit (a build-time constant; tools/build_variant.sh overrides it for A/B runs): room for 8 waves per SIMD (56 VGPRs as it
// stands; the cap also keeps the scalar registers at 78 -- with its natural 100 the hardware admits three workgroups per CU instead of four)
#ifndef FY_LD_ATTR
#define FY_LD_ATTR __attribute__((amdgpu_waves_per_eu(8)))
#endif
// ---- quad-lane exchange without the LDS: v_mov_b32 under a DPP quad_perm control -- every lane reads lane J of its own quad.  All four lanes of the
// quad must be active at the call (a disabled source lane reads as zero).
template <int J> __device__ __forceinline__ int quad_bcast(int v) { return __builtin_amdgcn_mov_dpp(v, J * 0x55, 0xf, 0xf, true); }
// 4 x 4 transpose inside every quad, one dword per (lane, register): on entry register r of lane q holds M[q][r], on return register w of lane j
// holds M[w][j].  Two butterfly stages (lane ^ 1 on the register pairs (0,1), (2,3); lane ^ 2 on (0,2), (1,3)), each a select of what to send, one DPP
// move and two selects of what to keep: 16 VALU operations per dword against 28 for "broadcast each source lane, pick mine".
__device__ __forceinline__ void quad_transpose(uint32_t& m0, uint32_t& m1, uint32_t& m2, uint32_t& m3, bool b0, bool b1) {
    constexpr int kXor1 = 1 | (0 << 2) | (3 << 4) | (2 << 6), kXor2 = 2 | (3 << 2) | (0 << 4) | (1 << 6);
    uint32_t t;
    t = (uint32_t)__builtin_amdgcn_mov_dpp((int)(b0 ? m0 : m1), kXor1, 0xf, 0xf, true); m0 = b0 ? t : m0; m1 = b0 ? m1 : t;
    t = (uint32_t)__builtin_amdgcn_mov_dpp((int)(b0 ? m2 : m3), kXor1, 0xf, 0xf, true); m2 = b0 ? t : m2; m3 = b0 ? m3 : t;
    t = (uint32_t)__builtin_amdgcn_mov_dpp((int)(b1 ? m0 : m2), kXor2, 0xf, 0xf, true); m0 = b1 ? t : m0; m2 = b1 ? m2 : t;
    t = (uint32_t)__builtin_amdgcn_mov_dpp((int)(b1 ? m1 : m3), kXor2, 0xf, 0xf, true); m1 = b1 ? t : m1; m3 = b1 ? m3 : t;
}
__device__ __forceinline__ void quad_transpose(uint4& m0, uint4& m1, uint4& m2, uint4& m3, int lq) {
    const bool b0 = lq & 1, b1 = lq & 2;
    quad_transpose(m0.x, m1.x, m2.x, m3.x, b0, b1); quad_transpose(m0.y, m1.y, m2.y, m3.y, b0, b1);
    quad_transpose(m0.z, m1.z, m2.z, m3.z, b0, b1); quad_transpose(m0.w, m1.w, m2.w, m3.w, b0, b1);
}
__device__ __forceinline__ double2 as_double2(uint4 v) {
    return make_double2(__hiloint2double((int)v.y, (int)v.x), __hiloint2double((int)v.w, (int)v.z));
}

// buildCellPartList FoamYade.C:265-288: pVol*w and (w*v)*pVol per (particle, cell) pair into the per-batch accumulators
#ifndef FY_DEP_THREADS
#define FY_DEP_THREADS 512
#endif
#ifndef FY_DEP_LOG2
#define FY_DEP_LOG2 10
#endif
constexpr int kDepThreads = FY_DEP_THREADS, kDepLog2 = FY_DEP_LOG2;      // 1024 slots x (4 + 32) B = 36 KiB of LDS (2048: 1.46 vs 1.36 ms for k_locate_deposit -- occupancy)
static_assert(kDepThreads == kOrderRun, "the runs that launch_order_blocks_by_chain orders are the locate's workgroups");
// table crowded (practically never): straight to memory.  Out of line -- k_locate_deposit inlines deposit_pair 24 times
__device__ __attribute__((noinline)) void deposit_direct(int32_t cid, double c0, double c1, double c2, double c3, double* __restrict__ pvol_acc,
                                                         double* __restrict__ up_acc, unsigned char* __restrict__ touched) {
    atomic_add_f64(&pvol_acc[cid], c0);
    atomic_add_f64(&up_acc[3 * (size_t)cid + 0], c1);
    atomic_add_f64(&up_acc[3 * (size_t)cid + 1], c2);
    atomic_add_f64(&up_acc[3 * (size_t)cid + 2], c3);
    touched[cid] = 1;
}

// one (particle, cell) contribution into the workgroup's table (or straight to memory when the table is crowded)
__device__ __forceinline__ void deposit_pair(uint32_t* keys, double* vals, int32_t cid, double c0, double c1, double c2, double c3,
                                             double* __restrict__ pvol_acc, double* __restrict__ up_acc, unsigned char* __restrict__ touched) {
    const int h = agg_slot<kDepLog2>(keys, (uint32_t)cid);
    if (h >= 0) {
        // the LDS atomic unit (~1.4 ds_add_f64 lanes per clock per CU, tools/micro/lds_atomic_rate.hip) is what bounds this half of the
        // kernel: adding an exact zero is the identity, so the momentum terms of a particle at rest are not issued at all
        constexpr int N = 1 << kDepLog2;
        lds_add_f64(&vals[agg_at<N>(h, 0)], c0);
        if (c1 != 0.0) lds_add_f64(&vals[agg_at<N>(h, 1)], c1);
        if (c2 != 0.0) lds_add_f64(&vals[agg_at<N>(h, 2)], c2);
        if (c3 != 0.0) lds_add_f64(&vals[agg_at<N>(h, 3)], c3);
    } else {
        deposit_direct(cid, c0, c1, c2, c3, pvol_acc, up_acc, touched);
    }
}
// work != nullptr: the particles listed there (k_locate_deposit's leftovers, placed by the walk), shared by a fixed grid
#ifndef FY_DEP_ATTR
#define FY_DEP_ATTR
#endif
__global__ __launch_bounds__(kDepThreads) FY_DEP_ATTR void k_deposit(ParticleSoA p, int64_t n, GaussParams gp, CellWindow cw, double* __restrict__ pvol_acc,
                                                          double* __restrict__ up_acc, unsigned char* __restrict__ touched,
                                                          const int32_t* __restrict__ work, const unsigned int* __restrict__ work_n, TileBuckets tb) {
    __shared__ uint32_t keys[1 << kDepLog2];
    __shared__ double vals[(1 << kDepLog2) * 4];
    __shared__ TileMapLds tmap;
    if (work) { n = (int64_t)*work_n; if ((int64_t)blockIdx.x * kDepThreads >= n) return; }      // (block-uniform)
    table_clear<(1 << kDepLog2), kDepThreads, 4>(keys, vals);
    __syncthreads();
    for (int64_t idx = (int64_t)blockIdx.x * kDepThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kDepThreads) {
        const int64_t i = work ? (int64_t)work[idx] : idx;
        const StencilSpan sp = stencil_span(p.chain_len[i]);
        const int chain = sp.chain, k = sp.k;
        if (k > 0) {
            const double dia = 2 * p.rad[i];                                  // FoamYade.C:219
            const double pVol = M_PI * cube3(dia) / 6.0;                      // FoamYade.H:36 (as k_locate_deposit forms it)
            const double vx = p.vx[i], vy = p.vy[i], vz = p.vz[i];
            // calcInterpWeightGaussian FoamYade.C:301-314, slots visited in ascending-d2 order (= reverse push order).  Round 6: the unnormalised weights no longer stay in 16
            // register pairs across the deposit loop (113 -> 70 VGPRs: three workgroups per CU instead of two, and the kernel waits on memory 71 % of its wave cycles: 1.18 ->
            // 1.09 ms); the loop below reads each squared distance again (cached), forms the same weight again, scales it and stores the normalised weight -- the same products.
            // (waves_per_eu(8) -- 64 VGPRs, four workgroups -- spills 32 B and is slower: 1.16.)
            double allwt = 0.0;
#pragma unroll
            for (int t = 0; t < kMaxK; ++t) {
                if (t < k) {
                    allwt += gauss_wu(gp, p.w[stencil_slot(p, i, chain - 1 - t)]);
                }
            }
            const double rallwt_ = 1.0 / allwt;
            size_t slot = stencil_slot(p, i, chain - 1);
            double w_next = p.w[slot];
            int32_t id_next = p.ids[slot];
#pragma unroll 1
            for (int t = 0; t < k; ++t) {
                const double weight = gauss_wu(gp, w_next) * rallwt_;
                const int64_t cl = (int64_t)id_next - cw.base;                // storage index (slab window)
                p.w[slot] = weight;
                if (t + 1 < k) {
                    slot = stencil_slot(p, i, chain - 2 - t);
                    w_next = p.w[slot]; id_next = p.ids[slot];
                }
                if (cl < 0 || cl >= cw.n_field) continue;
                const int32_t cid = (int32_t)cl;
                const double c0 = pVol * weight, c1 = (weight * vx) * pVol, c2 = (weight * vy) * pVol, c3 = (weight * vz) * pVol;
                deposit_pair(keys, vals, cid, c0, c1, c2, c3, pvol_acc, up_acc, touched);
            }
        }
    }
    __syncthreads();
    flush_table<(1 << kDepLog2), kDepThreads, 4>(keys, vals, tmap, tb, pvol_acc, up_acc, touched);
}

// k_locate_lists and k_deposit in one pass over the particles: the list scan keeps the unnormalised Gaussian weight of every listed
// node in a register (zero where the node did not enter the chain; slots are static because the scan is unrolled), so the chain's
// squared distances never travel through memory: ids and NORMALISED weights are stored once, for k_force_gaussian.  Same arithmetic
// as the two kernels: allwt adds the weights from the last push to the first (adding the zeros in between is exact).
// rec != nullptr: the binned SoA arrays are not filled yet -- the lane fetches its wire record through the placement (p.orig) itself and
// leaves the SoA copy behind for the force pass (k_bin_gather folded into this kernel: one launch and one coalesced read of the SoA less;
// the record fetch is the same random 80-byte read either way)
// This kernel's register allocation follows the order its expressions are first written in: with table_clear, stencil_span or stencil_slot in the places
// marked "own text" below it compiles to other code (57 VGPRs for 56).  Those places keep the expressions the helpers state; the other uses are the helpers.
__global__ __launch_bounds__(kDepThreads) FY_LD_ATTR void k_locate_deposit(LocateLists ll, ImplicitGeom ig, ParticleSoA p, int64_t n,
                                                                 GaussParams gp, SlabOwn own, CellWindow cw, double* __restrict__ pvol_acc,
                                                                 double* __restrict__ up_acc, unsigned char* __restrict__ touched, TileBuckets tb,
                                                                 const double* __restrict__ rec) {
    const unsigned short* __restrict__ lists = ll.lists;
    int32_t* __restrict__ fb_list = ll.fb_list;
    unsigned int* __restrict__ fb_count = ll.fb_count;
    __shared__ uint32_t keys[1 << kDepLog2];
    __shared__ double vals[(1 << kDepLog2) * 4];
    __shared__ TileMapLds tmap;
    for (int q = threadIdx.x; q < (1 << kDepLog2); q += kDepThreads) {      // table_clear (own text)
        keys[q] = kAggEmpty;
        vals[q] = 0.0; vals[q + (1 << kDepLog2)] = 0.0; vals[q + 2 * (1 << kDepLog2)] = 0.0; vals[q + 3 * (1 << kDepLog2)] = 0.0;
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kDepThreads + threadIdx.x;
    // an 80-byte record of a 16-byte aligned array is five aligned 16-byte words, of which this kernel wants words 0, 1, 2 and 4
    const bool rec16 = rec && (reinterpret_cast<uintptr_t>(rec) & 15) == 0;      // (uniform)
    // the four lanes of a quad fetch one record per instruction (lane q: word q, lane 3: word 4) -- a wave instruction looks up 16 record
    // starts instead of 64 -- and the words go home to the record's lane by DPP quad_perm moves (same values, no arithmetic involved)
    double2 qa = make_double2(0, 0), qb = qa, qc = qa, qe = qa;
    if (rec16) {
        const int lq = (int)(threadIdx.x & 3u);
        const int32_t o = i < n ? p.orig[i] : 0;
        const uint4* r4 = reinterpret_cast<const uint4*>(rec) + (lq < 3 ? lq : 4);
        uint4 g0 = r4[5 * (size_t)quad_bcast<0>(o)], g1 = r4[5 * (size_t)quad_bcast<1>(o)], g2 = r4[5 * (size_t)quad_bcast<2>(o)],
              g3 = r4[5 * (size_t)quad_bcast<3>(o)];      // round j: the quad's four words of lane j's record
        quad_transpose(g0, g1, g2, g3, lq);              // -> register w: word w (lane 3's: word 4) of MY record
        qa = as_double2(g0); qb = as_double2(g1); qc = as_double2(g2); qe = as_double2(g3);
    }
    // Straight-line (predicated) down to the list row, so that the four lanes of a quad are still together when the rows are fetched
    const bool live = i < n;
    double qx = 0, qy = 0, qz = 0, pvx = 0, pvy = 0, pvz = 0, prad = 0;
    if (live) {
        if (rec) {
            const double* r = rec + 10 * (size_t)p.orig[i];
            if (rec16) {
                const double2 a = qa, b = qb, cc = qc, e = qe;
                qx = a.x; qy = a.y; qz = b.x; pvx = b.y; pvy = cc.x; pvz = cc.y; prad = e.y;
            } else {
                qx = r[0]; qy = r[1]; qz = r[2]; pvx = r[3]; pvy = r[4]; pvz = r[5]; prad = r[9];
            }
            p.px[i] = qx; p.py[i] = qy; p.pz[i] = qz; p.vx[i] = pvx; p.vy[i] = pvy; p.vz[i] = pvz; p.rad[i] = prad;
        } else {
            qx = p.px[i]; qy = p.py[i]; qz = p.pz[i]; pvx = p.vx[i]; pvy = p.vy[i]; pvz = p.vz[i]; prad = p.rad[i];
        }
    }
    bool mine = live;
    if (live && own.active) {                                // another slab's particle: not located here (k = 0)
        int kz = (int)floor((qz - own.oz) / own.dx);
        kz = min(max(kz, 0), own.nzglob - 1);
        if (!(qz == qz) || !own_planes(own, p.orig[i], kz, qx, qy, qz)) { p.chain_len[i] = 0; mine = false; }
    }
    const double hdx = 0.5 * ig.dx;
    // Reciprocals instead of FP64 divisions (round 5; ~35 instructions each, 22 per particle: same-box A/B 1.167 -> 1.127 ms).  What they may move by an
    // ulp cannot change an answer: the lattice coordinate only picks the (cell, octant) list, and a particle within 2 kListEps of a cell face goes to
    // the walk anyway; the Gaussian's argument and the normalisation feed weights that are held to 1e-10, not to the bit.  Every comparison that steers
    // the chain (d < best, d < maxdist) is formed exactly as the reference forms it.
    const double rdx_ = 1.0 / ig.dx;
    const double sx = (qx - ig.ox) * rdx_, sy = (qy - ig.oy) * rdx_, sz = (qz - ig.oz) * rdx_;
    const double fx = floor(sx), fy_ = floor(sy), fz = floor(sz);
    const double tx = sx - fx, ty = sy - fy_, tz = sz - fz;
    const double tlo = 2 * kListEps, thi = 1.0 - 2 * kListEps;
    int sclass = 0;
    bool ok = mine && fx >= 0 && fx < ig.nx && fy_ >= 0 && fy_ < ig.ny && fz >= 0 && fz < ig.nz &&
              tx >= tlo && tx <= thi && ty >= tlo && ty <= thi && tz >= tlo && tz <= thi;      // (false for NaN)
    const int ci = ok ? (int)fx : 0, cj = ok ? (int)fy_ : 0, ck = ok ? (int)fz : 0;
    uint4 v[kListLen / 8];
#pragma unroll
    for (int ch = 0; ch < kListLen / 8; ++ch) v[ch] = make_uint4(kListEnd | (kListEnd << 16), 0, 0, 0);
    int32_t rowi = 0;                                        // (cell, octant) row of the lists; row 0 where there is none to fetch
    {
        const double cx = ig.ox + (double)(2 * ci + 1) * hdx, cy = ig.oy + (double)(2 * cj + 1) * hdx, cz = ig.oz + (double)(2 * ck + 1) * hdx;
        const int oct = (qx - cx < 0.0 ? 0 : 1) | (qy - cy < 0.0 ? 0 : 2) | (qz - cz < 0.0 ? 0 : 4);
        const int64_t cell = (int64_t)ci + (int64_t)ig.nx * ((int64_t)cj + (int64_t)ig.ny * (int64_t)ck) - ll.cell0;
        ok = ok && cell >= 0 && cell < ll.n_listed;          // (a slab lists its own planes only)
        if (ok) rowi = (int32_t)(cell * 8 + oct);
    }
    {
        // all three 16-byte chunks of the row at once (one or two lines): fetched only where the list goes on, the second and the third each cost
        // the wave a dependent memory round trip (round 5); what lies behind a list's end mark is never looked at
        const uint4* __restrict__ L4 = reinterpret_cast<const uint4*>(lists);
        static_assert(kListLen * sizeof(unsigned short) == 3 * sizeof(uint4), "a list row is three 16-byte words");
        // quad-cooperative as the record fetch above: round j, lanes 0..2 fetch their word of quad lane j's row (48 contiguous bytes per quad and
        // instruction instead of 16 bytes from each of four rows), lane 3 fetches nothing; then the 4 x 4 transpose
        const int lq = (int)(threadIdx.x & 3u);
        uint4 c0 = make_uint4(0, 0, 0, 0), c1 = c0, c2 = c0, c3 = c0;
        const int32_t w0 = quad_bcast<0>(rowi), w1 = quad_bcast<1>(rowi), w2 = quad_bcast<2>(rowi), w3 = quad_bcast<3>(rowi);
        if (lq < 3) { c0 = L4[3 * (size_t)w0 + lq]; c1 = L4[3 * (size_t)w1 + lq]; c2 = L4[3 * (size_t)w2 + lq]; c3 = L4[3 * (size_t)w3 + lq]; }
        quad_transpose(c0, c1, c2, c3, lq);              // -> c0, c1, c2: the three words of MY row (c3: lane 3's, nothing)
        if (ok) {
            v[0] = c0;
            ok = (c0.x & 0xffffu) != kListOverflow;
            if (ok && (c0.w >> 16) != kListEnd) { v[1] = c1; sclass = 1; if ((c1.w >> 16) != kListEnd) { v[2] = c2; sclass = 2; } }
        }
    }
    if (mine) {
        {
            if (p.scan_class) p.scan_class[i] = (unsigned char)(ok ? sclass : 2);
            if (!ok) {
                const unsigned int at = atomicAdd(fb_count, 1u);
                fb_list[at] = (int32_t)i;
            } else {
                // The scan keeps nothing per list position: an entry that enters the chain has its id and its UNNORMALISED weight stored at once, in the row of its push
                // index; the sum (last push first, FoamYade.C:301-311: the same additions as over the 24 positions with their zeros) and the normalisation + deposit
                // then run as loops over the CHAIN (k entries) that read the rows back (this lane's own stores: L2) -- not as 24 unrolled, mostly idle copies
                // of the deposit, and without 24 weights held in registers
                double best = 1e300;
                int pos = 0;
                bool done = false;
#pragma unroll
                for (int h = 0; h < kListLen; ++h) {
                    const uint4 vv = v[h >> 3];
                    const uint32_t wd = ((h >> 1) & 3) == 0 ? vv.x : (((h >> 1) & 3) == 1 ? vv.y : (((h >> 1) & 3) == 2 ? vv.z : vv.w));
                    const uint32_t code = (wd >> ((h & 1) * 16)) & 0xffffu;
                    if (code == kListEnd) done = true;
                    if (!done) {
                        const int ni = ci + (int)(code & 15u) - 8, nj = cj + (int)((code >> 4) & 15u) - 8, nk = ck + (int)((code >> 8) & 15u) - 8;
                        const double a = qx - (ig.ox + (double)(2 * ni + 1) * hdx), b = qy - (ig.oy + (double)(2 * nj + 1) * hdx),
                                     c = qz - (ig.oz + (double)(2 * nk + 1) * hdx);
                        double d = a * a;                    // meshTree.C:54-64
                        d += b * b;
                        d += c * c;
                        if (d < best) {                      // meshTree.C:192
                            best = d;
                            if (d < gp.maxdist && !(code & kListNoEmit)) {       // meshTree.C:195; the root is never pushed
                                const size_t slot = stencil_slot(p, i, pos);
                                p.ids[slot] = ni + ig.nx * (nj + ig.ny * nk);
                                p.w[slot] = gauss_wu(gp, d);                     // FoamYade.C:308
                                ++pos;
                            }
                        }
                    }
                }
                const int chain = pos;
                p.chain_len[i] = chain;
                if (chain > 0) {
                    // stencil_span and stencil_slot of pushes chain - k + t, oldest first (own text down to the loop's first slot)
                    const int k = chain < kMaxK ? chain : kMaxK;      // (a chain longer than the ring has lost its oldest rows, as in the walk: k newest)
                    double allwt = 0.0;
                    {   // all the rows at once (one round trip), then the reference's order: last push first (FoamYade.C:301-311); rows beyond the chain read as zero,
                        // and adding them is exact -- the same additions as round 5's sum over the 24 list positions
                        double u[kMaxK];
#pragma unroll
                        for (int t = 0; t < kMaxK; ++t) u[t] = t < k ? p.w[(size_t)((chain - k + t) & (kMaxK - 1)) * p.cap + (size_t)i] : 0.0;
#pragma unroll
                        for (int t = kMaxK - 1; t >= 0; --t) allwt += u[t];
                    }
                    const double rallwt_ = 1.0 / allwt;
                    const double dia = 2 * prad;                                      // FoamYade.C:219
                    const double pVol = M_PI * cube3(dia) / 6.0;                      // FoamYade.H:36
                    const double vx = pvx, vy = pvy, vz = pvz;
                    size_t slot = (size_t)((chain - k) & (kMaxK - 1)) * p.cap + (size_t)i;
                    double w_n = p.w[slot];
                    int32_t id_n = p.ids[slot];
#pragma unroll 1
                    for (int t = chain - k; t < chain; ++t) {
                        const double weight = w_n * rallwt_;                          // FoamYade.C:312-314
                        const int32_t id_t = id_n;
                        p.w[slot] = weight;
                        if (t + 1 < chain) {                                          // (the next entry travels while this one goes through the table)
                            slot = stencil_slot(p, i, t + 1);
                            w_n = p.w[slot]; id_n = p.ids[slot];
                        }
                        const int64_t cl = (int64_t)id_t - cw.base;                   // storage index (slab window)
                        if (cl >= 0 && cl < cw.n_field) {
                            const double c0 = pVol * weight, c1 = (weight * vx) * pVol, c2 = (weight * vy) * pVol, c3 = (weight * vz) * pVol;
                            deposit_pair(keys, vals, (int32_t)cl, c0, c1, c2, c3, pvol_acc, up_acc, touched);
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    flush_table<(1 << kDepLog2), kDepThreads, 4>(keys, vals, tmap, tb, pvol_acc, up_acc, touched);
}

}  // namespace

int launch_build_locate_start(hipStream_t s, const uint32_t* packed, ImplicitGeom ig, int32_t n_cells, double maxdist, unsigned long long* start) {
    const double md_cells = (maxdist / (ig.dx * ig.dx)) * (1.0 + 1e-6);
    hipLaunchKernelGGL(k_build_locate_start, dim3(div_up(n_cells, 256)), dim3(256), 0, s, packed, ig, n_cells, md_cells, start);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

// waves of the walk: kLocPPB particles each for a large cloud; a small one is spread over up to 8192 waves (at least 64 particles each) instead of leaving most CUs idle --
// 300 000 particles on 293 waves took 0.74 ms, 2.5 us per particle against 0.41 at 10 M; particle phase on the explicit tree, same box, 1024 per wave / at most 2048 / 4096 /
// 8192 / 16384 waves: 300 k 0.92 / 0.42 / 0.43 / 0.41 / 0.41 ms, 1 M 1.69 / 1.25 / 1.24 / 1.17 / 1.26, 2.5 M 2.42 / 2.42 / 2.56 / 2.37 / 2.39
static unsigned locate_grid(int64_t n) {
    const int64_t big = div_up(n, kLocPPB), spread = std::min<int64_t>(div_up(n, 64), 8192);
    return (unsigned)std::max<int64_t>(std::max(big, spread), 1);
}
int launch_locate(hipStream_t s, const KdNode* tree, const uint32_t* packed, ImplicitGeom ig, int32_t n_cells, int levels,
                  ParticleSoA p, int64_t n, GaussParams gp, const unsigned long long* start, SlabOwn own, LocateLists ll) {
    if (n <= 0) return FY_OK;
    // 8-byte entries need offsets and sizes < 2^25; an explicit tree past that takes the instance with 16-byte entries (an implicit one has no other)
    if (packed && n_cells >= (1 << 25)) return fail(FY_ERR_UNSUPPORTED, "implicit-coordinate tree limited to 2^25 cells");
    const bool wide = !packed && (n_cells >= (1 << 25) || locate_wide_forced());      // (FOAMYADE_LOCATE_WIDE: the 16-byte entries on a small tree, tests)
    const size_t esz = wide ? sizeof(uint4) : sizeof(unsigned long long);
    const size_t lds = (size_t)(levels + 1) * kWave * esz;
    const dim3 grid(locate_grid(n));
    auto explicit_walk = [&](size_t lds_bytes, const int32_t* work, const unsigned int* work_n, int cap, int32_t* ovf_list, unsigned int* ovf_count) {
        if (wide)
            hipLaunchKernelGGL((k_locate<false, false, true>), grid, dim3(kWave), lds_bytes, s, tree, packed, ig, n_cells, p, n, gp.maxdist, nullptr, own, work, work_n, WalkDeposit{}, cap, ovf_list,
                               ovf_count, ll.depth_hwm);
        else
            hipLaunchKernelGGL((k_locate<false, false, false>), grid, dim3(kWave), lds_bytes, s, tree, packed, ig, n_cells, p, n, gp.maxdist, nullptr, own, work, work_n, WalkDeposit{}, cap, ovf_list,
                               ovf_count, ll.depth_hwm);
    };
    if (packed) {
        hipLaunchKernelGGL((k_locate<true, false>), grid, dim3(kWave), lds, s, tree, packed, ig, n_cells, p, n, gp.maxdist, start, own, nullptr, nullptr, WalkDeposit{}, 0, nullptr, nullptr, nullptr);
    } else if (ll.fb_list && ll.fb_count && ll.stack_cap > 0 && ll.stack_cap < levels + 1) {
        // (levels + 1) entries per lane are 12 KB per wave at 4 M cells (23 KB with the 16-byte entries of rounds 4 - 5: 6 waves per CU), and the kernel is latency bound.  The stack
        // never gets that deep (starting from best <= maxdist only the split planes within the search radius of the query are stacked): a stack of the depth the walks have been
        // seen to need (ll.depth_hwm) serves them all, and a walk that needs more than that takes the second launch
        const int cap = ll.stack_cap;
        FY_HIP(hipMemsetAsync(ll.fb_count, 0, sizeof(unsigned int), s));
        explicit_walk((size_t)cap * kWave * esz, nullptr, nullptr, cap, ll.fb_list, ll.fb_count);
        FY_LAUNCH_CHECK();
        explicit_walk(lds, ll.fb_list, ll.fb_count, 0, nullptr, nullptr);
    } else {
        explicit_walk(lds, nullptr, nullptr, 0, nullptr, nullptr);
    }
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_nearest_cell(hipStream_t s, const KdNode* tree, const uint32_t* packed, ImplicitGeom ig, int32_t n_cells, const double* pos, int64_t n, int32_t* out) {
    return launch_n(s, packed ? k_nearest_cell<true> : k_nearest_cell<false>, n, 256, tree, packed, ig, n_cells, pos, n, out);
}

int launch_build_locate_lists(hipStream_t s, const uint32_t* packed, ImplicitGeom ig, int32_t n_cells, double maxdist, unsigned short* lists,
                              int32_t cell0, int32_t n_listed) {
    const double md_cells = maxdist / (ig.dx * ig.dx);
    hipLaunchKernelGGL(k_build_locate_lists, dim3(div_up((int64_t)n_listed * 8, 256)), dim3(256), 0, s, packed, ig, n_cells, md_cells, lists, cell0, n_listed);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_locate_deposit(hipStream_t s, const KdNode* tree, const uint32_t* packed, ImplicitGeom ig, int32_t n_cells, int levels, ParticleSoA p, int64_t n,
                          GaussParams gp, const unsigned long long* start, SlabOwn own, LocateLists ll, CellWindow cw, double* pvol_acc, double* up_acc,
                          unsigned char* touched, TileBuckets tb, SideStream side, const double* rec_gather) {
    if (n <= 0) return FY_OK;
    if (rec_gather && !(packed && ll.lists)) return fail(FY_ERR_INVALID, "launch_locate_deposit: the fused record gather needs the candidate lists");
    if (!(packed && ll.lists)) {
        FY_TRY(launch_locate(s, tree, packed, ig, n_cells, levels, p, n, gp, start, own, packed ? LocateLists{} : ll));      // (explicit tree: ll carries the overflow list)
        return launch_deposit(s, p, n, gp, cw, pvol_acc, up_acc, touched, tb);
    }
    if (n_cells >= (1 << 25)) return fail(FY_ERR_UNSUPPORTED, "implicit-coordinate tree limited to 2^25 cells");
    // the lists place and deposit almost every particle; the walk + k_deposit pair takes what is left (usually nothing: zero count, exit)
    if (!ll.fb_zeroed) FY_HIP(hipMemsetAsync(ll.fb_count, 0, sizeof(unsigned int), s));
    hipLaunchKernelGGL(k_locate_deposit, dim3(div_up(n, kDepThreads)), dim3(kDepThreads), 0, s, ll, ig, p, n, gp, own, cw, pvol_acc, up_acc, touched, tb, rec_gather);
    FY_LAUNCH_CHECK();
    // The leftovers (~5e-5 of the particles: within 8e-6 dx of a cell face) are one latency-bound launch (the walk, which also deposits for them).  With a side stream they run beside whatever the caller enqueues next on `s` (the cell-record pack); the caller waits
    // for side.join before anything reads the deposit.  Their few thousand contributions go out as plain atomics (no tile buckets).
    hipStream_t w = s;
    if (side.stream) {
        FY_HIP(hipEventRecord(side.fork, s));
        FY_HIP(hipStreamWaitEvent(side.stream, side.fork, 0));
        w = side.stream;
    }
    const size_t lds = (size_t)(levels + 1) * kWave * sizeof(unsigned long long);
    const dim3 wgrid((unsigned)std::min<int64_t>(div_up(n, kLocPPB), 2048));
    hipLaunchKernelGGL((k_locate<true, true>), wgrid, dim3(kWave), lds, w, tree, packed, ig, n_cells, p, n, gp.maxdist, start, SlabOwn{}, ll.fb_list, ll.fb_count,
                       WalkDeposit{gp, cw, pvol_acc, up_acc, touched}, 0, nullptr, nullptr, nullptr);
    FY_LAUNCH_CHECK();
    if (side.stream) FY_HIP(hipEventRecord(side.join, side.stream));
    return FY_OK;
}

int launch_deposit(hipStream_t s, ParticleSoA p, int64_t n, GaussParams gp, CellWindow cw, double* pvol_acc, double* up_acc, unsigned char* touched, TileBuckets tb) {
    return launch_n(s, k_deposit, n, kDepThreads, p, n, gp, cw, pvol_acc, up_acc, touched, nullptr, nullptr, tb);
}

}  // namespace fy
