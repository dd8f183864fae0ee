// FV half of the hot path as hand-written HIP for gfx950: the finite-volume operators behind icoFoamYade.C:65-149 and
// pimpleFoamYade.C:60-114 / UcEqn.H / pEqn.H on a uniform hex block.  One lane per cell (or per face), consecutive lanes on
// consecutive x-cells => every array access is a coalesced stream; y/z neighbours are re-reads served by L2.  FP64, no MFMA.
// Operator semantics follow OpenFOAM-6 (see DESIGN.md "FV discretisation"); parity for this half is UNPINNED (no OpenFOAM here).
// This source is compiled TWICE: as it stands (FY_FVK_GRADED 0: the uniform block of cubes, every kernel works with the constants dx, Af, V --
// namespace fy) and through fv_kernels_graded.hip (FY_FVK_GRADED 1: a graded, rectilinear block with per-axis cell sizes -- namespace fy::gr).
// Every geometric quantity goes through the geo_* functions below; in the uniform build they ARE the constants, in the expressions the
// kernels were written and measured with.  The closures that do not depend on the mesh at all -- limiters, turbulence sources, wall functions, bound --
// are fv_closures.hpp's, shared with ldu_kernels.hip.  What reads no geometry -- the pressure solver on the assembled PMat, the multigrid, the fold of the
// block partials -- is not here but in fv_linalg_kernels.hip, compiled once.
#include "fv_kernels.hpp"

#include "common.hpp"
#include "device_util.hpp"
#include "fv_closures.hpp"

#ifndef FY_FVK_GRADED
#define FY_FVK_GRADED 0
#endif

namespace fy {
#if FY_FVK_GRADED
namespace gr {
#endif
namespace {

constexpr double kSmall = 1e-15;     // OpenFOAM `small`

// ------------------------------------------------------------------------------------------------ index helpers
// t = owned-cell number in [0, Nc): lattice coordinates (k local) and storage index c = t + c0
__device__ __forceinline__ void ijk_of(const FvGeo& g, int t, int& i, int& j, int& k) {
    i = t % g.nx;
    const int q = t / g.nx;
    j = q % g.ny;
    k = q / g.ny;
}
__device__ __forceinline__ int cidx(const FvGeo& g, int i, int j, int k) { return i + g.nx * (j + g.ny * (k + g.gz)); }
__device__ __forceinline__ int stride_of(const FvGeo& g, int d) { return d == 0 ? 1 : d == 1 ? g.nx : g.nx * g.ny; }
// doubles between the rows of the stress tensor field G (stored as three vec3 fields over the whole storage, ghost planes included)
__device__ __forceinline__ size_t g_row_stride(const FvGeo& g) { return 3 * (size_t)g.nx * g.ny * (size_t)(g.nz + 2 * g.gz); }
__device__ __forceinline__ int ndim(const FvGeo& g, int d) { return d == 0 ? g.nx : d == 1 ? g.ny : g.nz; }
__device__ __forceinline__ int fid(const FvGeo& g, int d, int i, int j, int k) {
    return d == 0 ? i + (g.nx + 1) * (j + g.ny * k) : d == 1 ? i + g.nx * (j + (g.ny + 1) * k) : i + g.nx * (j + g.ny * k);
}
__device__ __forceinline__ int cface(const FvGeo& g, int d, int s, int i, int j, int k) {
    return fid(g, d, i + (d == 0 ? s : 0), j + (d == 1 ? s : 0), k + (d == 2 ? s : 0));
}
// ------------------------------------------------------------------------------------------------ geometry
// q = index along axis d: of a cell (geo_h, geo_rh, geo_rhalf, geo_lerp_side's qc) or of a face (geo_lerp, geo_rdelta: face q lies between
// cells q - 1 and q).  Linear-interpolation weight of the low-side cell at an internal face = distance from the face to the high-side
// centre over the centre distance [OF-6 surfaceInterpolation::weights]; |Sf| / |d| from the face area and the centre distance, centre to
// face at a boundary [OF-6 deltaCoeffs / fvPatch::deltaCoeffs].  kBfac: the uniform code writes a boundary coefficient as 2 x (gamma dx).
#if FY_FVK_GRADED
[[maybe_unused]] __device__ __forceinline__ double geo_h(const FvGeo& g, int d, int q) { return g.h[d][q]; }
__device__ __forceinline__ double geo_rh(const FvGeo& g, int d, int q) { return 1.0 / g.h[d][q]; }
__device__ __forceinline__ double geo_rhalf(const FvGeo& g, int d, int q) { return 2.0 / g.h[d][q]; }
__device__ __forceinline__ double geo_rdelta(const FvGeo& g, int d, int q) { return 2.0 / (g.h[d][q - 1] + g.h[d][q]); }
__device__ __forceinline__ double geo_V(const FvGeo& g, int i, int j, int k) { return (g.h[0][i] * g.h[1][j]) * g.h[2][k]; }
__device__ __forceinline__ double geo_rV(const FvGeo& g, int i, int j, int k) { return 1.0 / geo_V(g, i, j, k); }
// area of a face normal to d whose transverse indices are those of (i, j, k) (cell or face indices: the normal one is not used)
__device__ __forceinline__ double geo_Af(const FvGeo& g, int d, int i, int j, int k) { return d == 0 ? g.h[1][j] * g.h[2][k] : d == 1 ? g.h[0][i] * g.h[2][k] : g.h[0][i] * g.h[1][j]; }
__device__ __forceinline__ double geo_wlow(const FvGeo& g, int d, int q) { return g.h[d][q] / (g.h[d][q - 1] + g.h[d][q]); }
__device__ __forceinline__ double geo_lerp(const FvGeo& g, int d, int q, double lo, double hi) { const double w = geo_wlow(g, d, q); return w * lo + (1.0 - w) * hi; }
constexpr double kBfac = 1.0;
#else
[[maybe_unused]] __device__ __forceinline__ double geo_h(const FvGeo& g, int, int) { return g.dx; }
__device__ __forceinline__ double geo_rh(const FvGeo& g, int, int) { return g.rdx; }
__device__ __forceinline__ double geo_rhalf(const FvGeo& g, int, int) { return g.rhdx; }
__device__ __forceinline__ double geo_rdelta(const FvGeo& g, int, int) { return g.rdx; }
__device__ __forceinline__ double geo_V(const FvGeo& g, int, int, int) { return g.V; }
__device__ __forceinline__ double geo_rV(const FvGeo& g, int, int, int) { return g.rV; }
__device__ __forceinline__ double geo_Af(const FvGeo& g, int, int, int, int) { return g.Af; }
[[maybe_unused]] __device__ __forceinline__ double geo_wlow(const FvGeo&, int, int) { return 0.5; }
__device__ __forceinline__ double geo_lerp(const FvGeo&, int, int, double lo, double hi) { return 0.5 * (lo + hi); }
constexpr double kBfac = 2.0;
#endif
// value at face (d, s) of the cell with index qc along d, from the cell's own value and its neighbour's across that face
__device__ __forceinline__ double geo_lerp_side(const FvGeo& g, int d, int s, int qc, double own, double nb) {
#if FY_FVK_GRADED
    return s ? geo_lerp(g, d, qc + 1, own, nb) : geo_lerp(g, d, qc, nb, own);
#else
    return 0.5 * (own + nb);
#endif
}
// linear interpolate at face (d, s) of a cell from its own value and the value across the face (q = the FACE's index along d)
__device__ __forceinline__ double lerp_face(const FvGeo& g, int d, int s, int q, double own, double nbv) {
    return s ? geo_lerp(g, d, q, own, nbv) : geo_lerp(g, d, q, nbv, own);
}
// weight of the cell's own value at its face (d, s)
__device__ __forceinline__ double geo_wown(const FvGeo& g, int d, int s, int qc) {
#if FY_FVK_GRADED
    return s ? geo_wlow(g, d, qc + 1) : 1.0 - geo_wlow(g, d, qc);
#else
    return 0.5;
#endif
}
// 1 / (centre distance) across face (d, s) of the cell (i, j, k): centre to face on a physical boundary
__device__ __forceinline__ bool onb(const FvGeo& g, int d, int s, int i, int j, int k);
__device__ __forceinline__ double geo_rdist(const FvGeo& g, int d, int s, int i, int j, int k) {
#if FY_FVK_GRADED
    const int qc = d == 0 ? i : d == 1 ? j : k;
    return onb(g, d, s, i, j, k) ? geo_rhalf(g, d, qc) : geo_rdelta(g, d, qc + s);
#else
    return onb(g, d, s, i, j, k) ? g.rhdx : g.rdx;
#endif
}
// |Sf| / |d| of face (d, s) of cell (i, j, k).  Uniform block: dx for EVERY face -- the boundary's factor 2 is kBfac, where the uniform code has it
__device__ __forceinline__ double geo_sfd(const FvGeo& g, int d, int s, int i, int j, int k) {
#if FY_FVK_GRADED
    return geo_Af(g, d, i, j, k) * geo_rdist(g, d, s, i, j, k);
#else
    return g.dx;
#endif
}
// the same for a FACE given by its own indices (fi, fj, fk) (q = its index along d): boundary faces have q = 0 or q = n
__device__ __forceinline__ double geo_sfd_face(const FvGeo& g, int d, int q, int nq, int fi, int fj, int fk) {
#if FY_FVK_GRADED
    const double rd = q == 0 ? geo_rhalf(g, d, 0) : (q == nq ? geo_rhalf(g, d, nq - 1) : geo_rdelta(g, d, q));
    return geo_Af(g, d, fi, fj, fk) * rd;
#else
    return g.dx;
#endif
}
// cell size along d of the cell with STORAGE index c
__device__ __forceinline__ double geo_hc(const FvGeo& g, int d, int c) {
#if FY_FVK_GRADED
    const int t = c - g.c0;
    return g.h[d][d == 0 ? t % g.nx : d == 1 ? (t / g.nx) % g.ny : t / (g.nx * g.ny)];
#else
    return g.dx;
#endif
}
// LESdelta cubeRootVol [OF-6 cubeRootVolDelta.C]: deltaCoeff * cbrt(V) of the cell (storage index c); the uniform block's is one number
__device__ __forceinline__ double geo_delta(const FvGeo& g, double uniform_delta, int c) {
#if FY_FVK_GRADED
    return g.turb_dcoeff * cbrt((geo_hc(g, 0, c) * geo_hc(g, 1, c)) * geo_hc(g, 2, c));
#else
    return uniform_delta;
#endif
}
// nearWallDist: distance of the cell centre from its face on side d (half the cell's extent along d)
__device__ __forceinline__ double geo_ywall(const FvGeo& g, int d, int c) { return 0.5 * geo_hc(g, d, c); }

// is face (d, s) of owned cell (i,j,k) on a PHYSICAL boundary?  (slab interfaces in z are interior faces)
__device__ __forceinline__ bool onb(const FvGeo& g, int d, int s, int i, int j, int k) {
    if (d == 2) { const int kg = k + g.kglob0; return s ? kg == g.nzglob - 1 : kg == 0; }
    const int q = d == 0 ? i : j;
    return s ? q == ndim(g, d) - 1 : q == 0;
}
// face coordinate q along d (0..ndim): physical low / high boundary?
__device__ __forceinline__ bool face_low_b(const FvGeo& g, int d, int q) { return d == 2 ? (q + g.kglob0 == 0) : (q == 0); }
__device__ __forceinline__ bool face_high_b(const FvGeo& g, int d, int q) { return d == 2 ? (q + g.kglob0 == g.nzglob) : (q == ndim(g, d)); }
// Inlets (FvGeo::inl): the index of the boundary face of owned cell c (storage index) on side `patch` in "U_boundary"'s order -- the six sides x- x+ y- y+ z- z+,
// each side's faces with the lower remaining axis fastest.  Single domain only (an inlet refuses z-slabs): the storage index is the lattice index
__device__ __forceinline__ int boundary_face_of(const FvGeo& g, int patch, int c) {
    const int t = c - g.c0, i = t % g.nx, jk = t / g.nx;
    const int nyz = g.ny * g.nz, nxz = g.nx * g.nz, nxy = g.nx * g.ny, d = patch >> 1, s = patch & 1;
    return d == 0 ? s * nyz + jk : d == 1 ? 2 * nyz + s * nxz + (i + g.nx * (jk / g.ny)) : 2 * (nyz + nxz) + s * nxy + (i + g.nx * (jk % g.ny));
}
// component q of the value a fixedValue side `patch` carries at the boundary face of cell c: the side's one vector, or the face's own where the side is an inlet
// (null pointer, no inlets: exactly the uniform read, as it always was, behind one scalar test of a kernel argument)
__device__ __forceinline__ double u_fixed(const FvGeo& g, int patch, int c, int q) {
    if (g.inl != nullptr) { const InletView v = *g.inl; if ((v.sides >> patch) & 1) return v.u_face[3 * (size_t)boundary_face_of(g, patch, c) + q]; }
    return g.u_val[patch][q];
}
// ... and the whole vector behind one test
__device__ __forceinline__ void u_fixed3(const FvGeo& g, int patch, int c, double* out) {
    out[0] = g.u_val[patch][0]; out[1] = g.u_val[patch][1]; out[2] = g.u_val[patch][2];
    if (g.inl != nullptr) {
        const InletView v = *g.inl;
        if ((v.sides >> patch) & 1) { const double* u = v.u_face + 3 * (size_t)boundary_face_of(g, patch, c); out[0] = u[0]; out[1] = u[1]; out[2] = u[2]; }
    }
}
__device__ __forceinline__ void Ub(const FvGeo& g, const double* F, int c, int patch, double* out) {
    if (g.u_bc[patch] == 0) u_fixed3(g, patch, c, out);
    else { out[0] = F[3 * (size_t)c]; out[1] = F[3 * (size_t)c + 1]; out[2] = F[3 * (size_t)c + 2]; }
    // symmetryPlane / slip on a planar, axis-aligned patch [OF-6 basicSymmetryFvPatchField::evaluate]: the cell value without its normal component
    if (g.u_bc[patch] == 2) out[patch >> 1] = 0.0;
}
__device__ __forceinline__ double pbv(const FvGeo& g, const double* p, const CFace3& psn, int c, int d, int s, int face) {
    const int patch = 2 * d + s;
    if (g.p_bc[patch] == 1) return g.p_val[patch];
    if (g.p_bc[patch] == 2) return p[c] + (s ? 0.5 : -0.5) * geo_hc(g, d, c) * psn.a[d][face];
    return p[c];
}
// boundary value of nut on patch `patch` next to cell c (FvGeo: nut_bc 0 zeroGradient, 1 fixedValue, 2 nutkWallFunction)
__device__ __forceinline__ double nut_boundary(const FvGeo& g, int patch, int c) {
    const int t = g.nut_bc[patch];
    if (t == 1 || ((t == 2 || t == 3) && !g.nut_wall_live)) return g.nut_val[patch];
    if (t == 3) {                                       // calculated: correctNut()'s expression on the boundary values (fv_closures.hpp: nut_keqn, nut_kepsilon)
        const double kb = g.k_bc[patch] == 1 ? g.k_val[patch] : g.kturb[c];
        if (g.turb_model == 2) return nut_keqn(g.turb_ck, kb, geo_delta(g, g.turb_delta, c));
        const double eb = g.eps_bc[patch] == 1 ? g.eps_val[patch] : g.epsturb[c];
        return nut_kepsilon(g.turb_cmu, kb, eb);
    }
    if (t == 2) return nutk_wall_nut(g.wf_cmu25, geo_ywall(g, patch >> 1, c), g.kturb[c], g.nu, g.wf_yPlusLam, g.wf_kappa, g.wf_E);
    return g.nut[c];
}
// Value held by the previous / next lane of the wave (undefined in lane 0 / 63): one DPP move per dword.  A wave's lanes are consecutive
// x-cells, so the x-neighbours of a stencil are already in registers next door -- two more full-wave loads of an AoS vector field
// (24 cache lines each way for the address unit) become two single-lane loads at the wave's ends.
__device__ __forceinline__ double wave_prev(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);      // wave_shr:1
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_next(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x130, 0xf, 0xf, false);      // wave_shl:1
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x130, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// x-neighbours of an AoS vector field from the neighbouring lanes; call in wave-uniform control flow (every lane that holds a cell)
__device__ __forceinline__ void x_neighbours3(const double* __restrict__ F, int c, int i, int nx, const double (&own)[3], double (&L)[3], double (&R)[3]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < 3; ++q) { L[q] = wave_prev(own[q]); R[q] = wave_next(own[q]); }
    if (lane == 0 && i > 0) for (int q = 0; q < 3; ++q) L[q] = F[3 * (size_t)(c - 1) + q];
    if (lane == 63 && i + 1 < nx) for (int q = 0; q < 3; ++q) R[q] = F[3 * (size_t)(c + 1) + q];
}
// Strip order (round 5): on top of the XCD's contiguous z-slab, its blocks run strip by strip -- a strip = strip_B consecutive 256-cell blocks of a
// plane (a few rows), followed by the same strip of the next plane, and so on up the slab, before the next strip starts.  The cell above /
// below the one a block is working on was then touched strip_B blocks ago instead of a whole plane of blocks ago: with a dozen arrays in a sweep a
// plane of them (5 - 6 MB at 160^2) does not survive in the XCD's 4 MB L2 until the next plane comes by, a strip of them (300 KB) does.
// Host side (Solver::create): strips only when planes are whole numbers of blocks and every XCD gets whole planes; FOAMYADE_STRIP_BLOCKS.
// Returns the LOGICAL block (cells [256 b, 256 b + 256)); partial sums are stored under it, so folds do not depend on the order.
__device__ __forceinline__ int fv_block(const FvGeo& g, int bid, int nblk) {
    if (g.win_nblk > 0) return g.win_blk0 + bid;            // a window of whole z-planes (its blocks in storage order)
    if (g.strip_B <= 0) return swz_block(bid, nblk);
    const int x = bid & 7, l = bid >> 3;
    const int per = g.strip_nzx * g.strip_B;
    const int s = l / per, rem = l - s * per;
    const int kk = rem / g.strip_B, b = rem - kk * g.strip_B;
    return (x * g.strip_nzx + kk) * g.strip_bp + s * g.strip_B + b;
}

// FY_RED_LOOP (device_util.hpp) over the owned cells of g, blocks in strip order; fy_lb / fy_stride = the logical block and the whole sweep's
// block count (pass them to block_reduce_store)
#define FY_RED_LOOP_G(g, t) const int fy_lb = fv_block(g, blockIdx.x, gridDim.x); const int fy_stride = (g).win_nblk > 0 ? (g).red_stride : (int)gridDim.x; \
    const int t = fy_lb * 256 + (int)threadIdx.x; if (t < (g).Nc)

// ------------------------------------------------------------------------------------------------ face kernels
// generic face iteration: thread -> (d fixed per launch, face index f) -> local (i,j,k) of the face
__device__ __forceinline__ bool face_ijk(const FvGeo& g, int d, size_t f, int& i, int& j, int& k) {
    const int ex = g.nx + (d == 0), ey = g.ny + (d == 1), ez = g.nz + (d == 2);
    if (f >= (size_t)ex * ey * ez) return false;
    i = (int)(f % ex);
    const size_t t = f / ex;
    j = (int)(t % ey);
    k = (int)(t / ey);
    return true;
}

// fvc::flux(F) = linearInterpolate(F) & Sf with U's boundary conditions (createPhi; flux(HbyA) with constrainHbyA)
__device__ __forceinline__ double face_flux_vec(const FvGeo& g, const double* F, int d, int i, int j, int k) {
    const int q = d == 0 ? i : d == 1 ? j : k;
    double v;
    if (face_low_b(g, d, q)) { double b[3]; Ub(g, F, cidx(g, i, j, k), 2 * d, b); v = b[d]; }
    else if (face_high_b(g, d, q)) { double b[3]; Ub(g, F, cidx(g, i - (d == 0), j - (d == 1), k - (d == 2)), 2 * d + 1, b); v = b[d]; }
    else { const int c = cidx(g, i, j, k); v = geo_lerp(g, d, q, F[3 * (size_t)(c - stride_of(g, d)) + d], F[3 * (size_t)c + d]); }
    return v * geo_Af(g, d, i, j, k);
}

template <int D>
__global__ __launch_bounds__(256) void k_flux_of(FvGeo g, const double* __restrict__ F, double* __restrict__ out) {
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    int i, j, k;
    if (!face_ijk(g, D, f, i, j, k)) return;
    out[f] = face_flux_vec(g, F, D, i, j, k);
}

template <int D>
__device__ __forceinline__ void interp_alpha_face(const FvGeo& g, size_t f, int i, int j, int k, const double* __restrict__ alpha, double* __restrict__ af) {
    const int q = D == 0 ? i : D == 1 ? j : k;
    if (face_low_b(g, D, q) || face_high_b(g, D, q)) af[f] = 1.0;     // calculated patch, value 1 (`alpha = 1.0`, FoamYade.C:68)
    else { const int c = cidx(g, i, j, k); af[f] = geo_lerp(g, D, q, alpha[c - stride_of(g, D)], alpha[c]); }
}

template <int D>
__global__ __launch_bounds__(256) void k_interp_rAU(FvGeo g, const double* __restrict__ rAU, double* __restrict__ rf) {
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    int i, j, k;
    if (!face_ijk(g, D, f, i, j, k)) return;
    const int q = D == 0 ? i : D == 1 ? j : k;
    if (face_low_b(g, D, q)) rf[f] = rAU[cidx(g, i, j, k)];
    else if (face_high_b(g, D, q)) rf[f] = rAU[cidx(g, i - (D == 0), j - (D == 1), k - (D == 2))];
    else { const int c = cidx(g, i, j, k); rf[f] = geo_lerp(g, D, q, rAU[c - stride_of(g, D)], rAU[c]); }
}

// Every face of the block exactly once from a cell-centred sweep: an owned cell does its three low faces, and the high face where it
// is the last cell of its row / column / slab.  One pass over the cell fields instead of one per direction (the three per-direction
// launches each pulled the whole AoS vector fields through for one component: 264 -> 168 B/cell for phiHbyA); same arithmetic per face.
#define FY_CELL_FACES(g, i, j, k, CALL)                     \
    do {                                                    \
        CALL(0, i, j, k); if (i == g.nx - 1) CALL(0, i + 1, j, k); \
        CALL(1, i, j, k); if (j == g.ny - 1) CALL(1, i, j + 1, k); \
        CALL(2, i, j, k); if (k == g.nz - 1) CALL(2, i, j, k + 1); \
    } while (0)

// does cell (i, j, k) store face (D, S)?  its low faces always, a high face where no cell lies beyond it in this domain
__device__ __forceinline__ bool owns_face(const FvGeo& g, int d, int s, int i, int j, int k) {
    return s == 0 || (d == 0 ? i == g.nx - 1 : d == 1 ? j == g.ny - 1 : k == g.nz - 1);
}

// rAUcf = fvc::interpolate(rAUc) and phicForces = fvc::flux(rAUc*uSource) + rAUcf*(g & Sf) in one cell-centred sweep (UcEqn.H:15-20;
// uSource's calculated boundary value is 0)
template <int D>
__device__ __forceinline__ void rAUf_phi_forces_face(const FvGeo& g, size_t f, int i, int j, int k, const double* __restrict__ rAU,
                                                     const double* __restrict__ uSource, double* __restrict__ rf, double* __restrict__ out) {
    const int q = D == 0 ? i : D == 1 ? j : k;
    double r, fl = 0.0;
    if (face_low_b(g, D, q)) r = rAU[cidx(g, i, j, k)];
    else if (face_high_b(g, D, q)) r = rAU[cidx(g, i - (D == 0), j - (D == 1), k - (D == 2))];
    else {
        const int c = cidx(g, i, j, k), cm = c - stride_of(g, D);
        const double rm = rAU[cm], rc = rAU[c];
        r = geo_lerp(g, D, q, rm, rc);
        fl = geo_lerp(g, D, q, rm * uSource[3 * (size_t)cm + D], rc * uSource[3 * (size_t)c + D]) * geo_Af(g, D, i, j, k);
    }
    rf[f] = r;
    out[f] = fl + r * (g.g[D] * geo_Af(g, D, i, j, k));
}
__global__ __launch_bounds__(256) void k_rAUf_phi_forces_cells(FvGeo g, const double* __restrict__ rAU, const double* __restrict__ uSource, Face3 rf, Face3 out) {
    const int t = fv_block(g, blockIdx.x, gridDim.x) * 256 + (int)threadIdx.x;
    if (t >= g.Nc) return;
    int i, j, k; ijk_of(g, t, i, j, k);
#define FY_CALL(D, fi, fj, fk) { const size_t f = (size_t)fid(g, D, fi, fj, fk); rAUf_phi_forces_face<D>(g, f, fi, fj, fk, rAU, uSource, rf.a[D], out.a[D]); }
    FY_CELL_FACES(g, i, j, k, FY_CALL);
#undef FY_CALL
}

__global__ __launch_bounds__(256) void k_interp_alpha_cells(FvGeo g, const double* __restrict__ alpha, Face3 af) {
    const int t = fv_block(g, blockIdx.x, gridDim.x) * 256 + (int)threadIdx.x;
    if (t >= g.Nc) return;
    int i, j, k; ijk_of(g, t, i, j, k);
#define FY_CALL(D, fi, fj, fk) { const size_t f = (size_t)fid(g, D, fi, fj, fk); interp_alpha_face<D>(g, f, fi, fj, fk, alpha, af.a[D]); }
    FY_CELL_FACES(g, i, j, k, FY_CALL);
#undef FY_CALL
}

// phiHbyA = fvc::flux(HbyA) + [alphacf*]rAUf*fvc::ddtCorr(U, phi) [+ phicForces]; constrainPressure on fixedFluxPressure patches
// (icoFoamYade.C:101-111, pEqn.H:4-21).  ddtCorr = EulerDdtScheme::fvcDdtPhiCorr with fvcDdtPhiCoeff.
// KEEP: the ddtCorr term [alphacf] rAUf ddtCorr(U, phi) is made of old-time fields and of rAUf / alphacf, none of which changes between the correctors of one
// momentum assembly: the first corrector (KEEP 1) stores it per face, the later ones (KEEP 2) read it back instead of U.oldTime, phi.oldTime, rAUf and alphacf
// (96 B per cell less; the same value added in the same place, so the same bits).  KEEP 0: neither (no scratch field given)
template <int D, int KEEP>
__device__ __forceinline__ void phiHbyA_face(const FvGeo& g, size_t f, int i, int j, int k, const double* __restrict__ HbyA, const double* __restrict__ U,
                                             const double* __restrict__ Uold, const double* __restrict__ phiOld,
                                             const double* __restrict__ rAUf, const double* __restrict__ alphaf,
                                             const double* __restrict__ phiForces, double* __restrict__ out, double* __restrict__ psn, double* __restrict__ ddtc) {
    const int q = D == 0 ? i : D == 1 ? j : k;
    double v = face_flux_vec(g, HbyA, D, i, j, k);
    int bpatch = -1, bc = -1;
    if (face_low_b(g, D, q)) { bpatch = 2 * D; bc = cidx(g, i, j, k); }
    else if (face_high_b(g, D, q)) { bpatch = 2 * D + 1; bc = cidx(g, i - (D == 0), j - (D == 1), k - (D == 2)); }
    const double Afc = geo_Af(g, D, i, j, k);
    double add;
    if (KEEP == 2) {
        add = ddtc[f];
    } else {
        double uf;
        bool fixes = false;
        if (bpatch >= 0) { fixes = g.u_bc[bpatch] == 0; double b[3]; if (bpatch == 2 * D) Ub(g, Uold, bc, 2 * D, b); else Ub(g, Uold, bc, 2 * D + 1, b); uf = b[D] * Afc; }      // (the side as a constant: FvGeo's tables are indexed by it)
        else { const int c = cidx(g, i, j, k); uf = geo_lerp(g, D, q, Uold[3 * (size_t)(c - stride_of(g, D)) + D], Uold[3 * (size_t)c + D]) * Afc; }
        const double po = phiOld[f];
        const double phiCorr = po - uf;
        const double coef = fixes ? 0.0 : 1.0 - fmin(fabs(phiCorr) / (fabs(po) + kSmall), 1.0);
        add = rAUf[f] * (coef * (1.0 / g.dt) * phiCorr);
        if (g.pimple) add *= alphaf[f];
        if (KEEP == 1) ddtc[f] = add;
    }
    v += add;
    if (g.pimple) v += phiForces[f];
    out[f] = v;
    if (bpatch >= 0 && g.p_bc[bpatch] == 2) {
        double ub[3];
        if (bpatch == 2 * D) Ub(g, U, bc, 2 * D, ub); else Ub(g, U, bc, 2 * D + 1, ub);
        psn[f] = (v - ub[D] * Afc) / (rAUf[f] * Afc);
    }
}

template <int KEEP>
__global__ __launch_bounds__(256) void k_phiHbyA_cells(FvGeo g, const double* __restrict__ HbyA, const double* __restrict__ U,
                                                       const double* __restrict__ Uold, CFace3 phiOld, CFace3 rAUf, CFace3 alphaf,
                                                       CFace3 phiForces, Face3 out, Face3 psn, Face3 ddtc) {
    const int t = fv_block(g, blockIdx.x, gridDim.x) * 256 + (int)threadIdx.x;
    if (t >= g.Nc) return;
    int i, j, k; ijk_of(g, t, i, j, k);
#define FY_CALL(D, fi, fj, fk) { const size_t f = (size_t)fid(g, D, fi, fj, fk); \
        phiHbyA_face<D, KEEP>(g, f, fi, fj, fk, HbyA, U, Uold, phiOld.a[D], rAUf.a[D], alphaf.a[D], phiForces.a[D], out.a[D], psn.a[D], ddtc.a[D]); }
    FY_CELL_FACES(g, i, j, k, FY_CALL);
#undef FY_CALL
}

// ---- adjustPhi(phiHbyA, U, p) (icoFoamYade.C:108, pEqn.H:13-16) [OF-6 cfdTools/general/adjustPhi/adjustPhi.C].  Acts when no patch
// fixes the pressure: the outflow through the patches that do not fix U is scaled by massCorr = (massIn - fixedMassOut) / adjustableMassOut
// so that the pressure equation is solvable.  In pimpleFoamYade it is applied BEFORE phicForces are added (pEqn.H:13-18); phiHbyA here
// already carries them, so the flux it works on is phiHbyA - phicForces.  slots: 0 massIn, 1 fixedMassOut, 2 adjustableMassOut,
// 3 sum |flux| over the internal faces (the normalisation of the two tests)
template <int D>
__device__ __forceinline__ void adjust_phi_face(const FvGeo& g, size_t f, int i, int j, int k, const double* __restrict__ phiHbyA,
                                                const double* __restrict__ phiForces, double* v) {
    const int q = D == 0 ? i : D == 1 ? j : k;
    const double fl = phiHbyA[f] - (g.pimple ? phiForces[f] : 0.0);
    const bool lo = face_low_b(g, D, q), hi = face_high_b(g, D, q);
    if (lo || hi) {
        const double outw = lo ? -fl : fl;
        const bool fixes = g.u_bc[2 * D + (hi ? 1 : 0)] == 0;
        if (outw < 0.0) v[0] -= outw;
        else if (fixes) v[1] += outw;
        else v[2] += outw;
    } else if (!(D == 2 && k == g.nz)) {                    // a slab's top interface face belongs to the slab above (counted there)
        v[3] += fabs(fl);
    }
}
__global__ __launch_bounds__(256) void k_adjust_phi_sums(FvGeo g, CFace3 phiHbyA, CFace3 phiForces, double* __restrict__ partials) {
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    FY_RED_LOOP_G(g, t) {
        int i, j, k; ijk_of(g, t, i, j, k);
#define FY_CALL(D, fi, fj, fk) { const size_t f = (size_t)fid(g, D, fi, fj, fk); adjust_phi_face<D>(g, f, fi, fj, fk, phiHbyA.a[D], phiForces.a[D], v); }
        FY_CELL_FACES(g, i, j, k, FY_CALL);
#undef FY_CALL
    }
    const int mx[4] = {0, 0, 0, 0};
    block_reduce_store<4>(v, mx, partials, fy_lb, fy_stride);
}
// one thread per boundary face of the block (both sides of the three directions); err: set when OpenFOAM would stop with
// "Continuity error cannot be removed by adjusting the outflow"
__global__ __launch_bounds__(256) void k_adjust_phi_apply(FvGeo g, const double* __restrict__ sums, Face3 phiHbyA, CFace3 phiForces, CFace3 rAUf,
                                                          const double* __restrict__ U, Face3 psn, int* __restrict__ err) {
    const double massIn = sums[0], fixedOut = sums[1], adjOut = sums[2], total = 1e-300 + sums[3];
    double massCorr = 1.0;
    if (fabs(adjOut) > 1e-300 && fabs(adjOut) / total > kSmall) massCorr = (massIn - fixedOut) / adjOut;
    else if (fabs(fixedOut - massIn) / total > 1e-8) { if (blockIdx.x == 0 && threadIdx.x == 0) *err = 1; return; }
    if (massCorr == 1.0) return;
    const int nb[3] = {g.ny * g.nz, g.nx * g.nz, g.nx * g.ny};
    int t = blockIdx.x * 256 + threadIdx.x;
    int d = 0, s = 0;
    for (; d < 3; ++d) { if (t < 2 * nb[d]) { s = t >= nb[d]; t -= s * nb[d]; break; } t -= 2 * nb[d]; }
    if (d == 3) return;
    int i, j, k;
    if (d == 0) { j = t % g.ny; k = t / g.ny; i = s ? g.nx : 0; }
    else if (d == 1) { i = t % g.nx; k = t / g.nx; j = s ? g.ny : 0; }
    else { i = t % g.nx; j = t / g.nx; k = s ? g.nz : 0; }
    const int q = d == 0 ? i : d == 1 ? j : k;
    if (!(s ? face_high_b(g, d, q) : face_low_b(g, d, q))) return;        // (a slab's interface plane is not a patch)
    const int patch = 2 * d + s;
    if (g.u_bc[patch] == 0) return;                                        // fixes the value: not adjustable
    const size_t f = (size_t)fid(g, d, i, j, k);
    const double pf = g.pimple ? phiForces.a[d][f] : 0.0;
    const double fl = phiHbyA.a[d][f] - pf;
    const double outw = s ? fl : -fl;
    if (!(outw > 0.0)) return;
    const double v = fl * massCorr + pf;
    phiHbyA.a[d][f] = v;
    if (g.p_bc[patch] == 2) {                                              // constrainPressure sees the adjusted flux (pEqn.H:21)
        const int c = cidx(g, i - (d == 0 && s), j - (d == 1 && s), k - (d == 2 && s));
        double ub[3]; Ub(g, U, c, patch, ub);
        const double Afc = geo_Af(g, d, i, j, k);
        psn.a[d][f] = (v - ub[d] * Afc) / (rAUf.a[d][f] * Afc);
    }
}

// pEqn.flux() and phi = phiHbyA - pEqn.flux()[/alphacf]   (icoFoamYade.C:129, pEqn.H:39), all three directions in one cell-centred sweep
// (three per-direction launches: 3 x 36 us at 160^3; the pressure field went through three times).
// pimple: what is kept per face is not pEqn.flux() itself but the face term of the velocity reconstruction that follows (pEqn.H:43-45),
// (phicForces - pEqn.flux() / alphacf) / rAUcf -- its only reader, k_U_correct, then streams ONE face field instead of four (the same
// operations on the same operands in the same order, so the same bits; 48 B per cell and corrector less traffic)
template <int D>
__device__ __forceinline__ void flux_correct_face(const FvGeo& g, size_t f, int i, int j, int k, const double* __restrict__ p, const double* __restrict__ phiHbyA,
                                                  const double* __restrict__ rAUf, const double* __restrict__ alphaf, const double* __restrict__ psn,
                                                  const double* __restrict__ phiForces, double* __restrict__ pflux, double* __restrict__ phi) {
    const int q = D == 0 ? i : D == 1 ? j : k;
    const double af = g.pimple ? alphaf[f] : 1.0;
    double fl = 0.0;
    const bool lo = face_low_b(g, D, q), hi = face_high_b(g, D, q);
    if (lo || hi) {
        const int s = lo ? 0 : 1, patch = 2 * D + s;
        const int c = cidx(g, i - (D == 0 && s), j - (D == 1 && s), k - (D == 2 && s));
        if (g.p_bc[patch] == 1) { const double gb = kBfac * af * rAUf[f] * geo_sfd_face(g, D, q, ndim(g, D), i, j, k); fl = s ? gb * (g.p_val[patch] - p[c]) : gb * (p[c] - g.p_val[patch]); }
        else if (g.p_bc[patch] == 2) fl = af * rAUf[f] * geo_Af(g, D, i, j, k) * psn[f];
    } else {
        const int c = cidx(g, i, j, k);
        fl = af * rAUf[f] * geo_sfd_face(g, D, q, ndim(g, D), i, j, k) * (p[c] - p[c - stride_of(g, D)]);
    }
    const double fa = fl / af;
    pflux[f] = g.pimple ? (phiForces[f] - fa) / rAUf[f] : fl;
    phi[f] = phiHbyA[f] - fa;
}
__global__ __launch_bounds__(256) void k_flux_correct_cells(FvGeo g, const double* __restrict__ p, CFace3 phiHbyA, CFace3 rAUf, CFace3 alphaf, CFace3 psn,
                                                            CFace3 phiForces, Face3 pflux, Face3 phi) {
    const int t = fv_block(g, blockIdx.x, gridDim.x) * 256 + (int)threadIdx.x;
    if (t >= g.Nc) return;
    int i, j, k; ijk_of(g, t, i, j, k);
#define FY_CALL(D, fi, fj, fk) { const size_t f = (size_t)fid(g, D, fi, fj, fk); \
        flux_correct_face<D>(g, f, fi, fj, fk, p, phiHbyA.a[D], rAUf.a[D], alphaf.a[D], psn.a[D], phiForces.a[D], pflux.a[D], phi.a[D]); }
    FY_CELL_FACES(g, i, j, k, FY_CALL);
#undef FY_CALL
}

// ------------------------------------------------------------------------------------------------ cell kernels
// CourantNo.H:32-49: sumPhi = fvc::surfaceSum(mag(phi)); slots: 0 = max(sumPhi/V), 1 = sum(sumPhi)
__global__ __launch_bounds__(256) void k_courant(FvGeo g, CFace3 phi, double* __restrict__ partials) {
    double v[2] = {0.0, 0.0};
    FY_RED_LOOP_G(g, t) {
        int i, j, k; ijk_of(g, t, i, j, k);
        double s = 0.0;
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int sd = 0; sd < 2; ++sd) s += fabs(phi.a[d][cface(g, d, sd, i, j, k)]);
        v[0] = fmax(v[0], s * geo_rV(g, i, j, k));
        v[1] += s;
    }
    const int mx[2] = {1, 0};
    block_reduce_store<2>(v, mx, partials, fy_lb, fy_stride);
}

// ---- the explicit stress term G = alpha nuEff dev2(T(grad U)) and its divergence, piece by piece: stated once for the two sweeps that hand G through memory
// (k_pre_coupling, k_div_G) and for the sweep that keeps it in LDS (k_stress_div), so that both paths form every value by the same operations in the same order
// U at face (d, s) of a cell (qc = its index along d) from the cell's value uc and its neighbour's un: on a physical boundary Ub() on the cell's own value
__device__ __forceinline__ void u_face_value(const FvGeo& g, int d, int s, bool on_boundary, int qc, int c, const double (&uc)[3], const double* un, double (&fv)[3]) {
    if (on_boundary) {
        const int patch = 2 * d + s;
        if (g.u_bc[patch] == 0) u_fixed3(g, patch, c, fv);
        else { fv[0] = uc[0]; fv[1] = uc[1]; fv[2] = uc[2]; }
        if (g.u_bc[patch] == 2) fv[d] = 0.0;
    } else {
        for (int q = 0; q < 3; ++q) fv[q] = geo_lerp_side(g, d, s, qc, uc[q], un[q]);
    }
}
// row d of T = fvc::grad(U), Gauss linear, from the two face values along d
__device__ __forceinline__ void grad_row(const FvGeo& g, int d, int qc, const double (&fv)[2][3], double (&T)[9]) {
    const double rhd = geo_rh(g, d, qc);
    for (int q = 0; q < 3; ++q) T[3 * d + q] = (fv[1][q] - fv[0][q]) * rhd;
}
__device__ __forceinline__ double stress_trace(const double (&T)[9]) { return T[0] + T[4] + T[8]; }
// alpha nuEff (nuEff = nut + nu [OF-6 eddyViscosity/linearViscousStress])
__device__ __forceinline__ double stress_coeff(const FvGeo& g, const double* __restrict__ alpha, int c) { return g.nut ? alpha[c] * (g.nu + g.nut[c]) : alpha[c] * g.nu; }
__device__ __forceinline__ double stress_entry(double an, const double (&T)[9], double tr, int a, int b) { return an * (T[3 * b + a] - (a == b ? (2.0 / 3.0) * tr : 0.0)); }
// div G at a cell from row d of G at the cell (own[d]) and at its +-d neighbours (nbv[d][s]); a boundary face takes the cell's own row
__device__ __forceinline__ void div_of_rows(const FvGeo& g, const bool (&bnd)[3][2], const int (&ijk)[3], const double (&own)[3][3], const double (&nbv)[3][2][3], double (&acc)[3]) {
    acc[0] = acc[1] = acc[2] = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        double fv[2][3];
#pragma unroll
        for (int s = 0; s < 2; ++s)
            for (int q = 0; q < 3; ++q) fv[s][q] = bnd[d][s] ? own[d][q] : geo_lerp_side(g, d, s, ijk[d], own[d][q], nbv[d][s][q]);
        for (int q = 0; q < 3; ++q) acc[q] += (fv[1][q] - fv[0][q]) * geo_rh(g, d, ijk[d]);
    }
}

// vGrad = fvc::grad(U) (icoFoamYade.C:71, pimpleFoamYade.C:76); pimple also gradP = fvc::grad(p) (:74) and
// divT = 2 nu fvc::laplacian(alphac, Uc) (:75)
// In pimple mode the only consumer of grad(U) is the explicit stress term of divDevRhoReff (the Gaussian torque that would read vGrad
// is disabled in the reference, FoamYade.C:618), so the kernel can emit G = alpha nu dev2(T(grad U)) directly (Gout != nullptr) and
// skip the 72 B/cell vGrad store (write_vgrad = 0): one stencil pass instead of two plus a tensor round trip through HBM.
__global__ __launch_bounds__(256) void k_pre_coupling(FvGeo g, const double* __restrict__ U, const double* __restrict__ p,
                                                      const double* __restrict__ alpha, CFace3 psn, double* __restrict__ vGrad,
                                                      double* __restrict__ gradP, double* __restrict__ divT, double* __restrict__ Gout,
                                                      int write_vgrad, int write_pfields, CFace3 phi, double* __restrict__ ddtU, double* __restrict__ Uold_out,
                                                      double* __restrict__ cellrec, double rec_two_nu, double rec_rhoF, Face3 dcorr) {
    const int t = fv_block(g, blockIdx.x, gridDim.x) * 256 + (int)threadIdx.x;
    if (t >= g.Nc) return;
    int i, j, k; ijk_of(g, t, i, j, k);
    const int c = t + g.c0;
    const bool pf = g.pimple && write_pfields;          // gradP and divT wanted
    // ---- gather first (round 5): every neighbour value is loaded up front from an address that is always valid (across a boundary face the
    // "neighbour" is the cell itself), the faces are evaluated from registers afterwards.  With the loads inside the per-face branches a wave made
    // one dependent memory round trip per face: 240 us for this sweep's 200 B/cell
    const int ijk[3] = {i, j, k};
    bool bnd[3][2];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int s = 0; s < 2; ++s) bnd[d][s] = onb(g, d, s, i, j, k);
    const double uc[3] = {U[3 * (size_t)c], U[3 * (size_t)c + 1], U[3 * (size_t)c + 2]};
    const double pc = pf ? p[c] : 0.0, ac = pf ? alpha[c] : 0.0;
    double un6[3][2][3], pn6[3][2], an6[3][2];
#pragma unroll
    for (int d = 1; d < 3; ++d)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int nb = bnd[d][s] ? c : c + (s ? stride_of(g, d) : -stride_of(g, d));
            un6[d][s][0] = U[3 * (size_t)nb]; un6[d][s][1] = U[3 * (size_t)nb + 1]; un6[d][s][2] = U[3 * (size_t)nb + 2];
            pn6[d][s] = pf ? p[nb] : 0.0; an6[d][s] = pf ? alpha[nb] : 0.0;
        }
    const bool want_phi = ddtU != nullptr || dcorr.a[0] != nullptr;
    double phf[3][2];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int s = 0; s < 2; ++s) phf[d][s] = want_phi ? phi.a[d][cface(g, d, s, i, j, k)] : 0.0;
    // x-neighbours from the neighbouring lanes (wave_prev / wave_next); the wave's end lanes fetch theirs
    const int lane = threadIdx.x & 63;
    {
        const int xm = (lane == 0 && i > 0) ? c - 1 : c, xp = (lane == 63 && i + 1 < g.nx) ? c + 1 : c;      // (only the end lanes use what they load)
        double em[3] = {0, 0, 0}, ep[3] = {0, 0, 0}, epm = 0, epp = 0, eam = 0, eap = 0;
        if (lane == 0 || lane == 63) {
            for (int q = 0; q < 3; ++q) { em[q] = U[3 * (size_t)xm + q]; ep[q] = U[3 * (size_t)xp + q]; }
            if (pf) { epm = p[xm]; epp = p[xp]; eam = alpha[xm]; eap = alpha[xp]; }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) { un6[0][0][q] = wave_prev(uc[q]); un6[0][1][q] = wave_next(uc[q]); }
        pn6[0][0] = wave_prev(pc); pn6[0][1] = wave_next(pc); an6[0][0] = wave_prev(ac); an6[0][1] = wave_next(ac);
        if (lane == 0 && i > 0) { for (int q = 0; q < 3; ++q) un6[0][0][q] = em[q]; pn6[0][0] = epm; an6[0][0] = eam; }
        if (lane == 63 && i + 1 < g.nx) { for (int q = 0; q < 3; ++q) un6[0][1][q] = ep[q]; pn6[0][1] = epp; an6[0][1] = eap; }
    }
    if (Uold_out) { Uold_out[3 * (size_t)c] = uc[0]; Uold_out[3 * (size_t)c + 1] = uc[1]; Uold_out[3 * (size_t)c + 2] = uc[2]; }    // runTime++: U.oldTime() (single domain: no ghost planes to copy)
    double lap[3] = {0, 0, 0}, T[9], conv[3] = {0, 0, 0}, gp3[3] = {0, 0, 0};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        double fv[2][3], fp[2] = {0, 0};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            u_face_value(g, d, s, bnd[d][s], ijk[d], c, uc, un6[d][s], fv[s]);
            if (bnd[d][s]) {
                if (pf) {
                    fp[s] = pbv(g, p, psn, c, d, s, cface(g, d, s, i, j, k));
                    for (int q = 0; q < 3; ++q) lap[q] += 1.0 * geo_Af(g, d, i, j, k) * (fv[s][q] - uc[q]) * geo_rhalf(g, d, ijk[d]);     // alphaf = 1 on the boundary
                }
            } else {
                const double* un = un6[d][s];
                const int qc = ijk[d];
                if (pf) {
                    fp[s] = geo_lerp_side(g, d, s, qc, pc, pn6[d][s]);
                    const double af = geo_lerp_side(g, d, s, qc, ac, an6[d][s]);
                    for (int q = 0; q < 3; ++q) lap[q] += af * geo_Af(g, d, i, j, k) * (un[q] - uc[q]) * geo_rdelta(g, d, qc + s);
                }
            }
        }
        if (dcorr.a[0]) {
            // the old-time part of ddtCorr(U, phi) (EulerDdtScheme::fvcDdtPhiCorr with fvcDdtPhiCoeff; phiHbyA_face): coef / deltaT (phi.old - flux(U.old)) per
            // face, by the face's owner.  This sweep runs at the start of the step, where U is U.oldTime() and `phi` is phi.oldTime(), and already holds
            // U's face values; the correctors then need neither U.oldTime() nor phi.oldTime() (fused sweep k_corr_front)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (owns_face(g, d, s, i, j, k)) {
                    const int fi = i + (d == 0 ? s : 0), fj = j + (d == 1 ? s : 0), fk = k + (d == 2 ? s : 0);
                    const int f = cface(g, d, s, i, j, k);
                    const double uf = fv[s][d] * geo_Af(g, d, fi, fj, fk);
                    const double po = phf[d][s];
                    const double phiCorr = po - uf;
                    const bool fixes = bnd[d][s] && g.u_bc[2 * d + s] == 0;
                    const double coef = fixes ? 0.0 : 1.0 - fmin(fabs(phiCorr) / (fabs(po) + kSmall), 1.0);
                    dcorr.a[d][f] = coef * (1.0 / g.dt) * phiCorr;
                }
        }
        grad_row(g, d, ijk[d], fv, T);
        if (pf) gp3[d] = (fp[1] - fp[0]) * geo_rh(g, d, ijk[d]);
        if (ddtU) {     // fvc::div(phic, Uc), Gauss linear: the face values are the ones the gradient just used
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const double flux = (s ? 1.0 : -1.0) * phf[d][s];
                for (int q = 0; q < 3; ++q) conv[q] += flux * fv[s][q];
            }
        }
    }
    // pimpleFoamYade.C:73 ddtU_f = fvc::ddt(Uc) + fvc::div(phic, Uc); the ddt term is identically zero there (Uc.oldTime() is
    // stored on that access, before Uc is written in the new step), only consumer: addedMassForce (fy_set_force_models)
    if (ddtU)
        for (int q = 0; q < 3; ++q) ddtU[3 * (size_t)c + q] = conv[q] * geo_rV(g, i, j, k);
    if (write_vgrad)
        for (int q = 0; q < 9; ++q) vGrad[9 * (size_t)c + q] = T[q];
    if (pf)
        for (int q = 0; q < 3; ++q) gradP[3 * (size_t)c + q] = gp3[q];
    if (pf) {
        double dT[3];
        for (int q = 0; q < 3; ++q) { dT[q] = 2 * g.nu * (lap[q] * geo_rV(g, i, j, k)); divT[3 * (size_t)c + q] = dT[q]; }
        if (cellrec) {
            // the 64-byte record the force pass gathers per stencil cell, {U, alpha, 2 nu rho_f divT - gradP, V}, written from here instead of by
            // a pass of its own over U / gradP / divT (k_pack_cells: same operands, same operations, same bits; single domain only)
            double2* r = reinterpret_cast<double2*>(cellrec + 8 * (size_t)c);
            r[0] = make_double2(uc[0], uc[1]);
            r[1] = make_double2(uc[2], ac);
            r[2] = make_double2(((rec_two_nu * dT[0]) * rec_rhoF) - gp3[0], ((rec_two_nu * dT[1]) * rec_rhoF) - gp3[1]);
            r[3] = make_double2(((rec_two_nu * dT[2]) * rec_rhoF) - gp3[2], geo_V(g, i, j, k));
        }
    }
    if (Gout) {
        const double tr = stress_trace(T);
        const double an = stress_coeff(g, alpha, c);
        // stored BY ROWS (three vec3 arrays): k_div_G takes row d from the +-d neighbours only, so it streams 24-byte records
        // instead of picking 24 bytes out of 72-byte ones (fewer lines per load instruction, and the z-planes it re-reads fit L2)
        const size_t rs = g_row_stride(g);
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) Gout[(size_t)a * rs + 3 * (size_t)c + b] = stress_entry(an, T, tr, a, b);
    }
}

// divergence of the explicit part of divDevRhoReff (laminar Stokes), G = alpha nu dev2(T(grad U)) formed by k_pre_coupling, stored by rows
__global__ __launch_bounds__(256) void k_div_G(FvGeo g, const double* __restrict__ G, double* __restrict__ divG) {
    const int t = fv_block(g, blockIdx.x, gridDim.x) * 256 + (int)threadIdx.x;
    if (t >= g.Nc) return;
    int i, j, k; ijk_of(g, t, i, j, k);
    const int c = t + g.c0;
    const int ijk[3] = {i, j, k};
    // gather first (round 5): row d of the tensor at the cell and at its +-d neighbours (across a boundary face the cell itself), then the arithmetic
    const double g0[3] = {G[3 * (size_t)c], G[3 * (size_t)c + 1], G[3 * (size_t)c + 2]};      // row x at this cell; its x-neighbours come from the lanes next door
    double gx[2][3];
    x_neighbours3(G, c, i, g.nx, g0, gx[0], gx[1]);
    bool bnd[3][2];
    double own[3][3], nbv[3][2][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) { own[0][q] = g0[q]; nbv[0][0][q] = gx[0][q]; nbv[0][1][q] = gx[1][q]; }
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int s = 0; s < 2; ++s) bnd[d][s] = onb(g, d, s, i, j, k);
#pragma unroll
    for (int d = 1; d < 3; ++d) {
        const double* Gd = G + (size_t)d * g_row_stride(g);           // row d of the tensor field
#pragma unroll
        for (int q = 0; q < 3; ++q) own[d][q] = Gd[3 * (size_t)c + q];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int nb = bnd[d][s] ? c : c + (s ? stride_of(g, d) : -stride_of(g, d));
#pragma unroll
            for (int q = 0; q < 3; ++q) nbv[d][s][q] = Gd[3 * (size_t)nb + q];
        }
    }
    double acc[3];
    div_of_rows(g, bnd, ijk, own, nbv, acc);
    for (int q = 0; q < 3; ++q) divG[3 * (size_t)c + q] = acc[q];
}

// The two sweeps above in one, without the tensor's trip through memory (single domain, no linearUpwind: nobody else wants grad U or G).  k_div_G takes row d of G
// from the +-d neighbours only, so a tile of cells needs G at its own cells and ONE row at the cells of its six face slabs -- no edge or corner cells.  A workgroup
// forms G for its tile (one cell per thread, rows kept in registers and published to LDS), deals the face slabs' cells out over the same threads in a second round
// (row d of a slab cell needs grad of U_d and the trace: the loads of the other entries fall away), and takes the divergence from LDS after one barrier.
// LDS holds row d over the tile widened by one cell at both ends along d, one plane per component: 8-byte reads at consecutive addresses.  A cell's neighbour across
// a boundary face is the cell itself, as everywhere in this file, so no slab cell lies outside the block; partial tiles at the block's high ends leave lanes idle.
// Every value is formed by the functions k_pre_coupling and k_div_G form it with: the same bits.
#ifndef FY_STRESS_TILE_X
#define FY_STRESS_TILE_X 16
#endif
#ifndef FY_STRESS_TILE_Y
#define FY_STRESS_TILE_Y 8
#endif
#ifndef FY_STRESS_TILE_Z
#define FY_STRESS_TILE_Z 4
#endif
constexpr int kSTX = FY_STRESS_TILE_X, kSTY = FY_STRESS_TILE_Y, kSTZ = FY_STRESS_TILE_Z;
constexpr int kStressThreads = kSTX * kSTY * kSTZ;
constexpr int kSlabX = 2 * kSTY * kSTZ, kSlabY = 2 * kSTX * kSTZ, kSlabZ = 2 * kSTX * kSTY;
static_assert(kStressThreads % 64 == 0 && kStressThreads <= 1024, "a tile is a whole number of waves and one workgroup");
static_assert(((kSTX + 2) * kSTY * kSTZ + kSTX * (kSTY + 2) * kSTZ + kSTX * kSTY * (kSTZ + 2)) * 3 * sizeof(double) <= 64 * 1024, "the tile's rows fit static LDS");

// rows of G at cell (i, j, k) (ROWS: bit a = row a wanted; what the others alone need is never loaded).  Gather first, as k_pre_coupling does
template <unsigned ROWS>
__device__ __forceinline__ void stress_rows_at(const FvGeo& g, const double* __restrict__ U, const double* __restrict__ alpha, int i, int j, int k, double (&G)[3][3]) {
    const int c = cidx(g, i, j, k);
    const int ijk[3] = {i, j, k};
    const double uc[3] = {U[3 * (size_t)c], U[3 * (size_t)c + 1], U[3 * (size_t)c + 2]};
    bool bnd[3][2];
    double un6[3][2][3];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bnd[d][s] = onb(g, d, s, i, j, k);
            const int nb = bnd[d][s] ? c : c + (s ? stride_of(g, d) : -stride_of(g, d));
            un6[d][s][0] = U[3 * (size_t)nb]; un6[d][s][1] = U[3 * (size_t)nb + 1]; un6[d][s][2] = U[3 * (size_t)nb + 2];
        }
    double T[9];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        double fv[2][3];
#pragma unroll
        for (int s = 0; s < 2; ++s) u_face_value(g, d, s, bnd[d][s], ijk[d], c, uc, un6[d][s], fv[s]);
        grad_row(g, d, ijk[d], fv, T);
    }
    const double tr = stress_trace(T);
    const double an = stress_coeff(g, alpha, c);
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if ((ROWS >> a) & 1)
            for (int b = 0; b < 3; ++b) G[a][b] = stress_entry(an, T, tr, a, b);
}

__global__ __launch_bounds__(kStressThreads) void k_stress_div(FvGeo g, const double* __restrict__ U, const double* __restrict__ alpha, double* __restrict__ divG, int ntx, int nty) {
    __shared__ double sx[3][(kSTX + 2) * kSTY * kSTZ], sy[3][kSTX * (kSTY + 2) * kSTZ], sz[3][kSTX * kSTY * (kSTZ + 2)];
    // tiles in x-fastest order, an XCD's share of them contiguous: a range of z (swz_block)
    const int tile = swz_block(blockIdx.x, gridDim.x);
    const int tq = tile / ntx;
    const int i0 = (tile - tq * ntx) * kSTX, j0 = (tq % nty) * kSTY, k0 = (tq / nty) * kSTZ;
    const int tid = threadIdx.x;
    const int lx = tid % kSTX, ly = (tid / kSTX) % kSTY, lz = tid / (kSTX * kSTY);
    const int i = i0 + lx, j = j0 + ly, k = k0 + lz;
    const bool in = i < g.nx && j < g.ny && k < g.nz;
    // a cell's slot in the three images, and the step to its +-d neighbour's
    const int ex = (lx + 1) + (kSTX + 2) * (ly + kSTY * lz), ey = lx + kSTX * ((ly + 1) + (kSTY + 2) * lz), ez = lx + kSTX * (ly + kSTY * (lz + 1));
    double own[3][3];
    if (in) {
        stress_rows_at<7u>(g, U, alpha, i, j, k, own);
#pragma unroll
        for (int q = 0; q < 3; ++q) { sx[q][ex] = own[0][q]; sy[q][ey] = own[1][q]; sz[q][ez] = own[2][q]; }
    }
    // second round: the cells of the six face slabs, one row each (x slabs first, then y, then z; with the 16 x 8 x 4 tile every wave works on one direction)
    for (int h = tid; h < kSlabX + kSlabY + kSlabZ; h += kStressThreads) {
        double G[3][3];
        if (h < kSlabX) {
            const int s = h / (kSTY * kSTZ), r = h - s * (kSTY * kSTZ), hy = r % kSTY, hz = r / kSTY;
            const int hi = s ? i0 + kSTX : i0 - 1, hj = j0 + hy, hk = k0 + hz;
            if (hi >= 0 && hi < g.nx && hj < g.ny && hk < g.nz) {
                stress_rows_at<1u>(g, U, alpha, hi, hj, hk, G);
#pragma unroll
                for (int q = 0; q < 3; ++q) sx[q][(s ? kSTX + 1 : 0) + (kSTX + 2) * (hy + kSTY * hz)] = G[0][q];
            }
        } else if (h < kSlabX + kSlabY) {
            const int hh = h - kSlabX;
            const int s = hh / (kSTX * kSTZ), r = hh - s * (kSTX * kSTZ), hx = r % kSTX, hz = r / kSTX;
            const int hi = i0 + hx, hj = s ? j0 + kSTY : j0 - 1, hk = k0 + hz;
            if (hj >= 0 && hj < g.ny && hi < g.nx && hk < g.nz) {
                stress_rows_at<2u>(g, U, alpha, hi, hj, hk, G);
#pragma unroll
                for (int q = 0; q < 3; ++q) sy[q][hx + kSTX * ((s ? kSTY + 1 : 0) + (kSTY + 2) * hz)] = G[1][q];
            }
        } else {
            const int hh = h - kSlabX - kSlabY;
            const int s = hh / (kSTX * kSTY), r = hh - s * (kSTX * kSTY), hx = r % kSTX, hy = r / kSTX;
            const int hi = i0 + hx, hj = j0 + hy, hk = s ? k0 + kSTZ : k0 - 1;
            if (hk >= 0 && hk < g.nz && hi < g.nx && hj < g.ny) {
                stress_rows_at<4u>(g, U, alpha, hi, hj, hk, G);
#pragma unroll
                for (int q = 0; q < 3; ++q) sz[q][hx + kSTX * (hy + kSTY * (s ? kSTZ + 1 : 0))] = G[2][q];
            }
        }
    }
    __syncthreads();
    if (!in) return;
    const int ijk[3] = {i, j, k};
    bool bnd[3][2];
    double nbv[3][2][3];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int s = 0; s < 2; ++s) bnd[d][s] = onb(g, d, s, i, j, k);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        // (across a boundary face the cell's own slot, as k_div_G reads the cell itself: the value is not used)
        const int nx_ = bnd[0][s] ? ex : ex + (s ? 1 : -1);
        const int ny_ = bnd[1][s] ? ey : ey + (s ? kSTX : -kSTX);
        const int nz_ = bnd[2][s] ? ez : ez + (s ? kSTX * kSTY : -kSTX * kSTY);
#pragma unroll
        for (int q = 0; q < 3; ++q) { nbv[0][s][q] = sx[q][nx_]; nbv[1][s][q] = sy[q][ny_]; nbv[2][s][q] = sz[q][nz_]; }
    }
    double acc[3];
    div_of_rows(g, bnd, ijk, own, nbv, acc);
    const int c = cidx(g, i, j, k);
    for (int q = 0; q < 3; ++q) divG[3 * (size_t)c + q] = acc[q];
}

// continuousPhaseTurbulence->correct() (pimpleFoamYade.C:101-104) for LESModel Smagorinsky (DPMTurbulenceModels.C:73-74; fv_closures.hpp: smagorinsky_nut).
// grad U is the Gauss-linear gradient k_pre_coupling just wrote.
__global__ __launch_bounds__(256) void k_smagorinsky_nut(FvGeo g, const double* __restrict__ vGrad, double ck, double ce, double delta, double* __restrict__ nut) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= g.Nc) return;
    const int c = t + g.c0;
    delta = geo_delta(g, delta, c);
    double T[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) T[q] = vGrad[9 * (size_t)c + q];
    nut[c] = smagorinsky_nut(T, ck, ce, delta);
}

// epsilonWallFunction: the value imposed on a cell with wall faces is the average over them of the faces' terms (fv_closures.hpp: wall_epsilon_term); on the
// uniform block every y_w is dx / 2
__device__ __forceinline__ double wall_epsilon(const FvGeo& g, const TurbEqn& e, double kc, int c, int i, int j, int k) {
#if FY_FVK_GRADED
    double sum = 0.0;
    int W = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if (e.wall[2 * d + s] && onb(g, d, s, i, j, k)) { sum += wall_epsilon_term(e.cmu75, kc, e.kappa, geo_ywall(g, d, c)); ++W; }
    return sum / (double)W;
#else
    return wall_epsilon_term(e.cmu75, kc, e.kappa, geo_ywall(g, 0, c));
#endif
}

// Transport equations of LESModel kEqn (DPMTurbulenceModels.C:76-77) [OF-6 LES/kEqn/kEqn.C correct()] and RASModel kEpsilon
// (DPMTurbulenceModels.C:70-71) [OF-6 RAS/kEpsilon/kEpsilon.C correct()], see TurbEqn in fv_kernels.hpp:
//   fvm::ddt(alpha, rho, X) + fvm::div(alphaRhoPhi, X) - fvm::laplacian(alpha rho DXEff, X) == Su - fvm::SuSp(c1, X) - fvm::Sp(c2, X)
// then relax(), solve, bound(X, XMin), correctNut().  alpha.oldTime() == alpha (quirk F-Q1, as in UcEqn).  Face diffusivity: linear
// interpolate of the cell field alpha (nu + nut / sigma), boundary alpha_b (nu + nut_b / sigma), as in the momentum equation.
// [OF-6 fvm::SuSp: diag += V max(susp, 0), source -= V min(susp, 0) psi; fvm::Sp: diag += V sp; fvMatrix == volField: source += V field]
__global__ __launch_bounds__(256) void k_assemble_turb(FvGeo g, TurbEqn e, const double* __restrict__ kf, const double* __restrict__ ef,
                                                       const double* __restrict__ alpha, CFace3 alphaf, CFace3 phi, const double* __restrict__ vGrad,
                                                       const double* __restrict__ U, Mom7 M, double* __restrict__ b3, double* __restrict__ x3) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= g.Nc) return;
    int i, j, k; ijk_of(g, t, i, j, k);
    const int c = t + g.c0;
    const double nu = g.nu, dt = g.dt, V = geo_V(g, i, j, k);
    const double aP = alpha[c], nutc = g.nut[c];
    const double* X = e.mode == 1 ? ef : kf;
    const double xc = X[c];
    double dg = aP * V / dt;                                    // fvm::ddt(alpha, X)
    double src = aP * V * xc / dt;
    double sumPhi = 0.0, an[6];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int f = cface(g, d, s, i, j, k);
            const double af = alphaf.a[d][f];
            const double pv = (s ? 1.0 : -1.0) * phi.a[d][f];
            const double phio = af * pv;                          // alphaRhoPhi, outward
            sumPhi += pv;
            if (onb(g, d, s, i, j, k)) {
                an[2 * d + s] = 0.0;
                const int patch = 2 * d + s;
                const double nb = nut_boundary(g, patch, c);
                const double gam = (af * (nu + nb / e.sigma)) * geo_sfd(g, d, s, i, j, k);
                if (e.bc[patch] == 1) {
                    const double gb = kBfac * gam;
                    dg += gb;
                    src += (-phio + gb) * e.val[patch];
                } else {
                    dg += phio;
                }
            } else {
                const int nbc = c + (s ? stride_of(g, d) : -stride_of(g, d));
                const int qc = d == 0 ? i : d == 1 ? j : k;
                const double gam = geo_lerp_side(g, d, s, qc, aP * (nu + nutc / e.sigma), alpha[nbc] * (nu + g.nut[nbc] / e.sigma)) * geo_sfd(g, d, s, i, j, k);
                const double wP = geo_wown(g, d, s, qc);
#if FY_FVK_GRADED
                const double cP = e.upwind ? fmax(phio, 0.0) : wP * phio, cN = e.upwind ? fmin(phio, 0.0) : (1.0 - wP) * phio;
#else
                const double cP = e.upwind ? fmax(phio, 0.0) : wP * phio, cN = e.upwind ? fmin(phio, 0.0) : wP * phio;
#endif
                dg += cP + gam;
                an[2 * d + s] = cN - gam;
            }
        }
    double G = nutc * production_tensor(vGrad + 9 * (size_t)c);      // G = nut (gradU && dev(twoSymm(gradU)))
    // epsilonWallFunction: wall value of G, and (in the epsilon equation) the imposed cell value
    int Wc = 0;
    double Gw = 0.0;
    if (e.mode != 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (e.wall[2 * d + s] && onb(g, d, s, i, j, k)) {
                    const int patch = 2 * d + s;
                    double ub[3];
                    Ub(g, U, c, patch, ub);
                    const double ywall = geo_ywall(g, d, c);
                    // snGrad U = (U_b - U_P) / y: the general mesh multiplies by deltaCoeffs
                    const double d0 = (ub[0] - U[3 * (size_t)c]) / ywall, d1 = (ub[1] - U[3 * (size_t)c + 1]) / ywall, d2 = (ub[2] - U[3 * (size_t)c + 2]) / ywall;
                    Gw += wall_G_term(nut_boundary(g, patch, c), nu, sqrt(d0 * d0 + d1 * d1 + d2 * d2), e.cmu25, kf[c], e.kappa, ywall);
                    ++Wc;
                }
        if (Wc) G = Gw / (double)Wc;
    }
    const double divU = sumPhi * geo_rV(g, i, j, k);
    // the sources by e.mode: 0 kEqn's k, 1 epsilon, 2 kEpsilon's k (fv_closures.hpp); each branch reads only its own fields -- ef is null without kEpsilon
    TurbSource S;
    if (e.mode == 0) S = keqn_k_source(aP, G, divU, e.ce, geo_delta(g, e.delta, c), xc);
    else if (e.mode == 1) S = kepsilon_eps_source(aP, G, divU, e.c1, e.c2, e.c3, xc, kf[c]);
    else S = kepsilon_k_source(aP, G, divU, ef[c], xc);
    add_turb_source(S, V, xc, dg, src);                         // fvm::SuSp + fvm::Sp
    if (e.relax > 0) {                                          // fvMatrix::relax as in UcEqn
        double so = 0.0;
        for (int q = 0; q < 6; ++q) so += fabs(an[q]);
        relax_scalar_row(e.relax, so, xc, dg, src);
    }
    double x0 = xc;
    if (e.mode == 1) {
        // epsEqn.boundaryManipulate -> fvMatrix::setValues(faceCells, value) [OF-6 fvMatrix.C setValuesFromList]
        if (Wc) {
            const double v = wall_epsilon(g, e, kf[c], c, i, j, k);
            for (int q = 0; q < 6; ++q) an[q] = 0.0;
            src = dg * v;
            x0 = v;
        } else {
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    if (!onb(g, d, s, i, j, k)) {
                        const int ni = i + (d == 0 ? (s ? 1 : -1) : 0), nj = j + (d == 1 ? (s ? 1 : -1) : 0), nk = k + (d == 2 ? (s ? 1 : -1) : 0);
                        bool nwall = false;
#pragma unroll
                        for (int d2 = 0; d2 < 3; ++d2)
#pragma unroll
                            for (int s2 = 0; s2 < 2; ++s2) nwall = nwall || (e.wall[2 * d2 + s2] && onb(g, d2, s2, ni, nj, nk));
                        if (nwall) {
                            const int nbc = c + (s ? stride_of(g, d) : -stride_of(g, d));
                            src -= an[2 * d + s] * wall_epsilon(g, e, kf[nbc], nbc, ni, nj, nk);
                            an[2 * d + s] = 0.0;
                        }
                    }
        }
    }
    M.diag[c] = dg;
    for (int q = 0; q < 6; ++q) M.an[q][c] = an[q];
    b3[3 * (size_t)c] = src; b3[3 * (size_t)c + 1] = 0.0; b3[3 * (size_t)c + 2] = 0.0;
    x3[3 * (size_t)c] = x0; x3[3 * (size_t)c + 1] = 0.0; x3[3 * (size_t)c + 2] = 0.0;
}

// bound(X, XMin) (fv_closures.hpp: bound_value) -- the identity where X >= XMin, so it is applied without the global min test OpenFOAM guards it
// with -- then correctNut (see launch_turb_finish)
__global__ __launch_bounds__(256) void k_turb_finish(FvGeo g, TurbEqn e, const double* __restrict__ x3, double* __restrict__ Xf, int nut_mode, double cmu,
                                                     const double* __restrict__ ef, double* __restrict__ nut) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= g.Nc) return;
    int i, j, k; ijk_of(g, t, i, j, k);
    const int c = t + g.c0;
    const double xc = x3[3 * (size_t)c];
    double avg = xc;
    if (!(xc > 0.0)) {                                          // pos0(-X) = 1: the face-area average of the bounded neighbourhood
        const double mP = fmax(xc, e.xmin);
        double av = 0.0;
#if FY_FVK_GRADED
        double asum = 0.0;                                      // fvc::average: sum |Sf| x_f / sum |Sf|
#endif
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                double xf;
                if (onb(g, d, s, i, j, k)) {
                    const int patch = 2 * d + s;
                    xf = fmax(e.bc[patch] == 1 ? e.val[patch] : xc, e.xmin);
                } else {
                    const int nbc = c + (s ? stride_of(g, d) : -stride_of(g, d));
                    xf = geo_lerp_side(g, d, s, d == 0 ? i : d == 1 ? j : k, mP, fmax(x3[3 * (size_t)nbc], e.xmin));
                }
#if FY_FVK_GRADED
                const double Afc = geo_Af(g, d, i, j, k);
                av += Afc * xf; asum += Afc;
#else
                av += xf;
#endif
            }
#if FY_FVK_GRADED
        avg = av / asum;
#else
        avg = av / 6.0;                                         // (six equal faces)
#endif
    }
    const double xb = bound_value(xc, avg, e.xmin);
    Xf[c] = xb;
    if (nut_mode == 1) nut[c] = nut_keqn(e.ck, xb, geo_delta(g, e.delta, c));
    else if (nut_mode == 2) nut[c] = nut_kepsilon(cmu, xb, ef[c]);
}

// The fluid temperature equation (fy_thermal_desc; a capability the reference does not have -- DESIGN_FV.md "T equation"), next to the turbulence transport
// equations and assembled like them into the momentum matrix's storage as the {X, 0, 0} system:
//   alpha V (T - T_old) / dt + sum_f F_f T_f - T sum_f F_f - sum_f alpha_f Deff_f |S_f| / |d_f| (T_N - T) = (Su - Sp T) / (rho_f cp)
// F_f = alpha_f phi_f outward (alpha == nullptr: icoFoamYade, alpha = 1), the convection in its bounded form, T_f linear | upwind, alpha_f and Deff_f = D + nut / Prt
// the linear interpolates (alpha_f = 1 on a boundary face: the calculated patch's value, as in UcEqn), alpha.oldTime() == alpha (quirk F-Q1).  fixedValue side: half-cell
// distance and F_b T_b; zeroGradient side: T_b = T.  Sp, Su: what the particles' heat exchange scattered (W/K, W; nullptr: none)
__global__ __launch_bounds__(256) void k_assemble_scalar(FvGeo g, ScalarEqn e, const double* __restrict__ Tf, const double* __restrict__ alpha, CFace3 phi,
                                                         const double* __restrict__ Sp, const double* __restrict__ Su, Mom7 M, double* __restrict__ b3,
                                                         double* __restrict__ x3) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= g.Nc) return;
    int i, j, k; ijk_of(g, t, i, j, k);
    const int c = t + g.c0;
    const double dt = g.dt, V = geo_V(g, i, j, k);
    const double aP = alpha ? alpha[c] : 1.0;
    const double dP = e.D + (g.nut ? g.nut[c] * e.rPrt : 0.0);
    const double xc = Tf[c];
    double dg = aP * V / dt;                                    // fvm::ddt(alpha, T)
    double src = aP * V * xc / dt;
    double sumF = 0.0, an[6];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int f = cface(g, d, s, i, j, k);
            const double pv = (s ? 1.0 : -1.0) * phi.a[d][f];
            if (onb(g, d, s, i, j, k)) {
                an[2 * d + s] = 0.0;
                const int patch = 2 * d + s;
                const double F = pv;                              // alpha_f = 1 on the boundary
                sumF += F;
                if (e.bc[patch] == 1) {
                    const double db = e.D + (g.nut ? nut_boundary(g, patch, c) * e.rPrt : 0.0);
                    const double gb = kBfac * (db * geo_sfd(g, d, s, i, j, k));
                    dg += gb;
                    src += (gb - F) * e.val[patch];
                } else {
                    dg += F;
                }
            } else {
                const int nbc = c + (s ? stride_of(g, d) : -stride_of(g, d));
                const int qc = d == 0 ? i : d == 1 ? j : k;
                const double af = geo_lerp_side(g, d, s, qc, aP, alpha ? alpha[nbc] : 1.0);
                const double df = geo_lerp_side(g, d, s, qc, dP, e.D + (g.nut ? g.nut[nbc] * e.rPrt : 0.0));
                const double gam = (af * df) * geo_sfd(g, d, s, i, j, k);
                const double F = af * pv;
                sumF += F;
                const double wP = geo_wown(g, d, s, qc);
                const double cP = e.upwind ? fmax(F, 0.0) : wP * F, cN = e.upwind ? fmin(F, 0.0) : (1.0 - wP) * F;
                dg += cP + gam;
                an[2 * d + s] = cN - gam;
            }
        }
    dg -= sumF;                                                 // bounded convection: - T div(F)
    if (Sp) { dg += Sp[c] * e.rRhoCp; src += Su[c] * e.rRhoCp; }
    M.diag[c] = dg;
    for (int q = 0; q < 6; ++q) M.an[q][c] = an[q];
    b3[3 * (size_t)c] = src; b3[3 * (size_t)c + 1] = 0.0; b3[3 * (size_t)c + 2] = 0.0;
    x3[3 * (size_t)c] = xc; x3[3 * (size_t)c + 1] = 0.0; x3[3 * (size_t)c + 2] = 0.0;
}
// component 0 of the solved {X, 0, 0} system -> the scalar field
__global__ __launch_bounds__(256) void k_scalar_finish(FvGeo g, const double* __restrict__ x3, double* __restrict__ X) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= g.Nc) return;
    const int c = t + g.c0;
    X[c] = x3[3 * (size_t)c];
}


// UEqn (icoFoamYade.C:79-85) / UcEqn + relax (UcEqn.H:3-12): diag, 6 neighbour coefficients, source (no pressure term), rAU = 1/A
// ---- NVD / TVD limited convection schemes for div(phi,U) (fv_closures.hpp: nvd_r, nvd_limiter): one limiter per face from the scalar lPhi = magSqr(U), C the
// upwind cell of the face flux, grad the Gauss-linear gradient (boundary value magSqr(U_b)); the weight of the OWNER's value is limiter * w_linear +
// (1 - limiter) * pos0(faceFlux), used implicitly in the matrix.
__device__ __forceinline__ double magsqr3(const double* __restrict__ F, int c) {
    const double a = F[3 * (size_t)c], b = F[3 * (size_t)c + 1], e = F[3 * (size_t)c + 2];
    return (a * a + b * b) + e * e;
}
__global__ __launch_bounds__(256) void k_grad_magsqr(FvGeo g, const double* __restrict__ U, double* __restrict__ gradL) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= g.Nc) return;
    int i, j, k; ijk_of(g, t, i, j, k);
    const int c = t + g.c0;
    const double lc = magsqr3(U, c);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        double fv[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (onb(g, d, s, i, j, k)) { double b[3]; Ub(g, U, c, 2 * d + s, b); fv[s] = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]; }
            else fv[s] = geo_lerp_side(g, d, s, d == 0 ? i : d == 1 ? j : k, lc, magsqr3(U, c + (s ? stride_of(g, d) : -stride_of(g, d))));
        }
        gradL[3 * (size_t)c + d] = (fv[1] - fv[0]) * geo_rh(g, d, d == 0 ? i : d == 1 ? j : k);
    }
}
// weight of the owner's (low cell's) value on the interior face between own and nei (axis d; qn = the neighbour's index along d); flux: owner -> neighbour
__device__ __forceinline__ double limited_weight(const FvGeo& g, const double* __restrict__ U, const double* __restrict__ gradL, int d, int qn, int own,
                                                 int nei, double flux) {
    const double gradf = magsqr3(U, nei) - magsqr3(U, own);
    const double gradcf = (1.0 / geo_rdelta(g, d, qn)) * gradL[3 * (size_t)(flux > 0 ? own : nei) + d];
    const double lim = nvd_limiter(g.upwind, g.lim_twoByk, nvd_r(gradcf, gradf));
#if FY_FVK_GRADED
    const double wl = geo_wlow(g, d, qn);
#else
    const double wl = 0.5;
#endif
    return lim * wl + (1.0 - lim) * (flux >= 0 ? 1.0 : 0.0);
}

template <bool LIMITED>
__global__ __launch_bounds__(256) void k_assemble_momentum(FvGeo g, const double* __restrict__ U, const double* __restrict__ Uold,
                                                           const double* __restrict__ alpha, const double* __restrict__ alphaOld, CFace3 alphaf,
                                                           CFace3 phi, const double* __restrict__ uSource, const double* __restrict__ uSourceDrag,
                                                           const double* __restrict__ divG, const double* __restrict__ vGrad, Mom7 M,
                                                           double* __restrict__ src, double* __restrict__ rAU, const PorousDev* __restrict__ por) {
    const int t = fv_block(g, blockIdx.x, gridDim.x) * 256 + (int)threadIdx.x;
    if (t >= g.Nc) return;
    int i, j, k; ijk_of(g, t, i, j, k);
    const int c = t + g.c0;
    const double nu = g.nu, dt = g.dt, V = geo_V(g, i, j, k);
    const bool pim = g.pimple != 0;
    const double aP = pim ? alpha[c] : 1.0, aP0 = pim ? alphaOld[c] : 1.0;
    double dg = aP * V / dt;
    double s3[3];
    for (int q = 0; q < 3; ++q) s3[q] = aP0 * V * Uold[3 * (size_t)c + q] / dt;
    double divAPhi = 0.0, an[6];
    double bd[3] = {0.0, 0.0, 0.0};               // per-component boundary diagonal (slip patches; M.bd)
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int f = cface(g, d, s, i, j, k);
            // alphacf streamed from its face array, or (no array kept: alphaf.a[0] == nullptr) re-formed from alpha as interp_alpha_face forms it
            double af = 1.0;
            if (pim) {
                if (alphaf.a[0]) af = alphaf.a[d][f];
                else if (!onb(g, d, s, i, j, k)) af = lerp_face(g, d, s, (d == 0 ? i : d == 1 ? j : k) + s, aP, alpha[c + (s ? stride_of(g, d) : -stride_of(g, d))]);
            }
            const double phio = (s ? 1.0 : -1.0) * af * phi.a[d][f];
            divAPhi += phio;
            // fvm::laplacian(alpha nuEff, U): the face diffusivity is the linear interpolate of the cell field alpha (nu + nut) [OF-6
            // linearViscousStress::divDevRhoReff, gaussLaplacianScheme]; its boundary value is alpha_b (nu + nut_b).  Laminar: nu alphaf
            const double geo = geo_sfd(g, d, s, i, j, k);          // |Sf| / |d| (uniform block: dx; a boundary's factor 2 is kBfac)
            double gam = nu * af * geo;
            if (g.nut) {
                if (onb(g, d, s, i, j, k)) {
                    const double nb = nut_boundary(g, 2 * d + s, c);
                    gam = (af * (nu + nb)) * geo;
                } else {
                    const int nbc = c + (s ? stride_of(g, d) : -stride_of(g, d));
                    gam = geo_lerp_side(g, d, s, d == 0 ? i : d == 1 ? j : k, aP * (nu + g.nut[c]), alpha[nbc] * (nu + g.nut[nbc])) * geo;
                }
            }
            if (onb(g, d, s, i, j, k)) {
                an[2 * d + s] = 0.0;
                const int patch = 2 * d + s;
                if (g.u_bc[patch] == 0) {
                    const double gb = kBfac * gam;
                    dg += gb;
                    double ub[3];
                    u_fixed3(g, patch, c, ub);
                    for (int q = 0; q < 3; ++q) s3[q] += (-phio + gb) * ub[q];
                } else {
                    // symmetryPlane / slip [OF-6 transformFvPatchField::gradientInternalCoeffs with basicSymmetry's snGradTransformDiag]: the
                    // NORMAL component sees a fixed value 0 (implicit coefficient only), the tangential ones a zero gradient
                    if (g.u_bc[patch] == 2) bd[d] += kBfac * gam;
                    dg += phio;
                }
            } else {
                // fvm::div(phi, U): Gauss linear puts half the face flux on either side; Gauss upwind takes the whole of an
                // outgoing flux on the diagonal and the whole of an incoming one on the neighbour [OF-6 gaussConvectionScheme]
                const double wP = geo_wown(g, d, s, d == 0 ? i : d == 1 ? j : k);      // Gauss linear: w_P U_P + (1 - w_P) U_N at the face
#if FY_FVK_GRADED
                double cP = g.upwind ? fmax(phio, 0.0) : wP * phio, cN = g.upwind ? fmin(phio, 0.0) : (1.0 - wP) * phio;
#else
                double cP = g.upwind ? fmax(phio, 0.0) : wP * phio, cN = g.upwind ? fmin(phio, 0.0) : wP * phio;
#endif
                if (LIMITED) {                                 // (vGrad carries grad(magSqr(U)), three per cell)
                    const int nb = c + (s ? stride_of(g, d) : -stride_of(g, d));
                    const int qc = d == 0 ? i : d == 1 ? j : k;
                    const double w = limited_weight(g, U, vGrad, d, qc + s, s ? c : nb, s ? nb : c, af * phi.a[d][f]);
                    cP = s ? phio * w : phio * (1.0 - w);
                    cN = s ? phio * (1.0 - w) : phio * w;
                }
                dg += cP + gam;
                an[2 * d + s] = cN - gam;
                if (g.upwind == 2) {
                    // linearUpwind: implicit upwind + explicit (C_f - C_upwind) . grad(U)_upwind with the current Gauss-linear gradient
                    const int nb = c + (s ? stride_of(g, d) : -stride_of(g, d));
                    const int uw = phio > 0.0 ? c : nb;
                    // (C_f - C_upwind) along d: half the UPWIND cell's extent, towards the face
                    const double half = (phio > 0.0 ? (s ? 0.5 : -0.5) : (s ? -0.5 : 0.5)) * geo_hc(g, d, uw);
                    for (int q = 0; q < 3; ++q) s3[q] -= phio * (half * vGrad[9 * (size_t)uw + 3 * d + q]);
                }
            }
        }
    if (pim) {
        const double S = (alpha[c] - alphaOld[c]) / dt + divAPhi / V;
        dg -= V * S;
        dg -= V * uSourceDrag[c];
        for (int q = 0; q < 3; ++q) s3[q] += V * divG[3 * (size_t)c + q];
        double so = 0.0;
        for (int q = 0; q < 6; ++q) so += fabs(an[q]);
        if (g.u_relax > 0) {
            // fvMatrix::relax(alpha) [OF-6 fvMatrix.C]: D = max(|D|, sum|offdiag|) / alpha (the boundary coefficients, part of dg here all
            // along, take part in the dominance test), source += (D_new - D_old) psi; no factor for the equation: relax() does nothing
            // (a slip patch's coefficient differs by component: relax() adds cmptMax(cmptMag(internalCoeffs)) before the test and takes
            // cmptMin (= 0) off afterwards -- all of it joins the test, the scalar diagonal keeps what the test gave)
            // (a porous zone's coefficient joins the test with its component maximum, beside the boundary part as it stands)
            double dt0 = dg + ((bd[0] + bd[1]) + bd[2]);
            if (por) dt0 += porous_cell_max(por, c, nu, aP * V, U + 3 * (size_t)c);
            const double dn = fmax(fabs(dt0), so) / g.u_relax;
            for (int q = 0; q < 3; ++q) s3[q] += (dn - dg) * U[3 * (size_t)c + q];
            dg = dn;
        }
    } else {
        for (int q = 0; q < 3; ++q) s3[q] += V * uSource[3 * (size_t)c + q];
    }
    M.diag[c] = dg;
    for (int q = 0; q < 6; ++q) M.an[q][c] = an[q];
    for (int q = 0; q < 3; ++q) src[3 * (size_t)c + q] = s3[q];
    // porous zones (porous.hpp; por null: none -- a kernel argument, uniform over the grid): the cell's zone from one byte, and in a zone's cells a V C_q(U) per
    // component around the U the matrix is assembled with, on the per-component diagonal.  Formed here, after the row's stores (and once more inside the dominance
    // test above, in zone cells only), so that no register carries it across the sweep; the zone map is read at the storage index (zones run on one domain: c0 = 0) and a V
    // is formed from the aP the row already holds, so that no scalar register is kept for it either: with no zone the kernel keeps its occupancy
    if (por) {
        double pc[3];
        if (porous_cell(por, c, nu, aP * V, U + 3 * (size_t)c, pc)) for (int q = 0; q < 3; ++q) bd[q] += pc[q];
    }
    // 1 / UEqn.A(): fvMatrix::A() adds the COMPONENT AVERAGE of the boundary diagonal
    double bav = 0.0;
    if (M.bd) { for (int q = 0; q < 3; ++q) M.bd[3 * (size_t)c + q] = bd[q]; bav = ((bd[0] + bd[1]) + bd[2]) / 3.0; }
    rAU[c] = 1.0 / ((dg + bav) / V);
}

// RHS of the momentum predictor: ico  src - V grad(p)            (icoFoamYade.C:91-94)
//                                pimple src + V reconstruct(phicForces/rAUcf - snGrad(p) magSf)   (UcEqn.H:22-33)
__global__ __launch_bounds__(256) void k_bmom(FvGeo g, const double* __restrict__ src, const double* __restrict__ p, CFace3 psn,
                                              CFace3 phiForces, CFace3 rAUf, double* __restrict__ bmom) {
    const int t = fv_block(g, blockIdx.x, gridDim.x) * 256 + (int)threadIdx.x;
    if (t >= g.Nc) return;
    int i, j, k; ijk_of(g, t, i, j, k);
    const int c = t + g.c0;
    double out[3];      // stored together at the end: component stores issued far apart reach HBM as three partial-line writes
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if (!g.pimple) {
            double fv[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (onb(g, d, s, i, j, k)) fv[s] = pbv(g, p, psn, c, d, s, cface(g, d, s, i, j, k));
                else fv[s] = geo_lerp_side(g, d, s, d == 0 ? i : d == 1 ? j : k, p[c], p[c + (s ? stride_of(g, d) : -stride_of(g, d))]);
            }
            out[d] = src[3 * (size_t)c + d] - geo_V(g, i, j, k) * ((fv[1] - fv[0]) * geo_rh(g, d, d == 0 ? i : d == 1 ? j : k));
        } else {
            double sm = 0;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int f = cface(g, d, s, i, j, k);
                double sng;
                const double rds = geo_rdist(g, d, s, i, j, k);
                if (onb(g, d, s, i, j, k)) { const double pbd = pbv(g, p, psn, c, d, s, f); sng = s ? (pbd - p[c]) * rds : (p[c] - pbd) * rds; }
                else sng = s ? (p[c + stride_of(g, d)] - p[c]) * rds : (p[c] - p[c - stride_of(g, d)]) * rds;
                sm += phiForces.a[d][f] / rAUf.a[d][f] - sng * geo_Af(g, d, i, j, k);
            }
            out[d] = src[3 * (size_t)c + d] + geo_V(g, i, j, k) * (sm / (2.0 * geo_Af(g, d, i, j, k)));
        }
    }
    for (int d = 0; d < 3; ++d) bmom[3 * (size_t)c + d] = out[d];
}

// pimple: rAUcf / phicForces (UcEqn.H:15-20) and the momentum predictor's right-hand side (UcEqn.H:22-33) in one gather-first sweep:
// k_rAUf_phi_forces_cells + k_bmom without the two face fields being read back; a cell forms its six faces' rAUcf and phicForces itself (same
// expressions as rAUf_phi_forces_face), the face's owner stores phicForces (and rAUcf where somebody still streams it: rf_out.a[0] != nullptr)
__global__ __launch_bounds__(256) void k_bmom_faces(FvGeo g, const double* __restrict__ rAU, const double* __restrict__ uSource, const double* __restrict__ src,
                                                    const double* __restrict__ p, CFace3 psn, Face3 rf_out, Face3 pf_out, double* __restrict__ bmom) {
    const int t = fv_block(g, blockIdx.x, gridDim.x) * 256 + (int)threadIdx.x;
    if (t >= g.Nc) return;
    int i, j, k; ijk_of(g, t, i, j, k);
    const int c = t + g.c0;
    const int ijk[3] = {i, j, k};
    bool bnd[3][2]; int nb[3][2], fx[3][2];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bnd[d][s] = onb(g, d, s, i, j, k);
            nb[d][s] = bnd[d][s] ? c : c + (s ? stride_of(g, d) : -stride_of(g, d));
            fx[d][s] = cface(g, d, s, i, j, k);
        }
    const double rc = rAU[c], pc = p[c];
    const double us[3] = {uSource[3 * (size_t)c], uSource[3 * (size_t)c + 1], uSource[3 * (size_t)c + 2]};
    const double sr[3] = {src[3 * (size_t)c], src[3 * (size_t)c + 1], src[3 * (size_t)c + 2]};
    double rn[3][2], un[3][2], pn[3][2];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int s = 0; s < 2; ++s) { rn[d][s] = rAU[nb[d][s]]; un[d][s] = uSource[3 * (size_t)nb[d][s] + d]; pn[d][s] = p[nb[d][s]]; }
    double out[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        double sm = 0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int q = ijk[d] + s;
            const int fi = i + (d == 0 ? s : 0), fj = j + (d == 1 ? s : 0), fk = k + (d == 2 ? s : 0);
            const bool b = bnd[d][s];
            const double Afc = geo_Af(g, d, fi, fj, fk);
            const double r = b ? rc : lerp_face(g, d, s, q, rc, rn[d][s]);
            const double fl = b ? 0.0 : lerp_face(g, d, s, q, rc * us[d], rn[d][s] * un[d][s]) * Afc;
            const double pfv = fl + r * (g.g[d] * Afc);
            if (owns_face(g, d, s, i, j, k)) { pf_out.a[d][fx[d][s]] = pfv; if (rf_out.a[0]) rf_out.a[d][fx[d][s]] = r; }
            double sng;
            const double rds = geo_rdist(g, d, s, i, j, k);
            if (b) { const double pbd = pbv(g, p, psn, c, d, s, fx[d][s]); sng = s ? (pbd - pc) * rds : (pc - pbd) * rds; }
            else sng = s ? (pn[d][s] - pc) * rds : (pc - pn[d][s]) * rds;
            sm += pfv / r - sng * geo_Af(g, d, i, j, k);
        }
        out[d] = sr[d] + geo_V(g, i, j, k) * (sm / (2.0 * geo_Af(g, d, i, j, k)));
    }
    for (int d = 0; d < 3; ++d) bmom[3 * (size_t)c + d] = out[d];
}

// One fused Jacobi pass over the 3 velocity components: with x the current iterate, accumulate the L1 residual |b - A x|
// (slots 0..2), the lduMatrix normalisation sum |A x - A xbar| + |b - A xbar| (slots 3..5) and write the next iterate xn.
// WITH_H: the pass also leaves HbyA = rAU H(x) / V of ITS iterate x (k_HbyA's expression in k_HbyA's order: the same bits) -- the pass that finds x
// converged has then done the first corrector's H-operator sweep on the side, for 56 B/cell instead of a sweep of 128
template <bool WITH_H>
__global__ __launch_bounds__(256) void k_mom_pass(FvGeo g, Mom7 M, const double* __restrict__ b, const double* __restrict__ x,
                                                  double* __restrict__ xn, const double* __restrict__ xsum, double n_glob, double* __restrict__ partials,
                                                  const double* __restrict__ hsrc, const double* __restrict__ rAU, double* __restrict__ HbyA) {
    double v[6] = {0, 0, 0, 0, 0, 0};
    // xbar = average(x) (lduMatrix::solver::normFactor): the component sums stay on the device (k_sum3 + fold [+ all-reduce]); dividing
    // them here saves the host round trip the average used to make
    const double xb[3] = {xsum[0] / n_glob, xsum[1] / n_glob, xsum[2] / n_glob};
    FY_RED_LOOP_G(g, t) {
        int i, j, k; ijk_of(g, t, i, j, k);
        const int c = t + g.c0;
        const double dg = M.diag[c];
        double dq[3] = {dg, dg, dg};                      // (fvMatrix::solveSegregated: addBoundaryDiag per component)
        if (M.bd) for (int q = 0; q < 3; ++q) dq[q] += M.bd[3 * (size_t)c + q];
        double off[3] = {0, 0, 0}, rowsum = dg;
        const double xc[3] = {x[3 * (size_t)c], x[3 * (size_t)c + 1], x[3 * (size_t)c + 2]};
        double hacc[3] = {0, 0, 0};
        if (WITH_H) { hacc[0] = hsrc[3 * (size_t)c]; hacc[1] = hsrc[3 * (size_t)c + 1]; hacc[2] = hsrc[3 * (size_t)c + 2]; }
        double xx[2][3];
        x_neighbours3(x, c, i, g.nx, xc, xx[0], xx[1]);
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (!onb(g, d, s, i, j, k)) {
                    const int nb = c + (s ? stride_of(g, d) : -stride_of(g, d));
                    const double a = M.an[2 * d + s][c];
                    rowsum += a;
                    double xv[3];
                    if (d == 0) for (int q = 0; q < 3; ++q) xv[q] = xx[s][q];
                    else for (int q = 0; q < 3; ++q) xv[q] = x[3 * (size_t)nb + q];
                    for (int q = 0; q < 3; ++q) off[q] += a * xv[q];
                    if (WITH_H) for (int q = 0; q < 3; ++q) hacc[q] -= a * xv[q];
                }
        if (WITH_H) {
            if (M.bd) {
                const double b0 = M.bd[3 * (size_t)c], b1 = M.bd[3 * (size_t)c + 1], b2 = M.bd[3 * (size_t)c + 2];
                const double bav = ((b0 + b1) + b2) / 3.0;
                hacc[0] += (bav - b0) * xc[0]; hacc[1] += (bav - b1) * xc[1]; hacc[2] += (bav - b2) * xc[2];
            }
            const double r = rAU[c];
            for (int q = 0; q < 3; ++q) HbyA[3 * (size_t)c + q] = r * (hacc[q] * geo_rV(g, i, j, k));
        }
        for (int q = 0; q < 3; ++q) {
            const double bq = b[3 * (size_t)c + q];
            const double Ax = dq[q] * xc[q] + off[q];
            const double Aref = (rowsum + (dq[q] - dg)) * xb[q];
            v[q] += fabs(bq - Ax);
            v[3 + q] += fabs(Ax - Aref) + fabs(bq - Aref);
            xn[3 * (size_t)c + q] = (bq - off[q]) / dq[q];
        }
    }
    const int mx[6] = {0, 0, 0, 0, 0, 0};
    block_reduce_store<6>(v, mx, partials, fy_lb, fy_stride);
}

// HbyA = rAU * UEqn.H() (icoFoamYade.C:100, pEqn.H:2)
__global__ __launch_bounds__(256) void k_HbyA(FvGeo g, Mom7 M, const double* __restrict__ src, const double* __restrict__ U,
                                              const double* __restrict__ rAU, double* __restrict__ HbyA) {
    const int t = fv_block(g, blockIdx.x, gridDim.x) * 256 + (int)threadIdx.x;
    if (t >= g.Nc) return;
    int i, j, k; ijk_of(g, t, i, j, k);
    const int c = t + g.c0;
    double acc[3] = {src[3 * (size_t)c], src[3 * (size_t)c + 1], src[3 * (size_t)c + 2]};
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if (!onb(g, d, s, i, j, k)) {
                const int nb = c + (s ? stride_of(g, d) : -stride_of(g, d));
                const double a = M.an[2 * d + s][c];
                for (int q = 0; q < 3; ++q) acc[q] -= a * U[3 * (size_t)nb + q];
            }
    if (M.bd) {
        // fvMatrix::H(): per component (component-averaged boundary diagonal - that component's) * psi
        const double b0 = M.bd[3 * (size_t)c], b1 = M.bd[3 * (size_t)c + 1], b2 = M.bd[3 * (size_t)c + 2];
        const double bav = ((b0 + b1) + b2) / 3.0;
        acc[0] += (bav - b0) * U[3 * (size_t)c]; acc[1] += (bav - b1) * U[3 * (size_t)c + 1]; acc[2] += (bav - b2) * U[3 * (size_t)c + 2];
    }
    const double r = rAU[c];
    for (int q = 0; q < 3; ++q) HbyA[3 * (size_t)c + q] = r * (acc[q] * geo_rV(g, i, j, k));
}

// pEqn in SPD form: sum_f g_f (p_P - p_nb) [+ g_b (p_P - p_b)] = -(ddt(alpha) V + sum_out alphaf phiHbyA)   (icoFoamYade.C:118-123, pEqn.H:26-33)
// MATRIX = false: the right-hand side alone -- the second PISO corrector (and the non-orthogonal correctors) solve with the SAME matrix
// (rAU, alphacf have not changed), so the four coefficient arrays are neither recomputed nor rewritten and rAUf is read only where the
// right-hand side itself needs it (fixedFluxPressure / fixedValue boundary faces, the reference cell).  Same expressions, same bits.
template <bool MATRIX>
__global__ __launch_bounds__(256) void k_assemble_pressure(FvGeo g, CFace3 phiHbyA, CFace3 rAUf, CFace3 alphaf, CFace3 psn,
                                                           const double* __restrict__ alpha, const double* __restrict__ alphaOld, PMat A,
                                                           double* __restrict__ rhs) {
    const int t = fv_block(g, blockIdx.x, gridDim.x) * 256 + (int)threadIdx.x;
    if (t >= g.Nc) return;
    int i, j, k; ijk_of(g, t, i, j, k);
    const int c = t + g.c0;
    // fvMatrix::setReference: p_ref_cell is a GLOBAL cell number (i + nx*(j + ny*kglob))
    const bool refc = g.need_ref && (i + g.nx * (j + g.ny * (k + g.kglob0))) == g.p_ref_cell;
    double dg = 0.0, r = 0.0, up[3] = {0, 0, 0};
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int f = cface(g, d, s, i, j, k);
            const double af = g.pimple ? alphaf.a[d][f] : 1.0;
            double ph = (s ? 1.0 : -1.0) * af * phiHbyA.a[d][f];
            const bool b = onb(g, d, s, i, j, k);
            if (b && g.p_bc[2 * d + s] == 2) ph = (s ? 1.0 : -1.0) * af * (phiHbyA.a[d][f] - rAUf.a[d][f] * geo_Af(g, d, i, j, k) * psn.a[d][f]);
            r -= ph;
            if (b) {
                const int patch = 2 * d + s;
                if (g.p_bc[patch] == 1) { const double gb = kBfac * af * rAUf.a[d][f] * geo_sfd(g, d, s, i, j, k); dg += gb; r += gb * g.p_val[patch]; }
            } else if (MATRIX || refc) {
                const double gg = af * rAUf.a[d][f] * geo_sfd(g, d, s, i, j, k);
                dg += gg;
                if (s) up[d] = gg;
            }
        }
    if (g.pimple) r -= geo_V(g, i, j, k) * (alpha[c] - alphaOld[c]) / g.dt;
    if (refc) { r += dg * g.p_ref_value; dg += dg; }
    if (MATRIX) { A.diag[c] = dg; A.ux[c] = up[0]; A.uy[c] = up[1]; A.uz[c] = up[2]; }
    rhs[c] = r;
}

// slab interface below the first owned plane: its z-face coefficient goes to the ghost cell under it (read by p_row as uz[c - sz])
__global__ __launch_bounds__(256) void k_p_ghost_uz(FvGeo g, CFace3 rAUf, CFace3 alphaf, PMat A) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= g.nx * g.ny) return;
    const double af = g.pimple ? alphaf.a[2][t] : 1.0;           // z-face plane kf = 0
    A.uz[g.c0 - g.nx * g.ny + t] = af * rAUf.a[2][t] * g.dx;
}

// continuityErrs.H:32-46: contErr = [ddt(alpha) +] div([alphaf] phi); slots 0 = sum |contErr| V, 1 = sum contErr V
__global__ __launch_bounds__(256) void k_cont_err(FvGeo g, CFace3 phi, CFace3 alphaf, const double* __restrict__ alpha,
                                                  const double* __restrict__ alphaOld, double* __restrict__ partials) {
    double v[2] = {0, 0};
    FY_RED_LOOP_G(g, t) {
        int i, j, k; ijk_of(g, t, i, j, k);
        const int c = t + g.c0;
        double dv = 0;
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int s = 0; s < 2; ++s) { const int f = cface(g, d, s, i, j, k); dv += (s ? 1.0 : -1.0) * (g.pimple ? alphaf.a[d][f] : 1.0) * phi.a[d][f]; }
        double ce = dv * geo_rV(g, i, j, k);
        if (g.pimple) ce += (alpha[c] - alphaOld[c]) / g.dt;
        v[0] += fabs(ce) * geo_V(g, i, j, k);
        v[1] += ce * geo_V(g, i, j, k);
    }
    const int mx[2] = {0, 0};
    block_reduce_store<2>(v, mx, partials, fy_lb, fy_stride);
}

// ico:    U = HbyA - rAU*fvc::grad(p)                                                         icoFoamYade.C:136
// pimple: Uc = HbyA + rAUc*fvc::reconstruct((phicForces - pEqn.flux()/alphacf)/rAUcf)         pEqn.H:43-45
// DIAG: the same pass also forms the two per-cell diagnostics of the corrected flux that used to be sweeps of their own -- the continuity
// errors (continuityErrs.H:32-46, k_cont_err; slots 0, 1) and the Courant sums of the NEXT pass of the time loop (CourantNo.H:32-49,
// k_courant; slots 2 = max, 3 = sum: phi does not change between the last corrector and the next runTime++).  Same per-cell expressions
// and the same block partition as the stand-alone kernels, so the folded values are the same bits.
template <bool DIAG>
__global__ __launch_bounds__(256) void k_U_correct(FvGeo g, const double* __restrict__ HbyA, const double* __restrict__ rAU,
                                                   const double* __restrict__ p, CFace3 psn, CFace3 phiForces, CFace3 pflux, CFace3 alphaf,
                                                   CFace3 rAUf, double* __restrict__ U, CFace3 phi, const double* __restrict__ alpha,
                                                   const double* __restrict__ alphaOld, double* __restrict__ partials) {
    double v[4] = {0, 0, 0, 0};
    FY_RED_LOOP_G(g, t) {
        int i, j, k; ijk_of(g, t, i, j, k);
        const int c = t + g.c0;
        const double r = rAU[c];
        double out[3];      // see k_bmom
        double dv = 0.0, sp = 0.0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (!g.pimple) {
                double fv[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (onb(g, d, s, i, j, k)) fv[s] = pbv(g, p, psn, c, d, s, cface(g, d, s, i, j, k));
                    else fv[s] = geo_lerp_side(g, d, s, d == 0 ? i : d == 1 ? j : k, p[c], p[c + (s ? stride_of(g, d) : -stride_of(g, d))]);
                }
                out[d] = HbyA[3 * (size_t)c + d] - r * ((fv[1] - fv[0]) * geo_rh(g, d, d == 0 ? i : d == 1 ? j : k));
            } else {
                double sm = 0;
#pragma unroll
                for (int s = 0; s < 2; ++s) sm += pflux.a[d][cface(g, d, s, i, j, k)];          // (phicForces - pEqn.flux() / alphacf) / rAUcf, formed by flux_correct_face
                out[d] = HbyA[3 * (size_t)c + d] + r * (sm / (2.0 * geo_Af(g, d, i, j, k)));
            }
            if (DIAG) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int f = cface(g, d, s, i, j, k);
                    const double ph = phi.a[d][f];
                    dv += (s ? 1.0 : -1.0) * (g.pimple ? alphaf.a[d][f] : 1.0) * ph;
                    sp += fabs(ph);
                }
            }
        }
        for (int d = 0; d < 3; ++d) U[3 * (size_t)c + d] = out[d];
        if (DIAG) {
            double ce = dv * geo_rV(g, i, j, k);
            if (g.pimple) ce += (alpha[c] - alphaOld[c]) / g.dt;
            v[0] += fabs(ce) * geo_V(g, i, j, k);
            v[1] += ce * geo_V(g, i, j, k);
            v[2] = fmax(v[2], sp * geo_rV(g, i, j, k));
            v[3] += sp;
        }
    }
    if (DIAG) {
        const int mx[4] = {0, 0, 1, 0};
        block_reduce_store<4>(v, mx, partials, fy_lb, fy_stride);
    }
}

// ------------------------------------------------------------------------------------------------ fused corrector sweeps (round 5)
// The corrector used to be five cell-centred sweeps -- phiHbyA, pressure assembly, PCG's r0 = b - A p, flux correction, velocity correction --
// each of which handed its face fields to the next through HBM (phiHbyA 24, psn, the flux term 24, rAUf / alphaf streamed by every one of them,
// the matrix read back by k_p_init: SURVEY.md 8(d) prices a corrector at 504 B/cell, the five sweeps moved 730 - 800).  Here a cell forms the
// values of ALL SIX of its faces itself -- same expressions, same operands, same order as the face functions above, so the same bits on both
// sides of a face -- and uses them at once; only what a later pass needs is stored, by the face's owner (the cell on its high side; the low-side
// cell for the last face of a row).  The neighbour values a cell needs twice as often come out of L1 / L2, not HBM.
// FaceSrc: a linear face interpolate (alphacf, rAUf) either streamed from its face array or re-formed from the cell field (8 B/cell instead
// of 24; the expression of the kernel that fills the array)
struct FaceSrc { CFace3 arr; const double* cell; };
template <int D>
__device__ __forceinline__ double alphaf_at(const FvGeo& g, const FaceSrc& a, size_t f, int fi, int fj, int fk) {
    if (!a.cell) return a.arr.a[D][f];
    const int q = D == 0 ? fi : D == 1 ? fj : fk;
    if (face_low_b(g, D, q) || face_high_b(g, D, q)) return 1.0;      // interp_alpha_face
    const int c = cidx(g, fi, fj, fk);
    return geo_lerp(g, D, q, a.cell[c - stride_of(g, D)], a.cell[c]);
}
template <int D>
__device__ __forceinline__ double rAUf_at(const FvGeo& g, const FaceSrc& a, size_t f, int fi, int fj, int fk) {
    if (!a.cell) return a.arr.a[D][f];
    const int q = D == 0 ? fi : D == 1 ? fj : fk;
    if (face_low_b(g, D, q)) return a.cell[cidx(g, fi, fj, fk)];     // k_interp_rAU / rAUf_phi_forces_face
    if (face_high_b(g, D, q)) return a.cell[cidx(g, fi - (D == 0), fj - (D == 1), fk - (D == 2))];
    const int c = cidx(g, fi, fj, fk);
    return geo_lerp(g, D, q, a.cell[c - stride_of(g, D)], a.cell[c]);
}
// CALL(D, S, fi, fj, fk): the six faces of cell (i, j, k) in the order every per-cell sum over faces uses (x-, x+, y-, y+, z-, z+)
#define FY_ALL_FACES(i, j, k, CALL) \
    do { CALL(0, 0, i, j, k); CALL(0, 1, i + 1, j, k); CALL(1, 0, i, j, k); CALL(1, 1, i, j + 1, k); CALL(2, 0, i, j, k); CALL(2, 1, i, j, k + 1); } while (0)

// Both sweeps are written GATHER FIRST: every operand of the six faces is loaded up front from an address that is always valid (across a
// boundary face the "neighbour" is the cell itself), then the faces are evaluated from registers.  Written face by face -- a branch per face
// with its loads inside -- a wave makes one dependent memory round trip per face and more (the first version of these kernels: 385 us for what
// the three sweeps it replaced did in 396; 825 VALU instructions and 70 loads per wave, 3 % of the cycles waiting on anything but memory).
// Only what boundary faces alone need (psn, U at a fixedFluxPressure patch) stays behind a branch: interior waves skip it.

// value of a vector field's component d at a boundary face, from the field's own-cell value (Ub, component d: patch >> 1 == d here)
__device__ __forceinline__ double ub_normal(const FvGeo& g, int patch, int d, int c, double own_d) {
    return g.u_bc[patch] == 0 ? u_fixed(g, patch, c, d) : (g.u_bc[patch] == 2 ? 0.0 : own_d);
}
// flux correction + velocity correction [+ continuity errors + the next pass's Courant sums] in one sweep (icoFoamYade.C:127-137, pEqn.H:39-45,
// continuityErrs.H, CourantNo.H): k_flux_correct_cells and k_U_correct<DIAG> without the face field between them
template <bool DIAG, bool FFC>
__global__ __launch_bounds__(256) void k_corr_back(FvGeo g, const double* __restrict__ p, CFace3 phiHbyA, FaceSrc rAUf, FaceSrc alphaf, CFace3 psn,
                                                   CFace3 phiForces, Face3 phi, const double* __restrict__ HbyA, const double* __restrict__ rAU,
                                                   double* __restrict__ U, const double* __restrict__ alpha, const double* __restrict__ alphaOld,
                                                   double* __restrict__ partials) {
    double v[4] = {0, 0, 0, 0};
    FY_RED_LOOP_G(g, t) {
        int i, j, k; ijk_of(g, t, i, j, k);
        const int c = t + g.c0;
        const int ijk[3] = {i, j, k};
        const bool pim = g.pimple != 0;
        // ---- gather
        bool bnd[3][2]; int nb[3][2], fx[3][2];
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                bnd[d][s] = onb(g, d, s, i, j, k);
                nb[d][s] = bnd[d][s] ? c : c + (s ? stride_of(g, d) : -stride_of(g, d));
                fx[d][s] = cface(g, d, s, i, j, k);
            }
        const double pc = p[c], rc = rAU[c], ac = pim ? alpha[c] : 1.0;
        const double hb[3] = {HbyA[3 * (size_t)c], HbyA[3 * (size_t)c + 1], HbyA[3 * (size_t)c + 2]};
        double pn[3][2], rfv[3][2], afv[3][2], phh[3][2], pfo[3][2];
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                pn[d][s] = p[nb[d][s]];
                phh[d][s] = phiHbyA.a[d][fx[d][s]];
                pfo[d][s] = pim ? phiForces.a[d][fx[d][s]] : 0.0;
                if (FFC) { rfv[d][s] = rAU[nb[d][s]]; afv[d][s] = pim ? alpha[nb[d][s]] : 1.0; }
                else { rfv[d][s] = rAUf.arr.a[d][fx[d][s]]; afv[d][s] = pim ? alphaf.arr.a[d][fx[d][s]] : 1.0; }
            }
        // ---- the six faces (flux_correct_face's expressions)
        double pfl[3][2], ph[3][2];
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int q = ijk[d] + s;                       // the face's index along d
                const int fi = i + (d == 0 ? s : 0), fj = j + (d == 1 ? s : 0), fk = k + (d == 2 ? s : 0);
                const bool b = bnd[d][s];
                if (FFC) {
                    afv[d][s] = pim ? (b ? 1.0 : lerp_face(g, d, s, q, ac, afv[d][s])) : 1.0;          // interp_alpha_face
                    rfv[d][s] = b ? rc : lerp_face(g, d, s, q, rc, rfv[d][s]);                           // k_interp_rAU / rAUf_phi_forces_face
                }
                const double af = afv[d][s], rf = rfv[d][s];
                double fl = 0.0;
                if (b) {
                    const int patch = 2 * d + s;
                    if (g.p_bc[patch] == 1) { const double gb = kBfac * af * rf * geo_sfd_face(g, d, q, ndim(g, d), fi, fj, fk); fl = s ? gb * (g.p_val[patch] - pc) : gb * (pc - g.p_val[patch]); }
                    else if (g.p_bc[patch] == 2) fl = af * rf * geo_Af(g, d, fi, fj, fk) * psn.a[d][fx[d][s]];
                } else {
                    fl = af * rf * geo_sfd_face(g, d, q, ndim(g, d), fi, fj, fk) * (s ? pn[d][s] - pc : pc - pn[d][s]);
                }
                const double fa = fl / af;
                pfl[d][s] = pim ? (pfo[d][s] - fa) / rf : fl;
                ph[d][s] = phh[d][s] - fa;
                if (owns_face(g, d, s, i, j, k)) phi.a[d][fx[d][s]] = ph[d][s];
            }
        // ---- the velocity correction and the diagnostics (k_U_correct's expressions)
        double out[3];
        double dv = 0.0, sp = 0.0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (!pim) {
                double fv[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (bnd[d][s]) fv[s] = pbv(g, p, psn, c, d, s, fx[d][s]);
                    else fv[s] = geo_lerp_side(g, d, s, ijk[d], pc, pn[d][s]);
                }
                out[d] = hb[d] - rc * ((fv[1] - fv[0]) * geo_rh(g, d, ijk[d]));
            } else {
                double sm = 0;
#pragma unroll
                for (int s = 0; s < 2; ++s) sm += pfl[d][s];
                out[d] = hb[d] + rc * (sm / (2.0 * geo_Af(g, d, i, j, k)));
            }
            if (DIAG) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    dv += (s ? 1.0 : -1.0) * (pim ? afv[d][s] : 1.0) * ph[d][s];
                    sp += fabs(ph[d][s]);
                }
            }
        }
        for (int d = 0; d < 3; ++d) U[3 * (size_t)c + d] = out[d];
        if (DIAG) {
            double ce = dv * geo_rV(g, i, j, k);
            if (pim) ce += (ac - alphaOld[c]) / g.dt;
            v[0] += fabs(ce) * geo_V(g, i, j, k);
            v[1] += ce * geo_V(g, i, j, k);
            v[2] = fmax(v[2], sp * geo_rV(g, i, j, k));
            v[3] += sp;
        }
    }
    if (DIAG) {
        const int mx[4] = {0, 0, 1, 0};
        block_reduce_store<4>(v, mx, partials, fy_lb, fy_stride);
    }
}

// phiHbyA + constrainPressure, the pressure equation's assembly and PCG's first residual r0 = b - A p with its norm factor in one sweep
// (icoFoamYade.C:101-123, pEqn.H:4-33, PCG.C [OF-6]): k_phiHbyA_cells<KEEP>, k_assemble_pressure and k_p_init without phiHbyA, psn and the matrix
// being read back in between.  The residual's row uses the face coefficients in p_row's order (x-, x+, y-, y+, z-, z+; a boundary face's stored
// coefficient is 0 there, skipped here) and the block partition of k_p_init, so r0 and the two sums are k_p_init's bits.
// dcorr: the old-time part of the ddtCorr term per face, left by k_pre_coupling at the start of the step (coef / deltaT (phi.old - flux(U.old)));
// the term itself is rAUf dcorr [alphacf], the same product in every corrector.  STORE_A = false: a later corrector of the same momentum
// assembly -- the matrix in A stands (same rAU, same alphacf).  Register cap: room for 4 waves per SIMD (measured per kernel; the other gather-first
// sweeps keep the compiler's own choice)
template <bool STORE_A, bool FFC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_corr_front(FvGeo g, const double* __restrict__ HbyA, const double* __restrict__ U, CFace3 dcorr,
                                                    FaceSrc rAUf, FaceSrc alphaf, CFace3 phiForces, Face3 phiHbyA, Face3 psn,
                                                    const double* __restrict__ rAU, const double* __restrict__ alpha, const double* __restrict__ alphaOld, PMat A,
                                                    double* __restrict__ rhs, const double* __restrict__ x, const double* __restrict__ xbar_dev, double xsum_val,
                                                    double inv_n, double* __restrict__ res, double* __restrict__ partials) {
    double v[2] = {0, 0};
    const double xbar = (xbar_dev ? xbar_dev[0] : xsum_val) * inv_n;
    FY_RED_LOOP_G(g, t) {
        int i, j, k; ijk_of(g, t, i, j, k);
        const int c = t + g.c0;
        const int ijk[3] = {i, j, k};
        const bool pim = g.pimple != 0;
        const bool refc = g.need_ref && (i + g.nx * (j + g.ny * (k + g.kglob0))) == g.p_ref_cell;
        // ---- gather
        bool bnd[3][2]; int nb[3][2], fx[3][2];
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                bnd[d][s] = onb(g, d, s, i, j, k);
                nb[d][s] = bnd[d][s] ? c : c + (s ? stride_of(g, d) : -stride_of(g, d));
                fx[d][s] = cface(g, d, s, i, j, k);
            }
        const double xc = x[c], ac = pim ? alpha[c] : 1.0;
        const double rc = FFC ? rAU[c] : 0.0;
        const double hb[3] = {HbyA[3 * (size_t)c], HbyA[3 * (size_t)c + 1], HbyA[3 * (size_t)c + 2]};
        double hn[3][2], dc[3][2], pfo[3][2], xn[3][2], rfv[3][2], afv[3][2];
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                hn[d][s] = HbyA[3 * (size_t)nb[d][s] + d];
                dc[d][s] = dcorr.a[d][fx[d][s]];
                pfo[d][s] = pim ? phiForces.a[d][fx[d][s]] : 0.0;
                xn[d][s] = x[nb[d][s]];
                if (FFC) { rfv[d][s] = rAU[nb[d][s]]; afv[d][s] = pim ? alpha[nb[d][s]] : 1.0; }
                else { rfv[d][s] = rAUf.arr.a[d][fx[d][s]]; afv[d][s] = pim ? alphaf.arr.a[d][fx[d][s]] : 1.0; }
            }
        // ---- the six faces: phiHbyA_face, then k_assemble_pressure's terms
        double dg = 0.0, r = 0.0, up[3] = {0, 0, 0};
        double gg6[3][2];                          // coefficient towards the neighbour across face (d, s); 0 on a physical boundary
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int q = ijk[d] + s;
                const int fi = i + (d == 0 ? s : 0), fj = j + (d == 1 ? s : 0), fk = k + (d == 2 ? s : 0);
                const bool b = bnd[d][s];
                const int patch = 2 * d + s;
                if (FFC) {
                    afv[d][s] = pim ? (b ? 1.0 : lerp_face(g, d, s, q, ac, afv[d][s])) : 1.0;
                    rfv[d][s] = b ? rc : lerp_face(g, d, s, q, rc, rfv[d][s]);
                }
                const double af = afv[d][s], rf = rfv[d][s];
                const double Afc = geo_Af(g, d, fi, fj, fk);
                double pv = (b ? ub_normal(g, patch, d, c, hb[d]) : lerp_face(g, d, s, q, hb[d], hn[d][s])) * Afc;      // face_flux_vec(HbyA)
                double add = rf * dc[d][s];
                if (pim) add *= af;
                pv += add;
                if (pim) pv += pfo[d][s];
                const bool own = owns_face(g, d, s, i, j, k);
                if (own) phiHbyA.a[d][fx[d][s]] = pv;
                double ph = (s ? 1.0 : -1.0) * af * pv;
                gg6[d][s] = 0.0;
                if (b) {
                    if (g.p_bc[patch] == 2) {               // constrainPressure (fixedFluxPressure): snGrad(p) from the flux that must pass
                        const double ubd = ub_normal(g, patch, d, c, g.u_bc[patch] == 1 ? U[3 * (size_t)c + d] : 0.0);
                        const double psn_v = (pv - ubd * Afc) / (rf * Afc);
                        if (own) psn.a[d][fx[d][s]] = psn_v;
                        ph = (s ? 1.0 : -1.0) * af * (pv - rf * geo_Af(g, d, i, j, k) * psn_v);
                    }
                    r -= ph;
                    if (g.p_bc[patch] == 1) { const double gb = kBfac * af * rf * geo_sfd(g, d, s, i, j, k); dg += gb; r += gb * g.p_val[patch]; }
                } else {
                    r -= ph;
                    const double gg = af * rf * geo_sfd(g, d, s, i, j, k);
                    dg += gg; gg6[d][s] = gg;
                    if (s) up[d] = gg;
                }
            }
        if (pim) r -= geo_V(g, i, j, k) * (ac - alphaOld[c]) / g.dt;
        if (refc) { r += dg * g.p_ref_value; dg += dg; }
        if (STORE_A) { A.diag[c] = dg; A.ux[c] = up[0]; A.uy[c] = up[1]; A.uz[c] = up[2]; }
        rhs[c] = r;
        // ---- r0 = b - A x, sum |r0|, the norm factor's sum (k_p_init)
        double Ax = dg * xc, rs = dg;
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (!bnd[d][s]) { Ax -= gg6[d][s] * xn[d][s]; rs -= gg6[d][s]; }
        const double Aref = rs * xbar;
        const double rr = r - Ax;
        res[c] = rr;
        v[0] += fabs(rr);
        v[1] += fabs(Ax - Aref) + fabs(r - Aref);
    }
    const int mx[2] = {0, 0};
    block_reduce_store<2>(v, mx, partials, fy_lb, fy_stride);
}

// ------------------------------------------------------------------------------------------------ boundary values as fields; the monitors' face kernel
// Boundary face b of a single-domain block in the read-outs' order: the six sides 2 d + s (x- x+ y- y+ z- z+), each side's faces with the lower remaining axis
// fastest.  side = 2 d + s, r = the face's number on its side; false: b is past the last face
__device__ __forceinline__ bool bface_side(const FvGeo& g, int b, int& side, int& r) {
    const int nyz = g.ny * g.nz, nxz = g.nx * g.nz, nxy = g.nx * g.ny;
    if (b < 2 * nyz) { side = b >= nyz; r = b - side * nyz; return true; }
    b -= 2 * nyz;
    if (b < 2 * nxz) { const int s = b >= nxz; side = 2 + s; r = b - s * nxz; return true; }
    b -= 2 * nxz;
    if (b < 2 * nxy) { const int s = b >= nxy; side = 4 + s; r = b - s * nxy; return true; }
    return false;
}
// T on patch `patch` next to cell c, as k_assemble_scalar takes it: the patch value (fixedValue) or the cell's (zeroGradient).  The six conditions come as device
// arrays (TPatch), not as the by-value ScalarEqn: the six sides' cases below would be merged into one lane-indexed read of the kernel argument, i.e. a stack copy
__device__ __forceinline__ double Tbv(const TPatch& e, const double* T, int c, int patch) { return e.bc[patch] == 1 ? e.val[patch] : T[c]; }
// what face r of side (D, S) carries: its area, the flux out of the domain (the +axis oriented face field negated on a low side) and the boundary values pbv / Ub / Tbv.
// want: bit MF_* of monitors.hpp per component (phi, p, U, T) -- what is not wanted is neither read nor formed.  D and S are template arguments so that every patch
// index into FvGeo's tables is a constant, as in the sweeps' unrolled side loops
struct BFace { double A, phi, p, ux, uy, uz, T; };
template <int D, int S>
__device__ __forceinline__ void bface_values(const FvGeo& g, int r, int want, const double* __restrict__ p, const double* psn_d, const double* __restrict__ U,
                                             const double* __restrict__ T, const TPatch& te, const double* phi_d, BFace& o) {
    CFace3 psn{};
    psn.a[D] = psn_d;
    int i, j, k;
    if (D == 0) { j = r % g.ny; k = r / g.ny; i = S ? g.nx - 1 : 0; }
    else if (D == 1) { i = r % g.nx; k = r / g.nx; j = S ? g.ny - 1 : 0; }
    else { i = r % g.nx; j = r / g.nx; k = S ? g.nz - 1 : 0; }
    const int c = cidx(g, i, j, k), face = cface(g, D, S, i, j, k), patch = 2 * D + S;
    o.A = geo_Af(g, D, i, j, k);
    if (want & (1 << MF_PHI)) o.phi = (S ? 1.0 : -1.0) * phi_d[face];
    if (want & (1 << MF_P)) o.p = pbv(g, p, psn, c, D, S, face);
    if (want & (7 << MF_U)) { double u[3]; Ub(g, U, c, patch, u); o.ux = u[0]; o.uy = u[1]; o.uz = u[2]; }
    if (want & (1 << MF_T)) o.T = Tbv(te, T, c, patch);
}
__device__ __forceinline__ void bface_values_of(const FvGeo& g, int side, int r, int want, const double* __restrict__ p, CFace3 psn, const double* __restrict__ U,
                                                const double* __restrict__ T, const TPatch& te, CFace3 phi, BFace& o) {
    switch (side) {
        case 0: bface_values<0, 0>(g, r, want, p, psn.a[0], U, T, te, phi.a[0], o); break;
        case 1: bface_values<0, 1>(g, r, want, p, psn.a[0], U, T, te, phi.a[0], o); break;
        case 2: bface_values<1, 0>(g, r, want, p, psn.a[1], U, T, te, phi.a[1], o); break;
        case 3: bface_values<1, 1>(g, r, want, p, psn.a[1], U, T, te, phi.a[1], o); break;
        case 4: bface_values<2, 0>(g, r, want, p, psn.a[2], U, T, te, phi.a[2], o); break;
        default: bface_values<2, 1>(g, r, want, p, psn.a[2], U, T, te, phi.a[2], o); break;
    }
}

// "p_boundary", "U_boundary", "T_boundary" (null: not asked for) per boundary face
__global__ __launch_bounds__(256) void k_boundary_values(FvGeo g, const double* __restrict__ p, CFace3 psn, const double* __restrict__ U, const double* __restrict__ T, TPatch te,
                                                         double* __restrict__ pb, double* __restrict__ ub, double* __restrict__ tb) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    int side, r;
    if (!bface_side(g, b, side, r)) return;
    BFace v{};
    bface_values_of(g, side, r, (pb ? 1 << MF_P : 0) | (ub ? 7 << MF_U : 0) | (tb ? 1 << MF_T : 0), p, psn, U, T, te, CFace3{}, v);
    if (pb) pb[b] = v.p;
    if (ub) { ub[3 * (size_t)b] = v.ux; ub[3 * (size_t)b + 1] = v.uy; ub[3 * (size_t)b + 2] = v.uz; }
    if (tb) tb[b] = v.T;
}

// fy::Monitors' face kernel (monitors.hpp): one lane per boundary face, blockIdx.y = the surface object; a face belongs to the object when its side is in the object's
// mask.  Side, owner, face index and area come from FvGeo.  Each wanted component leaves the block as its five partials; the others are skipped (uniform: the table
// is a kernel argument)
__global__ __launch_bounds__(256) void k_monitor_faces(FvGeo g, MonFaceTable t, const double* __restrict__ p, CFace3 psn, const double* __restrict__ U, const double* __restrict__ T,
                                                       TPatch te, CFace3 phi, double* __restrict__ partials) {
    const MonFaceObj o = t.o[blockIdx.y];
    const int b = blockIdx.x * 256 + threadIdx.x;
    int side = 0, r = 0;
    bool in = bface_side(g, b, side, r);
    in = in && ((o.patch >> side) & 1);
    BFace v{};
    if (in) bface_values_of(g, side, r, o.fields | (1 << MF_PHI), p, psn, U, T, te, phi, v);
    const double x[kMonFaceComps] = {1.0, v.phi, v.p, v.ux, v.uy, v.uz, v.T};
    const int slot0 = (int)blockIdx.y * kMonFaceComps * kMonKinds;
#pragma unroll
    for (int q = 0; q < kMonFaceComps; ++q) {
        if (!((o.fields >> q) & 1)) continue;
        double w[kMonKinds];
        mon_terms(in, x[q], v.A, v.phi, w);
        mon_block_reduce_store(w, partials, slot0 + q * kMonKinds, (int)gridDim.x, (int)blockIdx.x);
    }
}

// ------------------------------------------------------------------------------------------------ wall loads (wall_loads.hpp): forces, wallShearStress, yPlus
// coordinate of node q / of the middle of cell q along axis d
__device__ __forceinline__ double wl_node(const FvGeo& g, const WlBlockGeo& w, int d, int q) {
#if FY_FVK_GRADED
    return w.xn[d][q];
#else
    return w.org[d] + q * g.dx;
#endif
}
__device__ __forceinline__ double wl_mid(const FvGeo& g, const WlBlockGeo& w, int d, int q) {
#if FY_FVK_GRADED
    return 0.5 * (w.xn[d][q] + w.xn[d][q + 1]);
#else
    return w.org[d] + (q + 0.5) * g.dx;
#endif
}
// face r of side (D, S) as wl_face_emit wants it: the owner's Gauss-linear gradient of U gathered through the structured neighbours as the stress term forms it
// (u_face_value, grad_row), s = (U_b - U_P) delta with the momentum equation's wall coefficient (geo_rhalf), p_b (pbv), nut_b (nut_boundary), y (geo_ywall), k_P
template <int D, int S>
__device__ __forceinline__ void wl_block_face(const FvGeo& g, const WlBlockGeo& wg, int r, const double* __restrict__ p, const CFace3& psn, const double* __restrict__ U, WlFace& f) {
    int i, j, k;
    if (D == 0) { j = r % g.ny; k = r / g.ny; i = S ? g.nx - 1 : 0; }
    else if (D == 1) { i = r % g.nx; k = r / g.nx; j = S ? g.ny - 1 : 0; }
    else { i = r % g.nx; j = r / g.nx; k = S ? g.nz - 1 : 0; }
    const int ijk[3] = {i, j, k};
    const int c = cidx(g, i, j, k), patch = 2 * D + S;
    f.patch = patch;
    f.A = geo_Af(g, D, i, j, k);
    f.Sf[0] = f.Sf[1] = f.Sf[2] = 0.0;
    f.Sf[D] = S ? f.A : -f.A;
#pragma unroll
    for (int a = 0; a < 3; ++a) f.Cf[a] = a == D ? wl_node(g, wg, a, S ? ndim(g, a) : 0) : wl_mid(g, wg, a, ijk[a]);
    const double uc[3] = {U[3 * (size_t)c], U[3 * (size_t)c + 1], U[3 * (size_t)c + 2]};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        double fv[2][3];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const bool ob = onb(g, d, s, i, j, k);
            const double* un = ob ? nullptr : U + 3 * (size_t)(c + (s ? stride_of(g, d) : -stride_of(g, d)));
            u_face_value(g, d, s, ob, ijk[d], c, uc, un, fv[s]);
        }
        grad_row(g, d, ijk[d], fv, f.G);
    }
    double ub[3];
    Ub(g, U, c, patch, ub);
    const double delta = geo_rhalf(g, D, ijk[D]);
    for (int q = 0; q < 3; ++q) f.s[q] = (ub[q] - uc[q]) * delta;
    f.pb = p ? pbv(g, p, psn, c, D, S, cface(g, D, S, i, j, k)) : 0.0;
    f.nut_b = g.nut ? nut_boundary(g, patch, c) : 0.0;
    f.nu = g.nu;
    f.y = geo_ywall(g, D, c);
    f.wall_fn = g.nut && g.kturb && g.nut_bc[patch] == 2;
    f.kP = f.wall_fn ? g.kturb[c] : 0.0;
    f.cmu25 = g.wf_cmu25;
}
__device__ __forceinline__ void wl_block_face_of(const FvGeo& g, const WlBlockGeo& wg, int side, int r, const double* __restrict__ p, const CFace3& psn, const double* __restrict__ U, WlFace& f) {
    switch (side) {
        case 0: wl_block_face<0, 0>(g, wg, r, p, psn, U, f); break;
        case 1: wl_block_face<0, 1>(g, wg, r, p, psn, U, f); break;
        case 2: wl_block_face<1, 0>(g, wg, r, p, psn, U, f); break;
        case 3: wl_block_face<1, 1>(g, wg, r, p, psn, U, f); break;
        case 4: wl_block_face<2, 0>(g, wg, r, p, psn, U, f); break;
        default: wl_block_face<2, 1>(g, wg, r, p, psn, U, f); break;
    }
}
// fy::WallLoads' face kernel: one lane per boundary face (the read-outs' order), blockIdx.y = the object; an object that is not due this step leaves at once
__global__ __launch_bounds__(256) void k_wall_loads(FvGeo g, WlTable t, WlBlockGeo wg, const double* __restrict__ p, CFace3 psn, const double* __restrict__ U,
                                                    double* __restrict__ wss, double* __restrict__ yplus, double* __restrict__ partials) {
    if (!((t.due >> blockIdx.y) & 1u)) return;
    const int b = blockIdx.x * 256 + threadIdx.x;
    int side = 0, r = 0;
    const bool have = bface_side(g, b, side, r);
    const WlObj& o = t.o[blockIdx.y];
    WlFace f{};
    f.patch = have ? side : -1;
    bool member = false;
    for (int q = 0; q < o.np; ++q) member = member || o.patch[q] == f.patch;
    if (have && member) wl_block_face_of(g, wg, side, r, p, psn, U, f);      // (a face outside the object's set is not gathered: wl_face_emit stores its zeros)
    wl_face_emit(o, have, f, b, wss, yplus, partials, (int)blockIdx.y * kWlComps * kMonKinds);
}
// "nut_boundary" and "nearWallDist" per boundary face
__global__ __launch_bounds__(256) void k_wall_readouts(FvGeo g, double* __restrict__ nutb, double* __restrict__ yw) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    int side, r;
    if (!bface_side(g, b, side, r)) return;
    const int D = side >> 1, S = side & 1;
    int i, j, k;
    if (D == 0) { j = r % g.ny; k = r / g.ny; i = S ? g.nx - 1 : 0; }
    else if (D == 1) { i = r % g.nx; k = r / g.nx; j = S ? g.ny - 1 : 0; }
    else { i = r % g.nx; j = r / g.nx; k = S ? g.nz - 1 : 0; }
    const int c = cidx(g, i, j, k);
    if (nutb) nutb[b] = g.nut ? nut_boundary(g, side, c) : 0.0;
    if (yw) yw[b] = geo_ywall(g, D, c);
}

// launch grids of the cell sweeps: the whole owned range, or the block window the geometry names (FvGeo::win_nblk: a range of z-planes, for the
// sweeps that run beside a halo exchange)
inline int fv_grid(const FvGeo& g) { return g.win_nblk > 0 ? g.win_nblk : div_up(g.Nc, 256); }
inline int fv_red_grid(const FvGeo& g) { return g.win_nblk > 0 ? g.win_nblk : red_blocks(g.Nc); }

}  // namespace

int launch_flux_of(hipStream_t s, FvGeo g, const double* F, Face3 out) {
    hipLaunchKernelGGL(k_flux_of<0>, dim3(div_up(fv_fsize(g, 0), 256)), dim3(256), 0, s, g, F, out.a[0]);
    hipLaunchKernelGGL(k_flux_of<1>, dim3(div_up(fv_fsize(g, 1), 256)), dim3(256), 0, s, g, F, out.a[1]);
    hipLaunchKernelGGL(k_flux_of<2>, dim3(div_up(fv_fsize(g, 2), 256)), dim3(256), 0, s, g, F, out.a[2]);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_courant(hipStream_t s, FvGeo g, CFace3 phi, double* partials) {
    hipLaunchKernelGGL(k_courant, dim3(fv_red_grid(g)), dim3(256), 0, s, g, phi, partials);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_pre_coupling(hipStream_t s, FvGeo g, const double* U, const double* p, const double* alpha, CFace3 psn, double* vGrad,
                        double* gradP, double* divT, double* Gout, int write_vgrad, int write_pfields, CFace3 phi, double* ddtU, double* Uold_out,
                        double* cellrec, double rec_nu, double rec_rhoF, Face3 dcorr) {
    hipLaunchKernelGGL(k_pre_coupling, dim3(fv_grid(g)), dim3(256), 0, s, g, U, p, alpha, psn, vGrad, gradP, divT, Gout, write_vgrad, write_pfields,
                       phi, ddtU, Uold_out, cellrec, 2.0 * rec_nu, rec_rhoF, dcorr);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_interp_alpha(hipStream_t s, FvGeo g, const double* alpha, Face3 af) {
    hipLaunchKernelGGL(k_interp_alpha_cells, dim3(fv_grid(g)), dim3(256), 0, s, g, alpha, af);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_div_G(hipStream_t s, FvGeo g, const double* G, double* divG) {
    hipLaunchKernelGGL(k_div_G, dim3(fv_grid(g)), dim3(256), 0, s, g, G, divG);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_stress_div(hipStream_t s, FvGeo g, const double* U, const double* alpha, double* divG) {
    if (g.gz != 0 || g.c0 != 0 || g.win_nblk > 0) return fail(FY_ERR_INVALID, "launch_stress_div: single domain only (a slab exchanges row z of G between the two sweeps)");
    const int ntx = (int)div_up(g.nx, kSTX), nty = (int)div_up(g.ny, kSTY), ntz = (int)div_up(g.nz, kSTZ);
    hipLaunchKernelGGL(k_stress_div, dim3((unsigned)(ntx * nty * ntz)), dim3(kStressThreads), 0, s, g, U, alpha, divG, ntx, nty);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_assemble_turb(hipStream_t s, FvGeo g, TurbEqn e, const double* k, const double* eps, const double* alpha, CFace3 alphaf, CFace3 phi,
                         const double* vGrad, const double* U, Mom7 M, double* b3, double* x3) {
    hipLaunchKernelGGL(k_assemble_turb, dim3(fv_grid(g)), dim3(256), 0, s, g, e, k, eps, alpha, alphaf, phi, vGrad, U, M, b3, x3);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_turb_finish(hipStream_t s, FvGeo g, TurbEqn e, const double* x3, double* X, int nut_mode, double cmu, const double* eps, double* nut) {
    hipLaunchKernelGGL(k_turb_finish, dim3(fv_grid(g)), dim3(256), 0, s, g, e, x3, X, nut_mode, cmu, eps, nut);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_assemble_scalar(hipStream_t s, FvGeo g, ScalarEqn e, const double* T, const double* alpha, CFace3 phi, const double* Sp, const double* Su, Mom7 M,
                           double* b3, double* x3) {
    hipLaunchKernelGGL(k_assemble_scalar, dim3(fv_grid(g)), dim3(256), 0, s, g, e, T, alpha, phi, Sp, Su, M, b3, x3);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_scalar_finish(hipStream_t s, FvGeo g, const double* x3, double* X) {
    hipLaunchKernelGGL(k_scalar_finish, dim3(fv_grid(g)), dim3(256), 0, s, g, x3, X);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_smagorinsky_nut(hipStream_t s, FvGeo g, const double* vGrad, double ck, double ce, double delta, double* nut) {
    hipLaunchKernelGGL(k_smagorinsky_nut, dim3(fv_grid(g)), dim3(256), 0, s, g, vGrad, ck, ce, delta, nut);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_assemble_momentum(hipStream_t s, FvGeo g, const double* U, const double* Uold, const double* alpha, const double* alphaOld,
                             CFace3 alphaf, CFace3 phi, const double* uSource, const double* uSourceDrag, const double* divG, const double* vGrad,
                             Mom7 M, double* src, double* rAU, const PorousDev* por) {
    if (g.upwind >= 3) hipLaunchKernelGGL(k_assemble_momentum<true>, dim3(fv_grid(g)), dim3(256), 0, s, g, U, Uold, alpha, alphaOld, alphaf, phi, uSource,
                                          uSourceDrag, divG, vGrad, M, src, rAU, por);
    else hipLaunchKernelGGL(k_assemble_momentum<false>, dim3(fv_grid(g)), dim3(256), 0, s, g, U, Uold, alpha, alphaOld, alphaf, phi, uSource,
                            uSourceDrag, divG, vGrad, M, src, rAU, por);
    FY_LAUNCH_CHECK();
    return FY_OK;
}
int launch_grad_magsqr(hipStream_t s, FvGeo g, const double* U, double* gradL) {
    hipLaunchKernelGGL(k_grad_magsqr, dim3(fv_grid(g)), dim3(256), 0, s, g, U, gradL);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_interp_rAU(hipStream_t s, FvGeo g, const double* rAU, Face3 rf) {
    hipLaunchKernelGGL(k_interp_rAU<0>, dim3(div_up(fv_fsize(g, 0), 256)), dim3(256), 0, s, g, rAU, rf.a[0]);
    hipLaunchKernelGGL(k_interp_rAU<1>, dim3(div_up(fv_fsize(g, 1), 256)), dim3(256), 0, s, g, rAU, rf.a[1]);
    hipLaunchKernelGGL(k_interp_rAU<2>, dim3(div_up(fv_fsize(g, 2), 256)), dim3(256), 0, s, g, rAU, rf.a[2]);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_bmom(hipStream_t s, FvGeo g, const double* src, const double* p, CFace3 psn, CFace3 phiForces, CFace3 rAUf, double* bmom) {
    hipLaunchKernelGGL(k_bmom, dim3(fv_grid(g)), dim3(256), 0, s, g, src, p, psn, phiForces, rAUf, bmom);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_bmom_faces(hipStream_t s, FvGeo g, const double* rAU, const double* uSource, const double* src, const double* p, CFace3 psn, Face3 rAUf_out,
                      Face3 phiForces, double* bmom) {
    hipLaunchKernelGGL(k_bmom_faces, dim3(fv_grid(g)), dim3(256), 0, s, g, rAU, uSource, src, p, psn, rAUf_out, phiForces, bmom);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_mom_pass(hipStream_t s, FvGeo g, Mom7 M, const double* b, const double* x, double* xn, const double* xsum, double n_glob, double* partials,
                    const double* hsrc, const double* rAU, double* HbyA) {
    if (HbyA) hipLaunchKernelGGL(k_mom_pass<true>, dim3(fv_red_grid(g)), dim3(256), 0, s, g, M, b, x, xn, xsum, n_glob, partials, hsrc, rAU, HbyA);
    else hipLaunchKernelGGL(k_mom_pass<false>, dim3(fv_red_grid(g)), dim3(256), 0, s, g, M, b, x, xn, xsum, n_glob, partials, hsrc, rAU, HbyA);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_HbyA(hipStream_t s, FvGeo g, Mom7 M, const double* src, const double* U, const double* rAU, double* HbyA) {
    hipLaunchKernelGGL(k_HbyA, dim3(fv_grid(g)), dim3(256), 0, s, g, M, src, U, rAU, HbyA);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_phiHbyA(hipStream_t s, FvGeo g, const double* HbyA, const double* U, const double* Uold, CFace3 phiOld, CFace3 rAUf,
                   CFace3 alphaf, CFace3 phiForces, Face3 out, Face3 psn, Face3 ddtc, int keep) {
    if (keep == 1) hipLaunchKernelGGL(k_phiHbyA_cells<1>, dim3(fv_grid(g)), dim3(256), 0, s, g, HbyA, U, Uold, phiOld, rAUf, alphaf, phiForces, out, psn, ddtc);
    else if (keep == 2) hipLaunchKernelGGL(k_phiHbyA_cells<2>, dim3(fv_grid(g)), dim3(256), 0, s, g, HbyA, U, Uold, phiOld, rAUf, alphaf, phiForces, out, psn, ddtc);
    else hipLaunchKernelGGL(k_phiHbyA_cells<0>, dim3(fv_grid(g)), dim3(256), 0, s, g, HbyA, U, Uold, phiOld, rAUf, alphaf, phiForces, out, psn, ddtc);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_adjust_phi_sums(hipStream_t s, FvGeo g, CFace3 phiHbyA, CFace3 phiForces, double* partials) {
    hipLaunchKernelGGL(k_adjust_phi_sums, dim3(fv_red_grid(g)), dim3(256), 0, s, g, phiHbyA, phiForces, partials);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_adjust_phi_apply(hipStream_t s, FvGeo g, const double* sums, Face3 phiHbyA, CFace3 phiForces, CFace3 rAUf, const double* U, Face3 psn, int* err) {
    const size_t nbf = 2 * ((size_t)g.ny * g.nz + (size_t)g.nx * g.nz + (size_t)g.nx * g.ny);
    hipLaunchKernelGGL(k_adjust_phi_apply, dim3(div_up(nbf, 256)), dim3(256), 0, s, g, sums, phiHbyA, phiForces, rAUf, U, psn, err);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_rAUf_phi_forces(hipStream_t s, FvGeo g, const double* rAU, const double* uSource, Face3 rf, Face3 out) {
    hipLaunchKernelGGL(k_rAUf_phi_forces_cells, dim3(fv_grid(g)), dim3(256), 0, s, g, rAU, uSource, rf, out);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_assemble_pressure(hipStream_t s, FvGeo g, CFace3 phiHbyA, CFace3 rAUf, CFace3 alphaf, CFace3 psn, const double* alpha,
                             const double* alphaOld, PMat A, double* rhs, bool matrix) {
    if (matrix) hipLaunchKernelGGL(k_assemble_pressure<true>, dim3(fv_grid(g)), dim3(256), 0, s, g, phiHbyA, rAUf, alphaf, psn, alpha, alphaOld, A, rhs);
    else hipLaunchKernelGGL(k_assemble_pressure<false>, dim3(fv_grid(g)), dim3(256), 0, s, g, phiHbyA, rAUf, alphaf, psn, alpha, alphaOld, A, rhs);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_flux_correct(hipStream_t s, FvGeo g, const double* p, CFace3 phiHbyA, CFace3 rAUf, CFace3 alphaf, CFace3 psn, CFace3 phiForces, Face3 pflux, Face3 phi) {
    hipLaunchKernelGGL(k_flux_correct_cells, dim3(fv_grid(g)), dim3(256), 0, s, g, p, phiHbyA, rAUf, alphaf, psn, phiForces, pflux, phi);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_cont_err(hipStream_t s, FvGeo g, CFace3 phi, CFace3 alphaf, const double* alpha, const double* alphaOld, double* partials) {
    hipLaunchKernelGGL(k_cont_err, dim3(fv_red_grid(g)), dim3(256), 0, s, g, phi, alphaf, alpha, alphaOld, partials);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_U_correct(hipStream_t s, FvGeo g, const double* HbyA, const double* rAU, const double* p, CFace3 psn, CFace3 phiForces,
                     CFace3 pflux, CFace3 alphaf, CFace3 rAUf, double* U) {
    hipLaunchKernelGGL(k_U_correct<false>, dim3(fv_red_grid(g)), dim3(256), 0, s, g, HbyA, rAU, p, psn, phiForces, pflux, alphaf, rAUf, U, CFace3{}, nullptr, nullptr, nullptr);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_U_correct_diag(hipStream_t s, FvGeo g, const double* HbyA, const double* rAU, const double* p, CFace3 psn, CFace3 phiForces,
                          CFace3 pflux, CFace3 alphaf, CFace3 rAUf, double* U, CFace3 phi, const double* alpha, const double* alphaOld, double* partials) {
    hipLaunchKernelGGL(k_U_correct<true>, dim3(fv_red_grid(g)), dim3(256), 0, s, g, HbyA, rAU, p, psn, phiForces, pflux, alphaf, rAUf, U, phi, alpha, alphaOld, partials);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_corr_back(hipStream_t s, FvGeo g, const double* p, CFace3 phiHbyA, CFace3 rAUf, CFace3 alphaf, CFace3 psn, CFace3 phiForces, Face3 phi,
                     const double* HbyA, const double* rAU, double* U, const double* alpha, const double* alphaOld, double* partials, bool faces_from_cells) {
    const FaceSrc rs{rAUf, faces_from_cells ? rAU : nullptr}, as{alphaf, faces_from_cells ? alpha : nullptr};
    const dim3 grid(fv_red_grid(g)), blk(256);
#define FY_BACK(DG, FC) hipLaunchKernelGGL((k_corr_back<DG, FC>), grid, blk, 0, s, g, p, phiHbyA, rs, as, psn, phiForces, phi, HbyA, rAU, U, alpha, alphaOld, partials)
    if (partials) { if (faces_from_cells) FY_BACK(true, true); else FY_BACK(true, false); }
    else { if (faces_from_cells) FY_BACK(false, true); else FY_BACK(false, false); }
#undef FY_BACK
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_corr_front(hipStream_t s, FvGeo g, const double* HbyA, const double* U, CFace3 dcorr, CFace3 rAUf, CFace3 alphaf, CFace3 phiForces, Face3 phiHbyA,
                      Face3 psn, const double* rAU, const double* alpha, const double* alphaOld, PMat A, double* rhs, bool store_A, const double* x,
                      const double* xsum_dev, double xsum_val, double inv_n, double* res, double* partials, bool faces_from_cells) {
    const FaceSrc rs{rAUf, faces_from_cells ? rAU : nullptr}, as{alphaf, faces_from_cells ? alpha : nullptr};
    const dim3 grid(fv_red_grid(g)), blk(256);
#define FY_FRONT(SA, FC) hipLaunchKernelGGL((k_corr_front<SA, FC>), grid, blk, 0, s, g, HbyA, U, dcorr, rs, as, phiForces, phiHbyA, psn, rAU, alpha, alphaOld, A, rhs, \
                                            x, xsum_dev, xsum_val, inv_n, res, partials)
    if (store_A) { if (faces_from_cells) FY_FRONT(true, true); else FY_FRONT(true, false); }
    else { if (faces_from_cells) FY_FRONT(false, true); else FY_FRONT(false, false); }
#undef FY_FRONT
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_p_ghost_uz(hipStream_t s, FvGeo g, CFace3 rAUf, CFace3 alphaf, PMat A) {
    hipLaunchKernelGGL(k_p_ghost_uz, dim3(div_up((size_t)g.nx * g.ny, 256)), dim3(256), 0, s, g, rAUf, alphaf, A);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_boundary_values(hipStream_t s, FvGeo g, const double* p, CFace3 psn, const double* U, const double* T, TPatch te, double* pb, double* ub, double* tb) {
    const size_t nb = 2 * ((size_t)g.ny * g.nz + (size_t)g.nx * g.nz + (size_t)g.nx * g.ny);
    hipLaunchKernelGGL(k_boundary_values, dim3(div_up(nb, 256)), dim3(256), 0, s, g, p, psn, U, T, te, pb, ub, tb);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_monitor_faces(hipStream_t s, FvGeo g, MonFaceTable t, const double* p, CFace3 psn, const double* U, const double* T, TPatch te, CFace3 phi, double* partials, int nblk) {
    if (t.n <= 0) return FY_OK;
    hipLaunchKernelGGL(k_monitor_faces, dim3(nblk, t.n), dim3(256), 0, s, g, t, p, psn, U, T, te, phi, partials);
    FY_LAUNCH_CHECK();
    return FY_OK;
}
int launch_wall_loads(hipStream_t s, FvGeo g, WlTable t, WlBlockGeo wg, const double* p, CFace3 psn, const double* U, double* wss, double* yplus, double* partials, int nblk) {
    if (t.n <= 0) return FY_OK;
    hipLaunchKernelGGL(k_wall_loads, dim3(nblk, t.n), dim3(256), 0, s, g, t, wg, p, psn, U, wss, yplus, partials);
    FY_LAUNCH_CHECK();
    return FY_OK;
}
int launch_wall_readouts(hipStream_t s, FvGeo g, double* nutb, double* yw) {
    const int nb = 2 * (g.ny * g.nz + g.nx * g.nz + g.nx * g.ny);
    hipLaunchKernelGGL(k_wall_readouts, dim3(div_up(nb, 256)), dim3(256), 0, s, g, nutb, yw);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

#if FY_FVK_GRADED
}  // namespace gr
#endif
}  // namespace fy
