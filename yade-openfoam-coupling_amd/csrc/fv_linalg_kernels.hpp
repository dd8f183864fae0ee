// Launchers of fv_linalg_kernels.hip: the pressure solver's building blocks, the geometric multigrid and the plain vector kernels.  None takes
// an FvGeo: they exist once, in namespace fy, for the uniform block, the graded block and (PCG update, fold, copy) the general-mesh solver.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace fy {

// symmetric 7-point pressure matrix of one multigrid level: (A x)_c = diag_c x_c - sum u_f x_nb, u_* stored at the owner (low) cell
struct PMat {
    int nx, ny, nz, N;      // owned extent of this level
    int c0, ntot;           // storage index of the first owned cell, storage size (owned + ghost planes)
    double *diag, *ux, *uy, *uz;
};

// reducing kernels emit one partial per 256-cell block; the count is rounded up to a multiple of 8 for the XCD-aware block order
inline int red_blocks(int n) { return (((n + 255) / 256) + 7) & ~7; }

constexpr int kMgDirectMax = 128, kMgDirectBand = 64;
constexpr int kMgTailMax = 6;
constexpr int kMgTailCells = 1024;   // measured: at 8000 cells one workgroup (137 us) is SLOWER than the ~20 separate launches it replaces
struct MgWeights { int n; double w[4]; };      // the smoother's Jacobi weights per sweep (pre-smoothing order; post-smoothing runs them backwards)

// ---- reductions: kernels over n cells write per-block partials to scratch[slot*red_blocks(n) + block]; finalize folds them in fixed order
// flag/seq (mapped host memory, optional): flag[slot] = seq is stored, system scope, after out[slot] -- the host may spin on it
int launch_reduce_finalize(hipStream_t s, const double* partials, int n_cells, int nslots, const int* ops /*0 sum,1 max (device)*/, double* out,
                           unsigned long long* flag = nullptr, unsigned long long seq = 0);
int launch_sum3(hipStream_t s, const double* x, int n, double* partials);                                  // slots 0..2 = component sums

// ---- pressure solver building blocks
int launch_p_apply(hipStream_t s, PMat A, const double* x, double* y);                                     // y = A x (the roofline kernel)
int launch_p_apply_dot(hipStream_t s, PMat A, const double* x, const double* r /* or nullptr */, double* y, double* partials);   // y = A x; slot 1 = x.y; with r also slot 0 = x.r
// r = b - A x; slots 0 |r|, 1 norm factor; xbar = xsum_dev[0] * inv_n stays on the device (it is an all-reduced sum)
int launch_p_init(hipStream_t s, PMat A, const double* b, const double* x, const double* xsum_dev /* sum(x) on the device, or nullptr: */, double xsum_val, double inv_n,
                  double* r, double* partials);
int launch_dot(hipStream_t s, int n, int c0, const double* a, const double* b /* nullptr: sum(a) */, double* partials);   // slot 0, over [c0, c0+n)
// single-reduction PCG update (k_pcg_cg_update): sc[0] = u.r, sc[1] = u.w; it == 0: x += alpha u, r -= alpha w only (p = u, s = w: the caller swaps buffers)
int launch_pcg_cg_update(hipStream_t s, int n, int c0, const double* u, const double* w, double* p, double* sv, double* x, double* r, double* sc, int it, double* partials);
int launch_jacobi_precond(hipStream_t s, PMat A, const double* r, double* z);
// ref_term != nullptr: the coarse cell ref_c (local index of C, -1: not in C) holds the pressure reference cell and keeps its point term unscaled
// (see k_mg_coarsen); launch_mg_ref_term leaves that term (level 0's, 0 where ref_local < 0) in out[0]
int launch_mg_coarsen(hipStream_t s, PMat F, PMat C, int ref_c = -1, const double* ref_term = nullptr);
int launch_mg_ref_term(hipStream_t s, PMat A0, int ref_local, double* out);
int launch_mg_smooth_first(hipStream_t s, PMat A, const double* b, double* x, double w);                   // x = w b / diag
int launch_mg_smooth_two_from_zero(hipStream_t s, PMat A, const double* b, double* xn, double w, double w2);      // smooth_first(w) + smooth(w2) fused (bit-identical)
int launch_mg_smooth(hipStream_t s, PMat A, const double* b, const double* x, double* xn, double w);
// the same sweep + the block partials of xn . b (slot 0), what launch_dot(xn, b) would leave there
int launch_mg_smooth_dot(hipStream_t s, PMat A, const double* b, const double* x, double* xn, double w, double* partials);      // xn = x + w (b - A x)/diag
int launch_mg_residual_restrict(hipStream_t s, PMat A, const double* b, const double* x, PMat C, double* bc);   // bc = P^T (b - A x)
int launch_mg_prolong_add(hipStream_t s, PMat A, double* x, PMat C, const double* xc);
int launch_mg_prolong_add_planes(hipStream_t s, PMat A /* a range of planes */, int kofs /* its first plane relative to the first owned one */, double* x, PMat C, const double* xc);
int launch_mg_smooth_prolong(hipStream_t s, PMat A, const double* b, const double* x, PMat C, const double* xc, double* xn, double w);   // x += P xc, then one sweep (fused)
// the coarsest level: x = A^-1 b from the banded Cholesky factor `fac` (launch_mg_coarse_factor: mg_coarse_factor_doubles(A) doubles; for
// levels with mg_coarse_direct_ok(A): no ghost planes, <= kMgDirectMax cells, band <= kMgDirectBand); fac == nullptr or a failed
// factorisation: `sweeps` damped-Jacobi sweeps from a zero guess
bool mg_coarse_direct_ok(PMat A);
int mg_coarse_factor_doubles(PMat A);
int launch_mg_coarse_factor(hipStream_t s, PMat A, double* fac);
int launch_mg_coarse_solve(hipStream_t s, PMat A, const double* b, double* x, double* tmp, int sweeps, double w, const double* fac = nullptr);
// the whole V-cycle below a size threshold in one workgroup; level l result: x1[l] (x0 for the coarsest / a single-level tail)
int launch_mg_tail(hipStream_t s, const PMat* A, double* const* x0, double* const* x1, double* const* b, int n, double w, int coarse_sweeps, MgWeights W,
                   const double* fac = nullptr);

int launch_copy_f64(hipStream_t s, double* dst, const double* src, size_t n);
int launch_relax_field(hipStream_t s, double* x, const double* prev, double alpha, size_t n);   // x = prev + alpha (x - prev)
// the ghost plane's z-face coefficients of a coarse level, from the fine level's (slab interfaces; level 0's: launch_p_ghost_uz)
int launch_mg_coarsen_ghost(hipStream_t s, PMat F, PMat C);
// y += x on a contiguous range (reverse-halo accumulation)
int launch_add_f64(hipStream_t s, double* y, const double* x, size_t n);
// Boussinesq buoyancy: a[3 n] = (-beta (T - T_ref)) g per cell, sum[3 n] = uSource + a (g: three host doubles)
int launch_buoyancy(hipStream_t s, size_t n_cells, const double* T, double beta, double T_ref, const double* g, const double* uSource, double* a, double* sum);

}  // namespace fy
