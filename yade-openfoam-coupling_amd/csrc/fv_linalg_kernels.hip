// The geometry-free half of the structured solver's kernels: the pressure solver's building blocks on a 7-point PMat (matrix apply, the
// single-reduction PCG update, the Jacobi preconditioner), the whole geometric multigrid (coarsening, smoothers, transfer, the one-workgroup
// tail, the banded Cholesky of the coarsest level, the two-cells-per-thread variants) and the plain vector kernels (fold of block partials,
// component sums, copy, add, relax).  Nothing here reads an FvGeo, so unlike fv_kernels.hip this source is compiled ONCE, into namespace fy:
// the uniform and the graded block (fy::gr sweeps) run the same pressure solver, and the general-mesh solver (ldu_*.hip / ldu_solver.cpp)
// shares the PCG update, the fold and the copy.  FP64, no MFMA: every kernel is bandwidth or latency bound.
#include "fv_linalg_kernels.hpp"

#include "device_util.hpp"

namespace fy {
namespace {

// fold the per-block partials of one slot per workgroup, in a fixed order: 1024 threads stride over the partials (16 000 of them at
// 160^3), then a shuffle + LDS tree.  (256 threads took 17 us per call x 23 calls per step.)
// flag != nullptr (out and flag in mapped host memory): the result is followed by a system-scope fence and flag[slot] = seq, which is
// what the host spins on instead of waiting for the stream to drain (a stream synchronisation costs ~15 us of idle GPU per read-back).
__global__ __launch_bounds__(1024) void k_reduce_finalize(const double* __restrict__ partials, int nblocks, const int* __restrict__ ops,
                                                          double* __restrict__ out, unsigned long long* flag, unsigned long long seq) {
    __shared__ double sh[16];
    const int slot = blockIdx.x;
    const int mx = ops ? ops[slot] : 0;
    double x = mx ? -1e300 : 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 1024) {
        const double y = partials[(size_t)slot * nblocks + b];
        x = mx ? fmax(x, y) : x + y;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double y = __shfl_down(x, o, 64);
        x = mx ? fmax(x, y) : x + y;
    }
    if (lane == 0) sh[wv] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = sh[0];
        for (int w = 1; w < 16; ++w) r = mx ? fmax(r, sh[w]) : r + sh[w];
        out[slot] = r;
        if (flag) {
            __threadfence_system();
            __hip_atomic_store(&flag[slot], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// component sums over a contiguous range of n vectors starting at x
__global__ __launch_bounds__(256) void k_sum3(const double* __restrict__ x, int n, double* __restrict__ partials) {
    double v[3] = {0, 0, 0};
    FY_RED_LOOP(c, n)
        for (int q = 0; q < 3; ++q) v[q] += x[3 * (size_t)c + q];
    const int mx[3] = {0, 0, 0};
    block_reduce_store<3>(v, mx, partials);
}

// ------------------------------------------------------------------------------------------------ pressure solver
// y = A x.  The pEqn Laplacian apply: 48 algorithmic bytes per cell (diag 8 + ux,uy,uz 24 + x 8 + y 8); the low-side
// coefficients ux[c-1], uy[c-nx], uz[c-nx*ny] and the six neighbour x values are re-reads served by L1/L2.
// High-side boundary faces store 0, so the wrapped low-side reads (e.g. ux[c-1] at i = 0) multiply by 0 and only the
// array ends need an index guard.  c is a STORAGE index; with ghost planes the z-neighbours always exist (their coefficient
// is 0 on a physical boundary, the interface coefficient otherwise) and the ghost x values come from the halo exchange.
__device__ __forceinline__ double p_row(const PMat& A, const double* __restrict__ x, int c) {
    // Guarded terms are loaded from clamped (always valid) addresses and SELECTED: written as `if (c >= 1) a -= ...` every guard
    // becomes a divergent branch with its loads inside, i.e. seven dependent memory round trips per row instead of one.
    const int sy = A.nx, sz = A.nx * A.ny, last = A.ntot - 1;
    const int xm = max(c - 1, 0), xp = min(c + 1, last), ym = max(c - sy, 0), yp = min(c + sy, last), zm = max(c - sz, 0), zp = min(c + sz, last);
    const double uxc = A.ux[c], uyc = A.uy[c], uzc = A.uz[c];
    const double t0 = A.ux[xm] * x[xm], t1 = uxc * x[xp], t2 = A.uy[ym] * x[ym], t3 = uyc * x[yp], t4 = A.uz[zm] * x[zm], t5 = uzc * x[zp];
    double a = A.diag[c] * x[c];
    a = (c >= 1) ? a - t0 : a;
    a = (c + 1 < A.ntot) ? a - t1 : a;
    a = (c >= sy) ? a - t2 : a;
    a = (c + sy < A.ntot) ? a - t3 : a;
    a = (c >= sz) ? a - t4 : a;
    a = (c + sz < A.ntot) ? a - t5 : a;
    return a;
}
__device__ __forceinline__ double p_rowsum(const PMat& A, int c) {
    const int sy = A.nx, sz = A.nx * A.ny;
    double rs = A.diag[c];
    if (c >= 1) rs -= A.ux[c - 1];
    if (c + 1 < A.ntot) rs -= A.ux[c];
    if (c >= sy) rs -= A.uy[c - sy];
    if (c + sy < A.ntot) rs -= A.uy[c];
    if (c >= sz) rs -= A.uz[c - sz];
    if (c + sz < A.ntot) rs -= A.uz[c];
    return rs;
}

__global__ __launch_bounds__(256) void k_p_apply(PMat A, const double* __restrict__ x, double* __restrict__ y) {
    const int t = swz_block(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
    if (t >= A.N) return;
    const int c = t + A.c0;
    y[c] = p_row(A, x, c);
}

// w = A u inside the single-reduction PCG (fv_pressure.cpp): slot 1 = u.w (delta); WITH_R: also slot 0 = u.r (gamma) -- on a single domain
// the V-cycle's last sweep has left gamma's partials in slot 0 already (k_mg_smooth_dot: same blocks, same order) and only delta is formed here
template <bool WITH_R>
__global__ __launch_bounds__(256) void k_p_apply_dot(PMat A, const double* __restrict__ x, const double* __restrict__ r, double* __restrict__ y, double* __restrict__ partials) {
    double v[2] = {0, 0};
    FY_RED_LOOP(t, A.N) {
        const int c = t + A.c0;
        const double a = p_row(A, x, c);
        y[c] = a;
        const double xc = x[c];
        if (WITH_R) v[0] += xc * r[c];
        v[1] += a * xc;
    }
    if (WITH_R) {
        const int mx[2] = {0, 0};
        block_reduce_store<2>(v, mx, partials);
    } else {
        double v1[1] = {v[1]};
        const int mx[1] = {0};
        block_reduce_store<1>(v1, mx, partials + gridDim.x);
    }
}

// r = b - A x ; slot 0 = sum|r| ; slot 1 = sum(|A x - A xbar| + |b - A xbar|)   (lduMatrix::solver::normFactor)
__global__ __launch_bounds__(256) void k_p_init(PMat A, const double* __restrict__ b, const double* __restrict__ x, const double* __restrict__ xbar_dev,
                                                double xsum_val, double inv_n, double* __restrict__ r, double* __restrict__ partials) {
    double v[2] = {0, 0};
    const double xbar = (xbar_dev ? xbar_dev[0] : xsum_val) * inv_n;      // sum(x) from the device, or the value the last update of x left with the host
    FY_RED_LOOP(t, A.N) {
        const int c = t + A.c0;
        const double Ax = p_row(A, x, c);
        const double Aref = p_rowsum(A, c) * xbar;
        const double rr = b[c] - Ax;
        r[c] = rr;
        v[0] += fabs(rr);
        v[1] += fabs(Ax - Aref) + fabs(b[c] - Aref);
    }
    const int mx[2] = {0, 0};
    block_reduce_store<2>(v, mx, partials);
}

// dot product / plain sum over the owned range [c0, c0 + n) of arrays given by their storage base
__global__ __launch_bounds__(256) void k_dot(int n, int c0, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ partials) {
    double v[1] = {0};
    FY_RED_LOOP(t, n) v[0] += a[t + c0] * (b ? b[t + c0] : 1.0);
    const int mx[1] = {0};
    block_reduce_store<1>(v, mx, partials);
}

// The vector update of the single-reduction (Chronopoulos-Gear) form of PCG.C's loop [OF-6]: with u = M^-1 r, w = A u and the ONE reduction
// gamma = u.r, delta = u.w per iteration,
//     beta = gamma / gamma_old,  alpha = gamma / (delta - beta gamma / alpha_old)      (beta = 0, alpha = gamma / delta in the first iteration)
//     p = u + beta p,  s = w + beta s  (= A p),  x += alpha p,  r -= alpha s
// -- the iterates of the textbook loop in exact arithmetic, with the search direction's image s carried by recurrence instead of a second dot
// product + all-reduce after the matrix-vector product.  sc[0] = gamma, sc[1] = delta (this iteration's fold); {gamma_old, alpha_old} live in
// sc[2 + 2 q], sc[3 + 2 q] with q = it & 1: an iteration reads set q and leaves set 1 - q, so no block reads what another one has rewritten.
// slot 0 = sum|r|, slot 1 = sum(x): the next solve's xbar (normFactor) -- k_dot's partition and order, so k_dot's bits, without k_dot's pass.
// FIRST: p = u and s = w need no pass of their own -- the host lets the two pairs of buffers trade places afterwards (fv_pressure.cpp)
template <bool FIRST>
__global__ __launch_bounds__(256) void k_pcg_cg_update(int n, int c0, const double* __restrict__ u, const double* __restrict__ w, double* __restrict__ p,
                                                       double* __restrict__ sv, double* __restrict__ x, double* __restrict__ r, double* __restrict__ sc, int it,
                                                       double* __restrict__ partials) {
    double v[2] = {0, 0};
    const double gamma = sc[0], delta = sc[1];
    double beta = 0.0, al = gamma / delta;
    if (!FIRST) {
        const double gold = sc[2 + 2 * (it & 1)], aold = sc[3 + 2 * (it & 1)];
        beta = gamma / gold;
        al = gamma / (delta - beta * gamma / aold);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { sc[2 + 2 * ((it + 1) & 1)] = gamma; sc[3 + 2 * ((it + 1) & 1)] = al; }
    FY_RED_LOOP(t, n) {
        const int c = t + c0;
        double pn = u[c], sn = w[c];
        if (!FIRST) {
            pn = pn + beta * p[c]; sn = sn + beta * sv[c];
            p[c] = pn; sv[c] = sn;
        }
        const double xn = x[c] + al * pn;
        x[c] = xn;
        const double rr = r[c] - al * sn;
        r[c] = rr;
        v[0] += fabs(rr);
        v[1] += xn;
    }
    const int mx[2] = {0, 0};
    block_reduce_store<2>(v, mx, partials);
}

__global__ __launch_bounds__(256) void k_jacobi_precond(PMat A, const double* __restrict__ r, double* __restrict__ z) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < A.N) { const int c = t + A.c0; z[c] = r[c] / A.diag[c]; }
}

// A_coarse = 1/2 P^T A P, piecewise-constant P over 2x2x2 aggregates (gather form: one thread per owned coarse cell).
// The z-face above the top owned fine plane is a slab interface (or a physical boundary with coefficient 0): always "crossing".
// ref_c / ref_term: fvMatrix::setReference adds a POINT term a_ref to the reference cell's diagonal (k_assemble_pressure); it is what
// makes the closed-box operator non-singular, i.e. 1^T A 1 = a_ref.  The Galerkin product with the factor 1/2 -- right for the Laplacian
// under piecewise-constant transfer -- would halve that term on every level, and an EXACT coarse solve would then over-correct the constant
// mode by 2^levels (measured: 2.0 -> 3.85 PCG iterations per step at C3 when the 120 Jacobi sweeps, which never touched that mode, became
// the direct solve).  So the aggregate that holds the reference cell gets the missing half back: every level carries a_ref unscaled.
__global__ __launch_bounds__(256) void k_mg_coarsen(PMat F, PMat C, int ref_c, const double* __restrict__ ref_term) {
    const int tc = blockIdx.x * 256 + threadIdx.x;
    if (tc >= C.N) return;
    const int I = tc % C.nx, q = tc / C.nx, J = q % C.ny, K = q / C.ny;
    double dg = 0, ux = 0, uy = 0, uz = 0;
    for (int dk = 0; dk < 2; ++dk) {
        const int k = 2 * K + dk; if (k >= F.nz) break;
        for (int dj = 0; dj < 2; ++dj) {
            const int j = 2 * J + dj; if (j >= F.ny) break;
            for (int di = 0; di < 2; ++di) {
                const int i = 2 * I + di; if (i >= F.nx) break;
                const int c = F.c0 + i + F.nx * (j + F.ny * k);
                dg += 0.5 * F.diag[c];
                if (di == 0 && i + 1 < F.nx) dg -= F.ux[c]; else ux += 0.5 * F.ux[c];
                if (dj == 0 && j + 1 < F.ny) dg -= F.uy[c]; else uy += 0.5 * F.uy[c];
                if (dk == 0 && k + 1 < F.nz) dg -= F.uz[c]; else uz += 0.5 * F.uz[c];
            }
        }
    }
    if (tc == ref_c) dg += 0.5 * ref_term[0];
    const int cc = tc + C.c0;
    C.diag[cc] = dg; C.ux[cc] = ux; C.uy[cc] = uy; C.uz[cc] = uz;
}

// a_ref of the comment above: half of the (doubled) diagonal of the reference cell at level 0; 0 on a rank that does not own the cell
__global__ void k_mg_ref_term(PMat A0, int ref_local, double* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = ref_local >= 0 ? 0.5 * A0.diag[A0.c0 + ref_local] : 0.0;
}

// coarse ghost plane under the first owned coarse plane: uz = 1/2 sum of the fine ghost-plane uz of its 2x2 footprint
__global__ __launch_bounds__(256) void k_mg_coarsen_ghost(PMat F, PMat C) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= C.nx * C.ny) return;
    const int I = t % C.nx, J = t / C.nx;
    double uz = 0;
    for (int dj = 0; dj < 2; ++dj) {
        const int j = 2 * J + dj; if (j >= F.ny) break;
        for (int di = 0; di < 2; ++di) {
            const int i = 2 * I + di; if (i >= F.nx) break;
            uz += 0.5 * F.uz[F.c0 - F.nx * F.ny + i + F.nx * j];
        }
    }
    C.uz[C.c0 - C.nx * C.ny + t] = uz;
}

__global__ __launch_bounds__(256) void k_mg_smooth_first(PMat A, const double* __restrict__ b, double* __restrict__ x, double w) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < A.N) { const int c = t + A.c0; x[c] = w * b[c] / A.diag[c]; }
}

// smooth_first + one smooth in a single pass (non-distributed levels >= 1, which are launch-latency bound): the neighbours' first iterate
// x1 = w b / diag is recomputed inline instead of being stored and re-read -- the same operations on the same operands, so x2 is bit-identical
__global__ __launch_bounds__(256) void k_mg_smooth_two_from_zero(PMat A, const double* __restrict__ b, double* __restrict__ xn, double w, double w2) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= A.N) return;
    const int c = t + A.c0;
    const int sy = A.nx, sz = A.nx * A.ny, last = A.ntot - 1;
    const int xm = max(c - 1, 0), xp = min(c + 1, last), ym = max(c - sy, 0), yp = min(c + sy, last), zm = max(c - sz, 0), zp = min(c + sz, last);
    const double dc = A.diag[c], bc = b[c];
    const double x1c = w * bc / dc;
    const double t0 = A.ux[xm] * (w * b[xm] / A.diag[xm]), t1 = A.ux[c] * (w * b[xp] / A.diag[xp]);
    const double t2 = A.uy[ym] * (w * b[ym] / A.diag[ym]), t3 = A.uy[c] * (w * b[yp] / A.diag[yp]);
    const double t4 = A.uz[zm] * (w * b[zm] / A.diag[zm]), t5 = A.uz[c] * (w * b[zp] / A.diag[zp]);
    double a = dc * x1c;                                   // p_row(A, x1, c), same order
    a = (c >= 1) ? a - t0 : a;
    a = (c + 1 < A.ntot) ? a - t1 : a;
    a = (c >= sy) ? a - t2 : a;
    a = (c + sy < A.ntot) ? a - t3 : a;
    a = (c >= sz) ? a - t4 : a;
    a = (c + sz < A.ntot) ? a - t5 : a;
    xn[c] = x1c + w2 * (bc - a) / dc;
}

// the last level-0 sweep of a V-cycle used as PCG preconditioner: z = xn, and PCG wants z.r next -- r is this level's b, already in a
// register -- so the block partials of the dot product (k_dot's, same blocks, same order) come out of the same pass
__global__ __launch_bounds__(256) void k_mg_smooth_dot(PMat A, const double* __restrict__ b, const double* __restrict__ x, double* __restrict__ xn, double w,
                                                       double* __restrict__ partials) {
    double v[1] = {0};
    FY_RED_LOOP(t, A.N) {
        const int c = t + A.c0;
        const double bc = b[c];
        const double z = x[c] + w * (bc - p_row(A, x, c)) / A.diag[c];
        xn[c] = z;
        v[0] += z * bc;
    }
    const int mx[1] = {0};
    block_reduce_store<1>(v, mx, partials);
}
__global__ __launch_bounds__(256) void k_mg_smooth(PMat A, const double* __restrict__ b, const double* __restrict__ x, double* __restrict__ xn, double w) {
    const int t = swz_block(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
    if (t >= A.N) return;
    const int c = t + A.c0;
    xn[c] = x[c] + w * (b[c] - p_row(A, x, c)) / A.diag[c];
}

// First post-smoothing sweep fused with the prolongation: the sweep reads x + P e -- its own cell's and its six neighbours' -- with e
// taken from the (8 x smaller, cache-resident) coarse solution, instead of a separate x += P e pass over the level (one launch and
// 16 B/cell fewer).  Same additions and the same row arithmetic as k_mg_prolong_add followed by k_mg_smooth (p_row's clamped-and-
// selected neighbour terms): bit-identical.  Levels without ghost planes only (c0 = 0).
__global__ __launch_bounds__(256) void k_mg_smooth_prolong(PMat A, const double* __restrict__ b, const double* __restrict__ x, PMat C,
                                                           const double* __restrict__ xc, double* __restrict__ xn, double w) {
    const int c = swz_block(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
    if (c >= A.N) return;
    const int i = c % A.nx, q = c / A.nx, j = q % A.ny, k = q / A.ny;
    const int sy = A.nx, sz = A.nx * A.ny, last = A.ntot - 1;
    const int I = i >> 1, J = j >> 1, K = k >> 1;
    const int Im = max(i - 1, 0) >> 1, Ip = min(i + 1, A.nx - 1) >> 1, Jm = max(j - 1, 0) >> 1, Jp = min(j + 1, A.ny - 1) >> 1,
              Km = max(k - 1, 0) >> 1, Kp = min(k + 1, A.nz - 1) >> 1;
    const double* e = xc + C.c0;
    const int rowc = C.nx * (J + C.ny * K);
    const int xm = max(c - 1, 0), xp = min(c + 1, last), ym = max(c - sy, 0), yp = min(c + sy, last), zm = max(c - sz, 0), zp = min(c + sz, last);
    // (a clamped neighbour index pairs with a clamped parent: its coefficient is zero or the term is deselected below, as in p_row)
    const double vc = x[c] + e[I + rowc];
    const double vxm = x[xm] + e[Im + rowc], vxp = x[xp] + e[Ip + rowc];
    const double vym = x[ym] + e[I + C.nx * (Jm + C.ny * K)], vyp = x[yp] + e[I + C.nx * (Jp + C.ny * K)];
    const double vzm = x[zm] + e[I + C.nx * (J + C.ny * Km)], vzp = x[zp] + e[I + C.nx * (J + C.ny * Kp)];
    const double uxc = A.ux[c], uyc = A.uy[c], uzc = A.uz[c];
    const double t0 = A.ux[xm] * vxm, t1 = uxc * vxp, t2 = A.uy[ym] * vym, t3 = uyc * vyp, t4 = A.uz[zm] * vzm, t5 = uzc * vzp;
    const double dg = A.diag[c];
    double a = dg * vc;
    a = (c >= 1) ? a - t0 : a;
    a = (c + 1 < A.ntot) ? a - t1 : a;
    a = (c >= sy) ? a - t2 : a;
    a = (c + sy < A.ntot) ? a - t3 : a;
    a = (c >= sz) ? a - t4 : a;
    a = (c + sz < A.ntot) ? a - t5 : a;
    xn[c] = vc + w * (b[c] - a) / dg;
}

__global__ __launch_bounds__(256) void k_mg_residual_restrict(PMat A, const double* __restrict__ b, const double* __restrict__ x, PMat C,
                                                              double* __restrict__ bc) {
    const int tc = blockIdx.x * 256 + threadIdx.x;
    if (tc >= C.N) return;
    const int I = tc % C.nx, q = tc / C.nx, J = q % C.ny, K = q / C.ny;
    double acc = 0;
    for (int dk = 0; dk < 2; ++dk) {
        const int k = 2 * K + dk; if (k >= A.nz) break;
        for (int dj = 0; dj < 2; ++dj) {
            const int j = 2 * J + dj; if (j >= A.ny) break;
            for (int di = 0; di < 2; ++di) {
                const int i = 2 * I + di; if (i >= A.nx) break;
                const int c = A.c0 + i + A.nx * (j + A.ny * k);
                acc += b[c] - p_row(A, x, c);
            }
        }
    }
    bc[tc + C.c0] = acc;
}

// Coalesced restriction for the big levels: a 256-thread block covers a 64 x 2 x 2 tile of FINE cells (one lane per fine cell,
// consecutive lanes on consecutive x: every load is a coalesced row), residuals meet in LDS and 32 lanes fold the 8 children of
// each coarse cell.  The gather form above (one thread per coarse cell, 8 strided stencil evaluations each) measured 101 us at
// 160^3 against 41 us for a smoother sweep of the same level.
__global__ __launch_bounds__(256) void k_mg_residual_restrict_tiled(PMat A, const double* __restrict__ b, const double* __restrict__ x, PMat C,
                                                                    double* __restrict__ bc) {
    __shared__ double r[2][2][64];
    const int tx = threadIdx.x & 63, ty = (threadIdx.x >> 6) & 1, tz = threadIdx.x >> 7;
    const int i = blockIdx.x * 64 + tx, j = blockIdx.y * 2 + ty, k = blockIdx.z * 2 + tz;
    double v = 0.0;
    if (i < A.nx && j < A.ny && k < A.nz) {
        const int c = A.c0 + i + A.nx * (j + A.ny * k);
        v = b[c] - p_row(A, x, c);
    }
    r[tz][ty][tx] = v;
    __syncthreads();
    if (threadIdx.x < 32) {
        const int I = blockIdx.x * 32 + (int)threadIdx.x, J = blockIdx.y, K = blockIdx.z;
        if (I < C.nx) {
            const int q = 2 * (int)threadIdx.x;
            bc[C.c0 + I + C.nx * (J + C.ny * K)] = ((r[0][0][q] + r[0][0][q + 1]) + (r[0][1][q] + r[0][1][q + 1])) +
                                                   ((r[1][0][q] + r[1][0][q + 1]) + (r[1][1][q] + r[1][1][q + 1]));
        }
    }
}

// ------------------------------------------------------------------------------------------------ two cells per thread (round 5)
// The scalar-field sweeps of the pressure solver with TWO consecutive cells per thread: every coefficient and field value of the pair and of its
// y / z neighbours comes as one 16-byte load (the x-neighbours of the pair's ends as 8-byte ones), half the load instructions for the same bytes.
// tools/micro/lap_pairs.hip: the Laplacian apply 365 -> 323 us at 320^3 (4.3 -> 4.9 TB/s), 29.4 -> 27.0 us at 160^3, 3.6 -> 2.9 us at 64^3; four cells
// per thread lose (lanes 32 bytes apart).  Needs an even row length, even c0 / N / ntot and 16-byte aligned arrays (pairs_ok); the rows are p_row's
// operations in p_row's order and the block partials are folded in the one-cell kernels' order: the same bits, by construction and by test.
__device__ __forceinline__ double2 ld2(const double* p) { return *reinterpret_cast<const double2*>(p); }
__device__ __forceinline__ void st2(double* p, double a, double b) { *reinterpret_cast<double2*>(p) = make_double2(a, b); }
struct PairIdx { int c, ym, yp, zm, zp, xm, xp; };
__device__ __forceinline__ PairIdx pair_idx(const PMat& A, int c) {
    const int sy = A.nx, sz = A.nx * A.ny, last = A.ntot - 1;
    // (a clamped index is that of a deselected term, or pairs with a zero coefficient -- as in p_row; the pair loads stay inside the array and aligned)
    return PairIdx{c, max(c - sy, 0), min(c + sy, last - 1), max(c - sz, 0), min(c + sz, last - 1), max(c - 1, 0), min(c + 2, last)};
}
struct P2 { double2 c, ym, yp, zm, zp; double xm, xp; };            // a field at the pair, at its y / z neighbour pairs and at the cells left and right of it
__device__ __forceinline__ P2 ld_p2(const double* __restrict__ f, const PairIdx& q) {
    return P2{ld2(f + q.c), ld2(f + q.ym), ld2(f + q.yp), ld2(f + q.zm), ld2(f + q.zp), f[q.xm], f[q.xp]};
}
struct C2 { double2 dg, ux, uy, uz, uym, uzm; double uxm; };
__device__ __forceinline__ C2 ld_c2(const PMat& A, const PairIdx& q) {
    return C2{ld2(A.diag + q.c), ld2(A.ux + q.c), ld2(A.uy + q.c), ld2(A.uz + q.c), ld2(A.uy + q.ym), ld2(A.uz + q.zm), A.ux[q.xm]};
}
// rows c and c + 1 of A applied to the field whose values are X
__device__ __forceinline__ double2 pair_rows(const PMat& A, const C2& K, const P2& X, int c) {
    const int sy = A.nx, sz = A.nx * A.ny, d = c + 1;
    double a = K.dg.x * X.c.x;
    a = (c >= 1) ? a - K.uxm * X.xm : a;
    a = (c + 1 < A.ntot) ? a - K.ux.x * X.c.y : a;
    a = (c >= sy) ? a - K.uym.x * X.ym.x : a;
    a = (c + sy < A.ntot) ? a - K.uy.x * X.yp.x : a;
    a = (c >= sz) ? a - K.uzm.x * X.zm.x : a;
    a = (c + sz < A.ntot) ? a - K.uz.x * X.zp.x : a;
    double b = K.dg.y * X.c.y;
    b = b - K.ux.x * X.c.x;                                           // (d >= 1 always)
    b = (d + 1 < A.ntot) ? b - K.ux.y * X.xp : b;
    b = (d >= sy) ? b - K.uym.y * X.ym.y : b;
    b = (d + sy < A.ntot) ? b - K.uy.y * X.yp.y : b;
    b = (d >= sz) ? b - K.uzm.y * X.zm.y : b;
    b = (d + sz < A.ntot) ? b - K.uz.y * X.zp.y : b;
    return make_double2(a, b);
}
// 128 threads x 2 cells = one 256-cell block of the one-cell kernels; the partial is folded in THEIR order: a wave of theirs is a half-wave here (lane l of it =
// lane l / 2, component l & 1), their shuffle offsets 32 .. 2 are lane offsets 16 .. 1 per component, their offset 1 is x + y in the half-wave's first lane
template <int N>
__device__ __forceinline__ void block_reduce_store_pairs(double2 (&v)[N], const int (&is_max)[N], double* partials, int lb = -1, int stride = 0) {
    if (lb < 0) lb = (int)blockIdx.x;
    if (stride <= 0) stride = (int)gridDim.x;
    __shared__ double sh[4][N];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        double x = v[q].x, y = v[q].y;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            const double x2 = __shfl_down(x, o, 64), y2 = __shfl_down(y, o, 64);
            x = is_max[q] ? fmax(x, x2) : x + x2;
            y = is_max[q] ? fmax(y, y2) : y + y2;
        }
        if ((lane & 31) == 0) sh[2 * wv + (lane >> 5)][q] = is_max[q] ? fmax(x, y) : x + y;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const int q = threadIdx.x;
        double x = sh[0][q];
        for (int w = 1; w < 4; ++w) x = is_max[q] ? fmax(x, sh[w][q]) : x + sh[w][q];
        partials[(size_t)q * stride + lb] = x;
    }
}
// reducing pair kernels: 128 threads, the logical 256-cell block of FY_RED_LOOP; plain ones: 256 threads, 512 cells per block
#define FY_RED_LOOP2(t, n) const int t = swz_block(blockIdx.x, gridDim.x) * 256 + 2 * (int)threadIdx.x; if (t < (n))
#define FY_PAIR_LOOP(t, n) const int t = swz_block(blockIdx.x, gridDim.x) * 512 + 2 * (int)threadIdx.x; if (t < (n))

__global__ __launch_bounds__(256) void k_p_apply2(PMat A, const double* __restrict__ x, double* __restrict__ y) {
    FY_PAIR_LOOP(t, A.N) {
        const int c = t + A.c0;
        const PairIdx q = pair_idx(A, c);
        const double2 a = pair_rows(A, ld_c2(A, q), ld_p2(x, q), c);
        st2(y + c, a.x, a.y);
    }
}
template <bool WITH_R>
__global__ __launch_bounds__(128) void k_p_apply_dot2(PMat A, const double* __restrict__ x, const double* __restrict__ r, double* __restrict__ y, double* __restrict__ partials) {
    double2 v[2] = {make_double2(0, 0), make_double2(0, 0)};
    FY_RED_LOOP2(t, A.N) {
        const int c = t + A.c0;
        const PairIdx q = pair_idx(A, c);
        const P2 X = ld_p2(x, q);
        const double2 a = pair_rows(A, ld_c2(A, q), X, c);
        st2(y + c, a.x, a.y);
        if (WITH_R) { const double2 rc = ld2(r + c); v[0] = make_double2(X.c.x * rc.x, X.c.y * rc.y); }
        v[1] = make_double2(a.x * X.c.x, a.y * X.c.y);
    }
    if (WITH_R) {
        const int mx[2] = {0, 0};
        block_reduce_store_pairs<2>(v, mx, partials);
    } else {
        double2 v1[1] = {v[1]};
        const int mx[1] = {0};
        block_reduce_store_pairs<1>(v1, mx, partials + gridDim.x);
    }
}
template <bool FIRST>
__global__ __launch_bounds__(128) void k_pcg_cg_update2(int n, int c0, const double* __restrict__ u, const double* __restrict__ w, double* __restrict__ p,
                                                        double* __restrict__ sv, double* __restrict__ x, double* __restrict__ r, double* __restrict__ sc, int it,
                                                        double* __restrict__ partials) {
    double2 v[2] = {make_double2(0, 0), make_double2(0, 0)};
    const double gamma = sc[0], delta = sc[1];
    double beta = 0.0, al = gamma / delta;
    if (!FIRST) {
        const double gold = sc[2 + 2 * (it & 1)], aold = sc[3 + 2 * (it & 1)];
        beta = gamma / gold;
        al = gamma / (delta - beta * gamma / aold);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { sc[2 + 2 * ((it + 1) & 1)] = gamma; sc[3 + 2 * ((it + 1) & 1)] = al; }
    FY_RED_LOOP2(t, n) {
        const int c = t + c0;
        double2 pn = ld2(u + c), sn = ld2(w + c);
        if (!FIRST) {
            const double2 po = ld2(p + c), so = ld2(sv + c);
            pn = make_double2(pn.x + beta * po.x, pn.y + beta * po.y); sn = make_double2(sn.x + beta * so.x, sn.y + beta * so.y);
            st2(p + c, pn.x, pn.y); st2(sv + c, sn.x, sn.y);
        }
        const double2 xo = ld2(x + c), ro = ld2(r + c);
        const double xa = xo.x + al * pn.x, xb = xo.y + al * pn.y;
        st2(x + c, xa, xb);
        const double ra = ro.x - al * sn.x, rb = ro.y - al * sn.y;
        st2(r + c, ra, rb);
        v[0] = make_double2(fabs(ra), fabs(rb));
        v[1] = make_double2(xa, xb);
    }
    const int mx[2] = {0, 0};
    block_reduce_store_pairs<2>(v, mx, partials);
}
__global__ __launch_bounds__(256) void k_mg_smooth_two_from_zero2(PMat A, const double* __restrict__ b, double* __restrict__ xn, double w, double w2) {
    const int t = (int)blockIdx.x * 512 + 2 * (int)threadIdx.x;
    if (t >= A.N) return;
    const int c = t + A.c0;
    const PairIdx q = pair_idx(A, c);
    const P2 B = ld_p2(b, q), D = ld_p2(A.diag, q);
    C2 K = ld_c2(A, q);
    K.dg = D.c;
    // the first iterate x1 = w b / diag at the pair and at every neighbour, formed inline as by the one-cell kernel
    P2 X1;
    X1.c = make_double2(w * B.c.x / D.c.x, w * B.c.y / D.c.y);
    X1.ym = make_double2(w * B.ym.x / D.ym.x, w * B.ym.y / D.ym.y); X1.yp = make_double2(w * B.yp.x / D.yp.x, w * B.yp.y / D.yp.y);
    X1.zm = make_double2(w * B.zm.x / D.zm.x, w * B.zm.y / D.zm.y); X1.zp = make_double2(w * B.zp.x / D.zp.x, w * B.zp.y / D.zp.y);
    X1.xm = w * B.xm / D.xm; X1.xp = w * B.xp / D.xp;
    const double2 a = pair_rows(A, K, X1, c);
    st2(xn + c, X1.c.x + w2 * (B.c.x - a.x) / D.c.x, X1.c.y + w2 * (B.c.y - a.y) / D.c.y);
}
__global__ __launch_bounds__(128) void k_mg_smooth_dot2(PMat A, const double* __restrict__ b, const double* __restrict__ x, double* __restrict__ xn, double w,
                                                        double* __restrict__ partials) {
    double2 v[1] = {make_double2(0, 0)};
    FY_RED_LOOP2(t, A.N) {
        const int c = t + A.c0;
        const PairIdx q = pair_idx(A, c);
        const C2 K = ld_c2(A, q);
        const P2 X = ld_p2(x, q);
        const double2 bc = ld2(b + c), a = pair_rows(A, K, X, c);
        const double za = X.c.x + w * (bc.x - a.x) / K.dg.x, zb = X.c.y + w * (bc.y - a.y) / K.dg.y;
        st2(xn + c, za, zb);
        v[0] = make_double2(za * bc.x, zb * bc.y);
    }
    const int mx[1] = {0};
    block_reduce_store_pairs<1>(v, mx, partials);
}
__global__ __launch_bounds__(256) void k_mg_smooth2(PMat A, const double* __restrict__ b, const double* __restrict__ x, double* __restrict__ xn, double w) {
    FY_PAIR_LOOP(t, A.N) {
        const int c = t + A.c0;
        const PairIdx q = pair_idx(A, c);
        const C2 K = ld_c2(A, q);
        const P2 X = ld_p2(x, q);
        const double2 bc = ld2(b + c), a = pair_rows(A, K, X, c);
        st2(xn + c, X.c.x + w * (bc.x - a.x) / K.dg.x, X.c.y + w * (bc.y - a.y) / K.dg.y);
    }
}
// k_mg_smooth_prolong for a pair: the two cells share their parent and the parents of their y / z neighbours
__global__ __launch_bounds__(256) void k_mg_smooth_prolong2(PMat A, const double* __restrict__ b, const double* __restrict__ x, PMat C,
                                                            const double* __restrict__ xc, double* __restrict__ xn, double w) {
    FY_PAIR_LOOP(c, A.N) {
        const int i = c % A.nx, qq = c / A.nx, j = qq % A.ny, k = qq / A.ny;
        const int I = i >> 1, J = j >> 1, Kk = k >> 1;
        const int Im = max(i - 1, 0) >> 1, Ip = min(i + 2, A.nx - 1) >> 1, Jm = max(j - 1, 0) >> 1, Jp = min(j + 1, A.ny - 1) >> 1,
                  Km = max(k - 1, 0) >> 1, Kp = min(k + 1, A.nz - 1) >> 1;
        const double* e = xc + C.c0;
        const int rowc = C.nx * (J + C.ny * Kk);
        const PairIdx q = pair_idx(A, c);
        const C2 K = ld_c2(A, q);
        P2 V = ld_p2(x, q);
        const double ec = e[I + rowc], eym = e[I + C.nx * (Jm + C.ny * Kk)], eyp = e[I + C.nx * (Jp + C.ny * Kk)],
                     ezm = e[I + C.nx * (J + C.ny * Km)], ezp = e[I + C.nx * (J + C.ny * Kp)];
        V.c.x += ec; V.c.y += ec; V.ym.x += eym; V.ym.y += eym; V.yp.x += eyp; V.yp.y += eyp; V.zm.x += ezm; V.zm.y += ezm; V.zp.x += ezp; V.zp.y += ezp;
        V.xm += e[Im + rowc]; V.xp += e[Ip + rowc];
        const double2 bc = ld2(b + c), a = pair_rows(A, K, V, c);
        st2(xn + c, V.c.x + w * (bc.x - a.x) / K.dg.x, V.c.y + w * (bc.y - a.y) / K.dg.y);
    }
}
// k_mg_residual_restrict_tiled with a pair per lane: a block covers (2 PX) x TY x TZ fine cells (PX TY TZ = 256), a lane's two residuals are the first sum of its
// coarse cell's fold, the four lanes of a coarse cell meet in LDS.  The x-extent of the tile is chosen per level so that the blocks of a row are full
// (160 cells = 5 tiles of 32; with a fixed 128-cell tile the second block of a 160-cell row was a quarter full: 42.5 -> 37.3 us at 160^3)
template <int PX, int TY, int TZ>
__global__ __launch_bounds__(256) void k_mg_residual_restrict_tiled2(PMat A, const double* __restrict__ b, const double* __restrict__ x, PMat C,
                                                                     double* __restrict__ bc) {
    static_assert(PX * TY * TZ == 256 && TY % 2 == 0 && TZ % 2 == 0, "tile shape");
    __shared__ double r[TZ][TY][PX];
    const int tx = threadIdx.x % PX, ty = (threadIdx.x / PX) % TY, tz = threadIdx.x / (PX * TY);
    const int i = blockIdx.x * (2 * PX) + 2 * tx, j = blockIdx.y * TY + ty, k = blockIdx.z * TZ + tz;
    double v = 0.0;
    if (i < A.nx && j < A.ny && k < A.nz) {
        const int c = A.c0 + i + A.nx * (j + A.ny * k);
        const PairIdx q = pair_idx(A, c);
        const double2 bb = ld2(b + c), a = pair_rows(A, ld_c2(A, q), ld_p2(x, q), c);
        v = (bb.x - a.x) + (bb.y - a.y);
    }
    r[tz][ty][tx] = v;
    __syncthreads();
    constexpr int NC = PX * (TY / 2) * (TZ / 2);          // coarse cells of the tile
    if ((int)threadIdx.x < NC) {
        const int cx = threadIdx.x % PX, cy = (threadIdx.x / PX) % (TY / 2), cz = threadIdx.x / (PX * (TY / 2));
        const int I = blockIdx.x * PX + cx, J = blockIdx.y * (TY / 2) + cy, K = blockIdx.z * (TZ / 2) + cz;
        if (I < C.nx && J < C.ny && K < C.nz)
            bc[C.c0 + I + C.nx * (J + C.ny * K)] = (r[2 * cz][2 * cy][cx] + r[2 * cz][2 * cy + 1][cx]) + (r[2 * cz + 1][2 * cy][cx] + r[2 * cz + 1][2 * cy + 1][cx]);
    }
}

// The tail of the V-cycle -- every level with <= kMgTailCells cells (20^3 and below at 160^3) -- inside ONE 1024-thread workgroup:
// pre-smoothing, restriction, coarsest solve, prolongation and post-smoothing of up to kMgTailMax levels separated by
// __syncthreads() instead of kernel boundaries.  Those levels are launch/latency bound (4-15 us per launch for microseconds of
// work, ~24 launches per V-cycle); arithmetic and operation order are exactly those of the per-level kernels.
constexpr int kMgCoarseMax = 256;     // = the hierarchy's kMgCoarsest: the coarsest level a single wave solves out of LDS
struct MgTail {
    int n;                       // levels in the tail (level 0 of the tail is the finest of them)
    PMat A[kMgTailMax];
    double* x0[kMgTailMax];
    double* x1[kMgTailMax];
    double* b[kMgTailMax];
    const double* fac;           // banded Cholesky factor of the coarsest operator (k_mg_coarse_factor); null: Jacobi sweeps
    int cache_n, cache_off;      // cache_n > 0: the tail's first level (that many cells, not the coarsest) lives in LDS for the whole kernel, cache_off doubles into the dynamic LDS
};

// The coarsest level's exact solve from its banded Cholesky factor (k_mg_coarse_factor): fac = {N, bw, ok} as three doubles, then the band rows
// [N][bw + 1]: entry d of row i = L(i, i - d), d >= 1, and 1 / L(i, i) at d = 0.  ONE wave does both substitutions with the solution vector in
// REGISTERS (lane l holds rows l and l + 64: N <= 128): per column the owner's value is broadcast with a lane read, every lane in the band
// updates its row with one multiply-subtract -- no LDS round trip in the dependent chain, ~40 cycles per column, a few microseconds per solve
// (the 120 Jacobi sweeps they replace took ~60).  `Ls` (LDS, N * (bw + 1) doubles) must hold the factor; called by the wave tid < 64 only.
__device__ __forceinline__ double read_lane_f64(double v, int src_lane) {      // src_lane is wave-uniform: two v_readlane, no LDS crossbar
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
    return __hiloint2double(hi, lo);
}
// one sweep of eight-column groups over columns [ja, jb) (FWD: ascending, L y = b; else descending, L^T x = y) whose owners' values sit in v0 (LO) or v1.
// Per column the ONLY dependent chain is  lane read of the owner -> times 1 / L(j, j) -> times the row's coefficient -> subtract:  the coefficients come up front
// from clamped LDS addresses, zeroed where a row is not in the column's band (subtracting 0 * y leaves a row as it is), and an owner is NOT overwritten with its
// result inside the loop -- once its column has passed nothing changes it any more, so all owners are scaled by their 1 / L(i, i) in one operation afterwards
// (the same product the loop formed for the updates).  Round 5, measured with timing-only variants of the tail at C3: empty kernel 4.8 us, way down (first level in
// LDS) + 3.3, factor into LDS + 2.4, THIS solve + 30, way up + 5.5.  Factor entries fetched up front instead of in the chain: 51.4 -> 46.2 us; selects and the
// owner's write-back out of the chain (8 instructions per column, 4 of them dependent): 43.1.  What is left is ~27 ns per dependent operation of a lone wave.
// (DO0 / DO1: whether rows < 64 / rows >= 64 can lie in the band of the columns of this range at all -- a range that cannot touch one half skips its work)
template <bool FWD, bool LO, bool DO0, bool DO1>
__device__ __forceinline__ void band_columns(const double* Ls, int N, int bw, int ja, int jb, int lane, double& v0, double& v1) {
    if (jb <= ja) return;
    constexpr int U = 8;
    const int Wd = bw + 1, r0 = min(lane, N - 1), r1 = min(lane + 64, N - 1);
    for (int g = 0; g < jb - ja; g += U) {
        double dj[U], a0[U], a1[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int jr = FWD ? ja + g + u : jb - 1 - g - u;                 // the column (may run past the range: then its coefficients are zero)
            const bool live = FWD ? jr < jb : jr >= ja;
            const int j = min(max(jr, 0), N - 1);
            dj[u] = live ? Ls[(size_t)j * Wd] : 0.0;
            const int d0 = FWD ? lane - jr : jr - lane, d1 = FWD ? lane + 64 - jr : jr - (lane + 64);      // distance of my rows from the diagonal, on the side the sweep updates
            a0[u] = 0.0; a1[u] = 0.0;
            if (DO0) {
                const double c0 = FWD ? Ls[(size_t)r0 * Wd + min(max(d0, 0), bw)] : Ls[(size_t)j * Wd + min(max(d0, 0), bw)];
                a0[u] = (live && d0 >= 1 && d0 <= bw && lane < N) ? c0 : 0.0;
            }
            if (DO1) {
                const double c1 = FWD ? Ls[(size_t)r1 * Wd + min(max(d1, 0), bw)] : Ls[(size_t)j * Wd + min(max(d1, 0), bw)];
                a1[u] = (live && d1 >= 1 && d1 <= bw && lane + 64 < N) ? c1 : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int jr = FWD ? ja + g + u : jb - 1 - g - u;
            const int j = min(max(jr, 0), N - 1);
            const double yj = read_lane_f64(LO ? v0 : v1, j & 63) * dj[u];
            if (DO0) v0 -= a0[u] * yj;
            if (DO1) v1 -= a1[u] * yj;
        }
    }
}
__device__ __forceinline__ void coarse_band_solve(const double* Ls, int N, int bw, const double* __restrict__ b, double* __restrict__ x, int lane) {
    const int Wd = bw + 1;
    double v0 = lane < N ? b[lane] : 0.0, v1 = lane + 64 < N ? b[lane + 64] : 0.0;
    const double dg0 = Ls[(size_t)min(lane, N - 1) * Wd], dg1 = Ls[(size_t)min(lane + 64, N - 1) * Wd];      // 1 / L(i, i) of my rows
    const int n0 = min(N, 64);
    // forward: L y = b.  Column j reaches rows j + 1 .. j + bw: rows >= 64 only from column 64 - bw on, rows < 64 only from columns < 64
    const int js = min(max(64 - bw, 0), n0);
    band_columns<true, true, true, false>(Ls, N, bw, 0, js, lane, v0, v1);
    band_columns<true, true, true, true>(Ls, N, bw, js, n0, lane, v0, v1);
    band_columns<true, false, false, true>(Ls, N, bw, 64, N, lane, v0, v1);
    v0 *= dg0; v1 *= dg1;
    // backward: L^T x = y.  Column j reaches rows j - bw .. j - 1: rows < 64 from columns < 64 + bw, rows >= 64 only from columns > 64
    const int jt = min(64 + bw, N);
    band_columns<false, false, false, true>(Ls, N, bw, jt, N, lane, v0, v1);
    band_columns<false, false, true, true>(Ls, N, bw, 64, jt, lane, v0, v1);
    band_columns<false, true, true, false>(Ls, N, bw, 0, n0, lane, v0, v1);
    v0 *= dg0; v1 *= dg1;
    if (lane < N) x[lane] = v0;
    if (lane + 64 < N) x[lane + 64] = v1;
}

__global__ __launch_bounds__(1024) void k_mg_tail(MgTail T, double w, int coarse_sweeps, MgWeights W) {
    const int tid = threadIdx.x;
    extern __shared__ double tail_lds[];
    // The tail's first level (<= kMgTailCells cells: one cell per thread) is touched by ~7 sweeps, each one global round trip and a barrier long: its operator,
    // right-hand side and both iterates are held in LDS instead (round 5; the same p_row on the same values, through generic pointers)
    const bool cached = T.cache_n > 0;
    double* const lc = tail_lds + T.cache_off;
    PMat AL = T.A[0];
    if (cached) {
        const int N0 = T.cache_n;
        AL.diag = lc; AL.ux = lc + N0; AL.uy = lc + 2 * N0; AL.uz = lc + 3 * N0;
        for (int c = tid; c < N0; c += 1024) {
            AL.diag[c] = T.A[0].diag[c]; AL.ux[c] = T.A[0].ux[c]; AL.uy[c] = T.A[0].uy[c]; AL.uz[c] = T.A[0].uz[c];
            lc[4 * N0 + c] = T.b[0][c];
        }
        __syncthreads();
    }
    const double* const lb = lc + 4 * T.cache_n;
    double* const lx0 = lc + 5 * T.cache_n;
    double* const lx1 = lc + 6 * T.cache_n;
    // ---- down: smooth_first, smooth, residual -> restricted rhs of the next level
    for (int l = 0; l + 1 < T.n; ++l) {
        const bool in_lds = cached && l == 0;
        const PMat A = in_lds ? AL : T.A[l];
        const double* b = in_lds ? lb : T.b[l];
        double* xa = in_lds ? lx0 : T.x0[l];
        double* xb = in_lds ? lx1 : T.x1[l];
        for (int c = tid; c < A.N; c += 1024) xa[c] = W.w[0] * b[c] / A.diag[c];
        __syncthreads();
        for (int s = 1; s < W.n; ++s) {                       // the iterate alternates between x0 and x1; W.n is even, so it ends in x1
            for (int c = tid; c < A.N; c += 1024) xb[c] = xa[c] + W.w[s] * (b[c] - p_row(A, xa, c)) / A.diag[c];
            __syncthreads();
            double* t = xa; xa = xb; xb = t;
        }
        { double* t = xa; xa = xb; xb = t; }                  // xb = the level's iterate (x1), xa the scratch (x0)
        const PMat Cc = T.A[l + 1];
        double* bc = T.b[l + 1];
        for (int cc = tid; cc < Cc.N; cc += 1024) {
            const int I = cc % Cc.nx, q = cc / Cc.nx, J = q % Cc.ny, K = q / Cc.ny;
            double acc = 0;
            for (int dk = 0; dk < 2; ++dk) {
                const int k = 2 * K + dk; if (k >= A.nz) break;
                for (int dj = 0; dj < 2; ++dj) {
                    const int j = 2 * J + dj; if (j >= A.ny) break;
                    for (int di = 0; di < 2; ++di) {
                        const int i = 2 * I + di; if (i >= A.nx) break;
                        const int c = i + A.nx * (j + A.ny * k);
                        acc += b[c] - p_row(A, xb, c);
                    }
                }
            }
            bc[cc] = acc;
        }
        __syncthreads();
    }
    // ---- coarsest level (<= kMgCoarseMax cells): damped-Jacobi sweeps from a zero guess, result in x0.  ONE wave does all sweeps out of
    // LDS: 40 sweeps behind a 16-wave workgroup barrier each cost ~48 of this kernel's 55 us; inside a single wave the LDS operations
    // are ordered by the hardware and no barrier is needed at all.  Same arithmetic in the same order as the multi-wave loop.
    {
        const int l = T.n - 1;
        const PMat A = T.A[l];
        const double* b = T.b[l];
        __shared__ double c_dg[kMgCoarseMax], c_ux[kMgCoarseMax], c_uy[kMgCoarseMax], c_uz[kMgCoarseMax], c_b[kMgCoarseMax];
        __shared__ double c_x[2][kMgCoarseMax];
        if (T.fac && A.N <= kMgDirectMax && T.fac[2] == 1.0) {        // (uniform) the level's exact solve from its banded Cholesky factor
            double* const fac_lds = tail_lds;
            const int bw = (int)T.fac[1], cnt = A.N * (bw + 1);
            for (int q = tid; q < cnt; q += 1024) fac_lds[q] = T.fac[3 + q];
            __syncthreads();
            if (tid < 64) coarse_band_solve(fac_lds, A.N, bw, b, T.x0[l], tid);
            __syncthreads();
        } else if (A.N <= kMgCoarseMax) {
            if (tid < 64) {
                const int N = A.N, sy = A.nx, sz = A.nx * A.ny;
                for (int c = tid; c < N; c += 64) {
                    c_dg[c] = A.diag[c]; c_ux[c] = A.ux[c]; c_uy[c] = A.uy[c]; c_uz[c] = A.uz[c]; c_b[c] = b[c];
                    c_x[0][c] = w * b[c] / A.diag[c];
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
                int cur = 0;
                constexpr int R = kMgCoarseMax / 64;                    // cells per lane, processed together: their dependent FP64 chains
                for (int s = 1; s < coarse_sweeps; ++s) {               // (7 multiply-subtracts + a division) overlap instead of queueing
                    const double* xc = c_x[cur];
                    double* xn = c_x[cur ^ 1];
                    double a[R], xo[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int c = tid + 64 * r;
                        a[r] = 0.0; xo[r] = 0.0;
                        if (c < N) {
                            // p_row in the same order; the guarded terms are loaded from clamped addresses and selected, so the seven
                            // LDS reads go out together instead of one per divergent branch (that serialisation was the sweep's cost)
                            const int xm = max(c - 1, 0), xp = min(c + 1, N - 1), ym = max(c - sy, 0), yp = min(c + sy, N - 1);
                            const int zm = max(c - sz, 0), zp = min(c + sz, N - 1);
                            xo[r] = xc[c];
                            const double t0 = c_ux[xm] * xc[xm], t1 = c_ux[c] * xc[xp], t2 = c_uy[ym] * xc[ym], t3 = c_uy[c] * xc[yp];
                            const double t4 = c_uz[zm] * xc[zm], t5 = c_uz[c] * xc[zp];
                            double v = c_dg[c] * xo[r];
                            v = (c >= 1) ? v - t0 : v;
                            v = (c + 1 < N) ? v - t1 : v;
                            v = (c >= sy) ? v - t2 : v;
                            v = (c + sy < N) ? v - t3 : v;
                            v = (c >= sz) ? v - t4 : v;
                            v = (c + sz < N) ? v - t5 : v;
                            a[r] = v;
                        }
                    }
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int c = tid + 64 * r;
                        if (c < N) xn[c] = xo[r] + w * (c_b[c] - a[r]) / c_dg[c];
                    }
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
                    cur ^= 1;
                }
                for (int c = tid; c < N; c += 64) T.x0[l][c] = c_x[cur][c];
            }
            __syncthreads();
        } else {
            double* cur = T.x0[l];
            double* nxt = T.x1[l];
            for (int c = tid; c < A.N; c += 1024) cur[c] = w * b[c] / A.diag[c];
            __syncthreads();
            for (int s = 1; s < coarse_sweeps; ++s) {
                for (int c = tid; c < A.N; c += 1024) nxt[c] = cur[c] + w * (b[c] - p_row(A, cur, c)) / A.diag[c];
                __syncthreads();
                double* t = cur; cur = nxt; nxt = t;
            }
            if (cur != T.x0[l]) { for (int c = tid; c < A.N; c += 1024) T.x0[l][c] = cur[c]; __syncthreads(); }
        }
    }
    // ---- up: prolongation + two post-smoothing sweeps; a level's result ends in x1 (the coarsest's in x0)
    for (int l = T.n - 2; l >= 0; --l) {
        const bool in_lds = cached && l == 0;
        const PMat A = in_lds ? AL : T.A[l];
        const PMat Cc = T.A[l + 1];
        const double* b = in_lds ? lb : T.b[l];
        const double* xc = (l + 1 == T.n - 1) ? T.x0[l + 1] : T.x1[l + 1];
        double* xb = in_lds ? lx1 : T.x1[l];
        double* xa = in_lds ? lx0 : T.x0[l];
        for (int c = tid; c < A.N; c += 1024) {
            const int i = c % A.nx, q = c / A.nx, j = q % A.ny, k = q / A.ny;
            xb[c] += xc[(i >> 1) + Cc.nx * ((j >> 1) + Cc.ny * (k >> 1))];
        }
        __syncthreads();
        for (int s = W.n - 1; s >= 0; --s) {                  // post-smoothing: the weights in reverse; W.n even: the result is back in x1
            for (int c = tid; c < A.N; c += 1024) xa[c] = xb[c] + W.w[s] * (b[c] - p_row(A, xb, c)) / A.diag[c];
            __syncthreads();
            double* t = xa; xa = xb; xb = t;
        }
    }
    if (cached) for (int c = tid; c < T.cache_n; c += 1024) T.x1[0][c] = lx1[c];      // the level above prolongs from x1
}

__global__ __launch_bounds__(256) void k_mg_prolong_add(PMat A, double* __restrict__ x, PMat C, const double* __restrict__ xc) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= A.N) return;
    const int i = t % A.nx, q = t / A.nx, j = q % A.ny, k = q / A.ny;
    x[t + A.c0] += xc[C.c0 + (i >> 1) + C.nx * ((j >> 1) + C.ny * (k >> 1))];
}

// the same over a range of z-planes that starts `kofs` planes away from the level's first owned plane (negative: ghost planes below it; the
// communication-avoiding V-cycle of a z-slab, fv_pressure.cpp): C.c0 is the coarse cell under the fine level's first OWNED cell
__global__ __launch_bounds__(256) void k_mg_prolong_add_planes(PMat A, int kofs, double* __restrict__ x, PMat C, const double* __restrict__ xc) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= A.N) return;
    const int i = t % A.nx, q = t / A.nx, j = q % A.ny, k = q / A.ny + kofs;
    const int K = k >= 0 ? (k >> 1) : -((1 - k) >> 1);                  // floor(k / 2)
    x[t + A.c0] += xc[C.c0 + (i >> 1) + C.nx * ((j >> 1) + C.ny * K)];
}

// coarsest level (N <= 1024, never distributed: c0 = 0): all sweeps inside one workgroup
// The coarsest operator (<= kMgDirectMax = 128 cells) only changes when the pressure matrix is assembled, and every V-cycle in between solves
// with it: so it is FACTORED once per assembly -- banded Cholesky A = L L^T in LDS (band width = the operator's z stride, 25 for the 5^3
// level of C3: N bw^2 = 78 k multiply-adds; a dense 125^3 inversion was built first and cost 0.5 ms, LDS-bandwidth bound), one workgroup, one barrier per column -- and a V-cycle's coarse solve is two banded substitutions in one wave (coarse_band_solve) instead of
// 120 Jacobi sweeps that left the level's smoothest modes partly in.  The operator is a symmetric positive definite M-matrix (the
// reference cell or a fixed-value patch makes it non-singular); fac[2] = 0 if a pivot is not positive and finite (the sweeps then stand in).
template <int Q>
__global__ __launch_bounds__(1024) void k_mg_coarse_factor(PMat A, int bw, double* __restrict__ fac) {
    extern __shared__ double B[];                  // [N][bw + 1]: B[i][d] = A(i, i - d), overwritten by L
    __shared__ int bad;
    const int N = A.N, tid = threadIdx.x, NT = (int)blockDim.x, Wd = bw + 1, sy = A.nx, sz = A.nx * A.ny;
    if (tid == 0) bad = 0;
    for (int e = tid; e < N * Wd; e += NT) B[e] = 0.0;
    __syncthreads();
    for (int c = tid; c < N; c += NT) {          // the lower half of row c of p_row (zero coefficients at the walls); += : strides coincide on flat grids
        double* row = B + (size_t)c * Wd;
        row[0] += A.diag[c];
        if (c >= 1) row[1] -= A.ux[c - 1];
        if (A.ny > 1 && c >= sy && sy <= bw) row[sy] -= A.uy[c - sy];
        if (A.nz > 1 && c >= sz && sz <= bw) row[sz] -= A.uz[c - sz];
    }
    __syncthreads();
    // Right-looking elimination with the column entries left UNSCALED (they hold L(i, j) L(j, j)): the trailing update of column j,
    // A(i, k) -= A(i, j) A(k, j) / A(j, j) for j < k <= i <= j + m, reads column j and writes columns > j only -- ONE barrier per column --
    // and the division by L(j, j) is applied to every entry at the end.  A thread owns fixed positions (a, b) of the bw x bw update window
    // (bw <= 64: at most four), so there is no index arithmetic in the loop.
    // (round 5: only the lower triangle b <= a of the window does anything -- its bw (bw + 1) / 2 positions are dealt out, Q per thread; see the launcher)
    int ua[Q], ub[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int e = tid + NT * q;
        int a = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
        while ((a + 1) * (a + 2) / 2 <= e) ++a;             // (guards the rounding of the square root)
        while (a * (a + 1) / 2 > e) --a;
        ua[q] = a; ub[q] = e - a * (a + 1) / 2;
    }
    for (int j = 0; j < N; ++j) {
        const double d = B[(size_t)j * Wd];
        if (!(d > 0.0) || !(d < 1e300)) { if (tid == 0) bad = 1; break; }      // (uniform: every thread reads the same value)
        const double id = 1.0 / d;
        const int m = min(bw, N - 1 - j);           // rows below the diagonal in this column
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int a = ua[q], b = ub[q];
            if (a < m) B[(size_t)(j + 1 + a) * Wd + (a - b)] -= (B[(size_t)(j + 1 + a) * Wd + 1 + a] * B[(size_t)(j + 1 + b) * Wd + 1 + b]) * id;
        }
        __syncthreads();
    }
    __syncthreads();
    if (!bad) {
        for (int i = tid; i < N; i += NT) fac[3 + (size_t)i * Wd] = 1.0 / sqrt(B[(size_t)i * Wd]);      // 1 / L(i, i): the substitutions multiply
        for (int e = tid; e < N * Wd; e += NT) {
            const int i = e / Wd, dd = e - i * Wd;
            if (dd >= 1) fac[3 + e] = dd <= i ? B[e] / sqrt(B[(size_t)(i - dd) * Wd]) : 0.0;                   // L(i, i - dd) = stored / L(i - dd, i - dd)
        }
    }
    if (tid == 0) { fac[0] = (double)N; fac[1] = (double)bw; fac[2] = bad ? 0.0 : 1.0; }
}

__global__ __launch_bounds__(1024) void k_mg_coarse_solve(PMat A, const double* __restrict__ b, double* __restrict__ x, double* __restrict__ tmp,
                                                          int sweeps, double w, const double* __restrict__ fac) {
    if (fac && A.N <= kMgDirectMax && fac[2] == 1.0) {        // (uniform)
        extern __shared__ double fac_lds[];
        const int bw = (int)fac[1], cnt = A.N * (bw + 1);
        for (int q = threadIdx.x; q < cnt; q += 1024) fac_lds[q] = fac[3 + q];
        __syncthreads();
        if (threadIdx.x < 64) coarse_band_solve(fac_lds, A.N, bw, b, x, threadIdx.x);
        return;
    }
    const int c = threadIdx.x;
    const bool act = c < A.N;
    double* cur = x;
    double* nxt = tmp;
    if (act) cur[c] = w * b[c] / A.diag[c];
    __syncthreads();
    for (int s = 1; s < sweeps; ++s) {
        if (act) nxt[c] = cur[c] + w * (b[c] - p_row(A, cur, c)) / A.diag[c];
        __syncthreads();
        double* t = cur; cur = nxt; nxt = t;
    }
    if (cur != x) { if (act) x[c] = cur[c]; }
}

// GeometricField::relax(alpha), pEqn.H:41: p = prevIter + alpha (p - prevIter)
__global__ __launch_bounds__(256) void k_relax_field(double* __restrict__ x, const double* __restrict__ prev, double alpha, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] = prev[i] + alpha * (x[i] - prev[i]);
}

__global__ __launch_bounds__(256) void k_copy(double* __restrict__ dst, const double* __restrict__ src, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

__global__ __launch_bounds__(256) void k_add(double* __restrict__ y, const double* __restrict__ x, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] += x[i];
}

// Boussinesq buoyancy (fy_thermal_desc.beta): a_c = (-beta (T_c - T_ref)) g, and the momentum equations' source uSource + a.  One thread per component of a cell
__global__ __launch_bounds__(256) void k_buoyancy(size_t n3, const double* __restrict__ T, double beta, double T_ref, double gx, double gy, double gz,
                                                  const double* __restrict__ uSource, double* __restrict__ a_out, double* __restrict__ sum_out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n3) return;
    const size_t c = e / 3;
    const int q = (int)(e - 3 * c);
    const double a = (-beta * (T[c] - T_ref)) * (q == 0 ? gx : q == 1 ? gy : gz);
    a_out[e] = a;
    sum_out[e] = uSource[e] + a;
}

}  // namespace

int launch_buoyancy(hipStream_t s, size_t n_cells, const double* T, double beta, double T_ref, const double* g, const double* uSource, double* a, double* sum) {
    if (!n_cells) return FY_OK;
    hipLaunchKernelGGL(k_buoyancy, dim3(div_up(3 * n_cells, 256)), dim3(256), 0, s, 3 * n_cells, T, beta, T_ref, g[0], g[1], g[2], uSource, a, sum);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_reduce_finalize(hipStream_t s, const double* partials, int n_cells, int nslots, const int* ops, double* out, unsigned long long* flag,
                           unsigned long long seq) {
    hipLaunchKernelGGL(k_reduce_finalize, dim3(nslots), dim3(1024), 0, s, partials, red_blocks(n_cells), ops, out, flag, seq);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_sum3(hipStream_t s, const double* x, int n, double* partials) {
    hipLaunchKernelGGL(k_sum3, dim3(red_blocks(n)), dim3(256), 0, s, x, n, partials);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

// two cells per thread where the level allows it (see "two cells per thread" above); FOAMYADE_NO_PAIRS=1: the one-cell kernels everywhere (A/B switch, same bits)
static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static bool pairs_ok(const PMat& A) {
    return !pairs_disabled() && A.N >= 2 && A.nx % 2 == 0 && A.c0 % 2 == 0 && A.N % 2 == 0 && A.ntot % 2 == 0 && al16(A.diag) && al16(A.ux) && al16(A.uy) && al16(A.uz);
}
static bool pairs_ok(int n, int c0) {
    return !pairs_disabled() && n >= 2 && n % 2 == 0 && c0 % 2 == 0;
}

int launch_p_apply(hipStream_t s, PMat A, const double* x, double* y) {
    if (pairs_ok(A) && al16(x) && al16(y)) {
        hipLaunchKernelGGL(k_p_apply2, dim3(div_up(A.N, 512)), dim3(256), 0, s, A, x, y);
        FY_LAUNCH_CHECK();
        return FY_OK;
    }
    hipLaunchKernelGGL(k_p_apply, dim3(div_up(A.N, 256)), dim3(256), 0, s, A, x, y);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_p_apply_dot(hipStream_t s, PMat A, const double* x, const double* r, double* y, double* partials) {
    if (pairs_ok(A) && al16(x) && al16(y) && al16(r)) {
        if (r) hipLaunchKernelGGL(k_p_apply_dot2<true>, dim3(red_blocks(A.N)), dim3(128), 0, s, A, x, r, y, partials);
        else hipLaunchKernelGGL(k_p_apply_dot2<false>, dim3(red_blocks(A.N)), dim3(128), 0, s, A, x, r, y, partials);
    }
    else if (r) hipLaunchKernelGGL(k_p_apply_dot<true>, dim3(red_blocks(A.N)), dim3(256), 0, s, A, x, r, y, partials);
    else hipLaunchKernelGGL(k_p_apply_dot<false>, dim3(red_blocks(A.N)), dim3(256), 0, s, A, x, r, y, partials);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_p_init(hipStream_t s, PMat A, const double* b, const double* x, const double* xsum_dev, double xsum_val, double inv_n, double* r, double* partials) {
    hipLaunchKernelGGL(k_p_init, dim3(red_blocks(A.N)), dim3(256), 0, s, A, b, x, xsum_dev, xsum_val, inv_n, r, partials);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_dot(hipStream_t s, int n, int c0, const double* a, const double* b, double* partials) {
    hipLaunchKernelGGL(k_dot, dim3(red_blocks(n)), dim3(256), 0, s, n, c0, a, b, partials);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_pcg_cg_update(hipStream_t s, int n, int c0, const double* u, const double* w, double* p, double* sv, double* x, double* r, double* sc, int it, double* partials) {
    if (pairs_ok(n, c0) && al16(u) && al16(w) && al16(p) && al16(sv) && al16(x) && al16(r)) {
        if (it == 0) hipLaunchKernelGGL(k_pcg_cg_update2<true>, dim3(red_blocks(n)), dim3(128), 0, s, n, c0, u, w, p, sv, x, r, sc, it, partials);
        else hipLaunchKernelGGL(k_pcg_cg_update2<false>, dim3(red_blocks(n)), dim3(128), 0, s, n, c0, u, w, p, sv, x, r, sc, it, partials);
    }
    else if (it == 0) hipLaunchKernelGGL(k_pcg_cg_update<true>, dim3(red_blocks(n)), dim3(256), 0, s, n, c0, u, w, p, sv, x, r, sc, it, partials);
    else hipLaunchKernelGGL(k_pcg_cg_update<false>, dim3(red_blocks(n)), dim3(256), 0, s, n, c0, u, w, p, sv, x, r, sc, it, partials);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_jacobi_precond(hipStream_t s, PMat A, const double* r, double* z) {
    hipLaunchKernelGGL(k_jacobi_precond, dim3(div_up(A.N, 256)), dim3(256), 0, s, A, r, z);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_mg_ref_term(hipStream_t s, PMat A0, int ref_local, double* out) {
    hipLaunchKernelGGL(k_mg_ref_term, dim3(1), dim3(64), 0, s, A0, ref_local, out);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_mg_coarsen(hipStream_t s, PMat F, PMat C, int ref_c, const double* ref_term) {
    hipLaunchKernelGGL(k_mg_coarsen, dim3(div_up(C.N, 256)), dim3(256), 0, s, F, C, ref_term ? ref_c : -1, ref_term);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_mg_smooth_first(hipStream_t s, PMat A, const double* b, double* x, double w) {
    hipLaunchKernelGGL(k_mg_smooth_first, dim3(div_up(A.N, 256)), dim3(256), 0, s, A, b, x, w);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_mg_smooth_two_from_zero(hipStream_t s, PMat A, const double* b, double* xn, double w, double w2) {
    if (pairs_ok(A) && al16(b) && al16(xn)) hipLaunchKernelGGL(k_mg_smooth_two_from_zero2, dim3(div_up(A.N, 512)), dim3(256), 0, s, A, b, xn, w, w2);
    else hipLaunchKernelGGL(k_mg_smooth_two_from_zero, dim3(div_up(A.N, 256)), dim3(256), 0, s, A, b, xn, w, w2);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_mg_smooth_dot(hipStream_t s, PMat A, const double* b, const double* x, double* xn, double w, double* partials) {
    if (pairs_ok(A) && al16(b) && al16(x) && al16(xn)) hipLaunchKernelGGL(k_mg_smooth_dot2, dim3(red_blocks(A.N)), dim3(128), 0, s, A, b, x, xn, w, partials);
    else hipLaunchKernelGGL(k_mg_smooth_dot, dim3(red_blocks(A.N)), dim3(256), 0, s, A, b, x, xn, w, partials);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_mg_smooth(hipStream_t s, PMat A, const double* b, const double* x, double* xn, double w) {
    if (pairs_ok(A) && al16(b) && al16(x) && al16(xn)) hipLaunchKernelGGL(k_mg_smooth2, dim3(div_up(A.N, 512)), dim3(256), 0, s, A, b, x, xn, w);
    else hipLaunchKernelGGL(k_mg_smooth, dim3(div_up(A.N, 256)), dim3(256), 0, s, A, b, x, xn, w);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

// band width of a level's operator = its largest neighbour stride
static int band_width(const PMat& A) { return A.nz > 1 ? A.nx * A.ny : (A.ny > 1 ? A.nx : 1); }
static size_t fac_lds_bytes(int N, int bw) { return (size_t)N * (size_t)(bw + 1) * sizeof(double); }
static int allow_big_lds(const void* fn) {
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fac_lds_bytes(kMgDirectMax, kMgDirectBand)) == hipSuccess ? FY_OK
           : fail(FY_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
}

int mg_coarse_factor_doubles(PMat A) { return 3 + A.N * (band_width(A) + 1); }
bool mg_coarse_direct_ok(PMat A) { return A.c0 == 0 && A.N <= kMgDirectMax && band_width(A) <= kMgDirectBand; }

int launch_mg_coarse_factor(hipStream_t s, PMat A, double* fac) {
    if (!(mg_coarse_direct_ok)(A)) return fail(FY_ERR_INVALID, "direct coarse solve: level of %d cells, band %d (ghost offset %d)", A.N, band_width(A), A.c0);
    static bool attr_set = false;
    if (!attr_set) {
        FY_TRY(allow_big_lds(reinterpret_cast<const void*>(k_mg_coarse_factor<1>)));
        FY_TRY(allow_big_lds(reinterpret_cast<const void*>(k_mg_coarse_factor<2>)));
        FY_TRY(allow_big_lds(reinterpret_cast<const void*>(k_mg_coarse_factor<3>)));
        attr_set = true;
    }
    const int bw = band_width(A);
    // the update window's lower triangle dealt out Q positions per thread.  The kernel is one barrier and one dependent LDS round trip per column: fewer
    // positions per thread shorten the round trip, fewer waves the barrier (measured at the 5^3 level, band 25, 325 positions: 1024 threads x 4 positions of the
    // full window 72 us, 256 x 4 of the full window 51; of the triangle: 64 x 6 81, 128 x 3 54, 192 x 2 44, 384 x 1 39 us)
    const int tri = bw * (bw + 1) / 2;
    const int q = tri <= 1024 ? 1 : (tri <= 2048 ? 2 : 3);
    const int nt = std::min(1024, ((tri + q - 1) / q + 63) / 64 * 64);
    if (q == 1) hipLaunchKernelGGL(k_mg_coarse_factor<1>, dim3(1), dim3(nt), fac_lds_bytes(A.N, bw), s, A, bw, fac);
    else if (q == 2) hipLaunchKernelGGL(k_mg_coarse_factor<2>, dim3(1), dim3(nt), fac_lds_bytes(A.N, bw), s, A, bw, fac);
    else hipLaunchKernelGGL(k_mg_coarse_factor<3>, dim3(1), dim3(nt), fac_lds_bytes(A.N, bw), s, A, bw, fac);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_mg_tail(hipStream_t s, const PMat* A, double* const* x0, double* const* x1, double* const* b, int n, double w, int coarse_sweeps, MgWeights W,
                   const double* fac) {
    if (n < 1 || n > kMgTailMax) return fail(FY_ERR_INVALID, "bad multigrid tail depth %d", n);
    MgTail T;
    T.n = n;
    T.fac = fac;
    size_t lds = 0;
    static bool attr_set = false;
    if (!attr_set) {      // the factor of the coarsest level + seven arrays of the tail's first level
        const int want = (int)(fac_lds_bytes(kMgDirectMax, kMgDirectBand) + 7 * (size_t)kMgTailCells * sizeof(double));
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_mg_tail), hipFuncAttributeMaxDynamicSharedMemorySize, want) != hipSuccess)
            return fail(FY_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
        attr_set = true;
    }
    if (fac) {
        if (!(mg_coarse_direct_ok)(A[n - 1])) return fail(FY_ERR_INVALID, "multigrid tail: a factor was handed over for a level it cannot belong to");
        lds = fac_lds_bytes(A[n - 1].N, band_width(A[n - 1]));
    }
    T.cache_n = 0; T.cache_off = (int)(lds / sizeof(double));
    if (!tail_cache_disabled() && n >= 2 && A[0].N <= kMgTailCells) { T.cache_n = A[0].N; lds += 7 * (size_t)A[0].N * sizeof(double); }
    for (int l = 0; l < n; ++l) {
        if (A[l].c0 != 0) return fail(FY_ERR_INVALID, "multigrid tail levels must not carry ghost planes");
        T.A[l] = A[l]; T.x0[l] = x0[l]; T.x1[l] = x1[l]; T.b[l] = b[l];
    }
    if (W.n < 2 || (W.n & 1)) return fail(FY_ERR_INVALID, "the multigrid tail needs an even number of smoothing sweeps");
    hipLaunchKernelGGL(k_mg_tail, dim3(1), dim3(1024), lds, s, T, w, coarse_sweeps, W);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_mg_residual_restrict(hipStream_t s, PMat A, const double* b, const double* x, PMat C, double* bc) {
    if (C.N > 8192 && C.ny * 2 >= A.ny && C.nz * 2 >= A.nz) {       // big level: coalesced tile kernel (grid.y/z = coarse rows/planes)
        if (pairs_ok(A) && al16(b) && al16(x) && A.ny % 2 == 0 && A.nz % 2 == 0) {
            // the tile's x-extent (8, 16, 32 or 64 pairs) that wastes the fewest lanes on this row length
            const int px_opts[4] = {64, 32, 16, 8};
            int best = 64; double best_fill = 0.0;
            for (int px : px_opts) { const double fill = (double)A.nx / (double)(div_up(A.nx, 2 * px) * 2 * px); if (fill > best_fill + 1e-9) { best_fill = fill; best = px; } }
            if (best == 64) hipLaunchKernelGGL((k_mg_residual_restrict_tiled2<64, 2, 2>), dim3(div_up(A.nx, 128), div_up(A.ny, 2), div_up(A.nz, 2)), dim3(256), 0, s, A, b, x, C, bc);
            else if (best == 32) hipLaunchKernelGGL((k_mg_residual_restrict_tiled2<32, 4, 2>), dim3(div_up(A.nx, 64), div_up(A.ny, 4), div_up(A.nz, 2)), dim3(256), 0, s, A, b, x, C, bc);
            else if (best == 16) hipLaunchKernelGGL((k_mg_residual_restrict_tiled2<16, 4, 4>), dim3(div_up(A.nx, 32), div_up(A.ny, 4), div_up(A.nz, 4)), dim3(256), 0, s, A, b, x, C, bc);
            else hipLaunchKernelGGL((k_mg_residual_restrict_tiled2<8, 8, 4>), dim3(div_up(A.nx, 16), div_up(A.ny, 8), div_up(A.nz, 4)), dim3(256), 0, s, A, b, x, C, bc);
        }
        else hipLaunchKernelGGL(k_mg_residual_restrict_tiled, dim3(div_up(A.nx, 64), C.ny, C.nz), dim3(256), 0, s, A, b, x, C, bc);
        FY_LAUNCH_CHECK();
        return FY_OK;
    }
    hipLaunchKernelGGL(k_mg_residual_restrict, dim3(div_up(C.N, 256)), dim3(256), 0, s, A, b, x, C, bc);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_mg_smooth_prolong(hipStream_t s, PMat A, const double* b, const double* x, PMat C, const double* xc, double* xn, double w) {
    if (A.c0 != 0 || A.ntot != A.N) return fail(FY_ERR_INVALID, "k_mg_smooth_prolong works on levels without ghost planes");
    if (pairs_ok(A) && al16(b) && al16(x) && al16(xn)) hipLaunchKernelGGL(k_mg_smooth_prolong2, dim3(div_up(A.N, 512)), dim3(256), 0, s, A, b, x, C, xc, xn, w);
    else hipLaunchKernelGGL(k_mg_smooth_prolong, dim3(div_up(A.N, 256)), dim3(256), 0, s, A, b, x, C, xc, xn, w);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_mg_prolong_add(hipStream_t s, PMat A, double* x, PMat C, const double* xc) {
    hipLaunchKernelGGL(k_mg_prolong_add, dim3(div_up(A.N, 256)), dim3(256), 0, s, A, x, C, xc);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_mg_prolong_add_planes(hipStream_t s, PMat A, int kofs, double* x, PMat C, const double* xc) {
    hipLaunchKernelGGL(k_mg_prolong_add_planes, dim3(div_up(A.N, 256)), dim3(256), 0, s, A, kofs, x, C, xc);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_mg_coarse_solve(hipStream_t s, PMat A, const double* b, double* x, double* tmp, int sweeps, double w, const double* fac) {
    if (A.c0 != 0) return fail(FY_ERR_INVALID, "the coarsest multigrid level must be replicated (no ghost planes)");
    if (A.N > 1024) return fail(FY_ERR_INVALID, "coarsest multigrid level too large (%d cells)", A.N);
    size_t lds = 0;
    if (fac) {
        if (!(mg_coarse_direct_ok)(A)) return fail(FY_ERR_INVALID, "coarse solve: a factor was handed over for a level it cannot belong to");
        static bool attr_set = false;
        if (!attr_set) { FY_TRY(allow_big_lds(reinterpret_cast<const void*>(k_mg_coarse_solve))); attr_set = true; }
        lds = fac_lds_bytes(A.N, band_width(A));
    }
    hipLaunchKernelGGL(k_mg_coarse_solve, dim3(1), dim3(1024), lds, s, A, b, x, tmp, sweeps, w, fac);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_relax_field(hipStream_t s, double* x, const double* prev, double alpha, size_t n) {
    if (n == 0) return FY_OK;
    hipLaunchKernelGGL(k_relax_field, dim3(div_up(n, 256)), dim3(256), 0, s, x, prev, alpha, n);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_copy_f64(hipStream_t s, double* dst, const double* src, size_t n) {
    if (!n) return FY_OK;
    hipLaunchKernelGGL(k_copy, dim3(div_up(n, 256)), dim3(256), 0, s, dst, src, n);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_mg_coarsen_ghost(hipStream_t s, PMat F, PMat C) {
    hipLaunchKernelGGL(k_mg_coarsen_ghost, dim3(div_up((size_t)C.nx * C.ny, 256)), dim3(256), 0, s, F, C);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_add_f64(hipStream_t s, double* y, const double* x, size_t n) {
    if (!n) return FY_OK;
    hipLaunchKernelGGL(k_add, dim3(div_up(n, 256)), dim3(256), 0, s, y, x, n);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

}  // namespace fy
