// Particle half, the forces (the five sources: particle_bin.hip): the cell records the force pass gathers, the Gaussian-mode force with its closures and its
// momentum back-scatter, and the point-force mode.
#include "particle_kernels.hpp"

#include "common.hpp"
#include "device_util.hpp"
#include "scatter_table.hpp"
#include "stencil_ring.hpp"

namespace fy {
namespace {

// ------------------------------------------------------------------------------------------------ force + back-scatter
// What bounded the round-1 force pass was the vector-memory pipeline: 13 eight-byte gathers per (particle, cell) pair out of five
// cell arrays (U, alpha, gradP, divT and -- in the back-scatter loop -- uParticle), 632 M L1 accesses per launch.  Two changes:
//   * the interpolated cell data comes from ONE 64-byte record per cell, CellRec = {U[3], alpha, A[3], V} with
//     A = 2 nu rho_f divT - gradP (the two Archimedes terms of FoamYade.C:416-426 are both interpolated with the same weights, so their
//     per-cell combination is interpolated instead): four 16-byte loads per pair, all from one line, instead of ten 8-byte ones from four;
//   * the drag share of the momentum source, uSource[c] += -coeff w uParticle[c] / rho_f (FoamYade.C:386), has the per-CELL factor
//     uParticle[c]; it is pulled out of the per-pair loop: the pairs only accumulate D[c] = sum -coeff w / rho_f (which is the
//     reference's uSourceDrag contribution, FoamYade.C:385) and k_fold_sources adds D to uSourceDrag and uParticle[c] * D[c] to uSource once
//     per cell -- no uParticle gather per pair.  The Archimedes share -f w / (V rho_f) (FoamYade.C:433) goes into uSource directly.
// Rounding differs from the per-pair form in the last bits only (same terms, summed in another association): covered by the 1e-10 bar.
__global__ __launch_bounds__(256) void k_pack_cells(int64_t n_field, const double* __restrict__ U, const double* __restrict__ alpha,
                                                    const double* __restrict__ gradP, const double* __restrict__ divT,
                                                    const double* __restrict__ vol, double two_nu, double rhoF, double* __restrict__ R) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_field) return;
    const double* u = U + 3 * (size_t)c;
    const double* g = gradP + 3 * (size_t)c;
    const double* d = divT + 3 * (size_t)c;
    const double u0 = u[0], u1 = u[1], u2 = u[2];
    // FoamYade.C:421-426: -gradP w + ((2 nu divT) w) rho_f, per cell
    const double a0 = ((two_nu * d[0]) * rhoF) - g[0], a1 = ((two_nu * d[1]) * rhoF) - g[1], a2 = ((two_nu * d[2]) * rhoF) - g[2];
    double2* r = reinterpret_cast<double2*>(R + kRecDoubles * (size_t)c);
    r[0] = make_double2(u0, u1);
    r[1] = make_double2(u2, alpha[c]);
    r[2] = make_double2(a0, a1);
    r[3] = make_double2(a2, vol[c]);
}

// alpha of the listed cells only (ghost planes after their halo exchange)
__global__ __launch_bounds__(256) void k_patch_rec_alpha(int64_t c0, int64_t n, const double* __restrict__ alpha, double* __restrict__ R) {
    const int64_t c = c0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < c0 + n) R[kRecDoubles * (size_t)c + 3] = alpha[c];
}

// per-particle part of hydroDragForce + archimedesForce (+ the opt-in models) from the interpolated values (FoamYade.C:366-382, 426-427,
// 402-404, 477-478); returns the drag coefficient and the Archimedes (+ added-mass) force whose reaction is scattered, stores F
struct Interp { double ufx, ufy, ufz, alpha_f, pv, sax, say, saz; };
struct ModelSums { double t1, t2, t3, dux, duy, duz, pva; };
struct ParticleForce { double coeff, bx, by, bz; };

// The selectable closures (fy_set_drag_law; DESIGN.md section 3 "force laws"): K = beta / phi, the drag coefficient per unit SOLID volume, with
// eps = alpha_f, phi = max(1 - eps, 0), m = |u_r| and Re = small + m d / nu as in the reference law.  Every beta carries a factor phi, so K is formed
// without a division by phi: the force is pv K u_r and the scattered coefficient K phi.
template <int LAW> __device__ __forceinline__ double drag_K(double eps, double phi, double Re, double m, double dia, double rhoF, double nu) {
    if constexpr (LAW == FY_DRAG_DI_FELICE) {
        const double Re_e = eps * Re, q = 0.63 + 4.8 / sqrt(Re_e), l = 1.5 - log10(Re_e);
        const double chi = 3.7 - 0.65 * exp(-0.5 * (l * l));
        return 0.75 * (q * q) * rhoF * m * pow(eps, 2 - chi) / dia;
    } else if constexpr (LAW == FY_DRAG_KOCH_HILL) {
        const double Re_h = 0.5 * eps * Re;
        double F0;
        if (phi < 0.4) {
            const double plnp = phi > 0 ? phi * log(phi) : 0.0;
            F0 = (1 + 3 * sqrt(phi / 2) + (135.0 / 64.0) * plnp + 16.14 * phi) / (1 + 0.681 * phi - 8.48 * (phi * phi) + 8.16 * ((phi * phi) * phi));
        } else {
            F0 = 10 * phi / ((eps * eps) * eps);
        }
        const double e2 = eps * eps;
        const double F3 = 0.0673 + 0.212 * phi + 0.0232 / ((e2 * e2) * eps);
        return 18 * nu * rhoF * e2 / (dia * dia) * (F0 + 0.5 * F3 * Re_h);
    } else {                                                                          // FY_DRAG_BEETSTRA
        const double Re_e = eps * Re, e2 = eps * eps;
        const double num = 1 / eps + 3 * eps * phi + 8.4 * pow(Re_e, -0.343);
        const double den = 1 + pow(10.0, 3 * phi) * pow(Re_e, -0.5 * (1 + 4 * phi));
        const double Fb = 10 * phi / e2 + e2 * (1 + 1.5 * sqrt(phi)) + (0.413 * Re_e / (24 * e2)) * (num / den);
        return 18 * nu * rhoF * eps / (dia * dia) * Fb;
    }
}

template <int LAW, bool MODELS>
__device__ __forceinline__ ParticleForce force_law(const ForceParams& fp, const Interp& s, const ModelSums& ms, int k, double dia, double lvx, double lvy,
                                                   double lvz, const double* __restrict__ rec_orig, double* __restrict__ F) {
    const double rhoF = fp.rhoF, nu = fp.nu;
    const double alpha_p = 1 - s.alpha_f;                                             // FoamYade.C:366
    const double urx = s.ufx - lvx, ury = s.ufy - lvy, urz = s.ufz - lvz;
    const double magUR = sqrt(urx * urx + ury * ury + urz * urz);
    const double Re = fp.small + ((magUR * dia) / nu);                                // FoamYade.C:370
    double coeff, hfx, hfy, hfz;
    if constexpr (LAW == FY_DRAG_REFERENCE) {
        const double cd = Re < 1000 ? (24 / (Re)) * (1 + (0.15 * pow(Re, 0.687))) : 0.44;
        if (s.alpha_f > 0.8) {                                                        // FoamYade.C:373-374
            coeff = 0.75 * cd * s.alpha_f * alpha_p * rhoF * magUR * pow(s.alpha_f, -2.65);
        } else {                                                                      // FoamYade.C:376-378
            const double cf1 = 150 * ((alpha_p * alpha_p) / s.alpha_f) * ((nu * rhoF) / (dia * dia));
            const double cf2 = 1.75 * alpha_p * rhoF * (1 / dia) * magUR;
            coeff = cf1 + cf2;
        }
        const double s1 = s.pv * coeff, ia = 1 / (alpha_p);                           // FoamYade.C:381
        hfx = (s1 * urx) * ia; hfy = (s1 * ury) * ia; hfz = (s1 * urz) * ia;
    } else {
        const double phi = alpha_p > 0 ? alpha_p : 0.0;
        const double K = drag_K<LAW>(s.alpha_f, phi, Re, magUR, dia, rhoF, nu);
        const double s1 = s.pv * K;
        coeff = K * phi;                                                              // what FoamYade.C:385-386 scatter
        hfx = s1 * urx; hfy = s1 * ury; hfz = s1 * urz;
    }
    const double afx = s.pv * s.sax, afy = s.pv * s.say, afz = s.pv * s.saz;          // FoamYade.C:426
    double fx = (0.0 + hfx) + afx, fy_ = (0.0 + hfy) + afy, fz = (0.0 + hfz) + afz;   // FoamYade.C:382,427
    double tqx = 0.0, tqy = 0.0, tqz = 0.0;                                           // Gaussian torque disabled, FoamYade.C:618
    ParticleForce r{coeff, afx, afy, afz};
    if constexpr (MODELS) {
    if (fp.models & FY_FORCE_GAUSSIAN_TORQUE) {                                       // FoamYade.C:477-478
        const double c3 = M_PI * (pow(dia, 3.0));
        tqx = 0.0 + (((c3 * (ms.t1 - rec_orig[6])) * nu) * rhoF);
        tqy = 0.0 + (((c3 * (ms.t2 - rec_orig[7])) * nu) * rhoF);
        tqz = 0.0 + (((c3 * (ms.t3 - rec_orig[8])) * nu) * rhoF);
    }
    if (fp.models & FY_FORCE_ADDED_MASS) {                                            // FoamYade.C:402-404
        const double pva = ms.pva / (double)(unsigned)k;
        const double amx = (pva * (ms.dux - (lvx / fp.delta_t))) * fp.rhoP;
        const double amy = (pva * (ms.duy - (lvy / fp.delta_t))) * fp.rhoP;
        const double amz = (pva * (ms.duz - (lvz / fp.delta_t))) * fp.rhoP;
        fx = fx + amx; fy_ = fy_ + amy; fz = fz + amz;
        r.bx = r.bx + amx; r.by = r.by + amy; r.bz = r.bz + amz;                      // FoamYade.C:406-411: same -f w / (V rho_f) reaction
    }
    if (fp.models & FY_FORCE_SAFFMAN_MEI_LIFT) {
        // Saffman's shear lift with Mei's finite-Reynolds-number factor on the interpolated vorticity (ms.t = curl U, the torque's gather):
        // Cl = 3 / (2 pi sqrt(Re_w)) 6.46 f(Re_p, Re_w), F = rho_f pv Cl (u_r x omega); `small` keeps both quotients finite at rest and without shear
        const double magW = sqrt(ms.t1 * ms.t1 + ms.t2 * ms.t2 + ms.t3 * ms.t3);
        const double Re_p = (magUR * dia) / nu, Re_w = (magW * (dia * dia)) / nu;
        const double b = 0.5 * Re_w / (Re_p + fp.small), a = 0.3314 * sqrt(b);
        const double f = Re_p < 40 ? (1 - a) * exp(-0.1 * Re_p) + a : 0.0524 * sqrt(b * Re_p);
        const double cl = 3 / (2 * M_PI * sqrt(Re_w + fp.small)) * 6.46 * f;
        const double sl = rhoF * s.pv * cl;
        const double lx = sl * (ury * ms.t3 - urz * ms.t2), ly = sl * (urz * ms.t1 - urx * ms.t3), lz = sl * (urx * ms.t2 - ury * ms.t1);
        fx = fx + lx; fy_ = fy_ + ly; fz = fz + lz;
        r.bx = r.bx + lx; r.by = r.by + ly; r.bz = r.bz + lz;                         // the reaction reaches uSource like Archimedes' and the added mass's
    }
    }
    F[0] = fx; F[1] = fy_; F[2] = fz;
    if (!fp.torque_prezeroed) { F[3] = tqx; F[4] = tqy; F[5] = tqz; }    // permuted 48-byte records: half the store traffic when the torque is identically zero
    return r;
}

__device__ __forceinline__ void interp_add(Interp& s, const double* __restrict__ R, int64_t cl, double w, double volp) {
    const double2* r = reinterpret_cast<const double2*>(R + kRecDoubles * (size_t)cl);
    const double2 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    s.ufx += (r0.x * w); s.ufy += (r0.y * w); s.ufz += (r1.x * w);                    // FoamYade.C:361-365
    s.alpha_f += (r1.y * w);
    s.pv += (volp * w);
    s.sax += (r2.x * w); s.say += (r2.y * w); s.saz += (r3.x * w);                    // FoamYade.C:421-424 (per-cell combination, k_pack_cells)
}

__device__ __forceinline__ void model_add(ModelSums& ms, const ForceParams& fp, const double* __restrict__ vGrad, const double* __restrict__ ddtU, int64_t cl,
                                          double w, double volp) {
    if (fp.models & (FY_FORCE_GAUSSIAN_TORQUE | FY_FORCE_SAFFMAN_MEI_LIFT)) {         // calcHydroTorque FoamYade.C:468-476; the lift reads the same curl
        const double* G = vGrad + 9 * (size_t)cl;                                     // xx xy xz yx yy yz zx zy zz
        ms.t1 += ((G[5] - G[7]) * w); ms.t2 += ((G[6] - G[2]) * w); ms.t3 += ((G[3] - G[1]) * w);
    }
    if (fp.models & FY_FORCE_ADDED_MASS) {                                            // addedMassForce FoamYade.C:396-401
        const double* d = ddtU + 3 * (size_t)cl;
        ms.pva += (volp * w);
        ms.dux = ms.dux + (d[0] * w); ms.duy = ms.duy + (d[1] * w); ms.duz = ms.duz + (d[2] * w);
    }
}

// register budget of k_force_gaussian (a build-time constant; tools/build_variant.sh overrides it for A/B runs): room for 6 waves per SIMD = 80 VGPRs (the
// compiler's own choice is 82: five waves, i.e. TWO 512-thread workgroups per CU; with 80 a third one fits: 1.05 -> 0.93 ms at C3, no spills; 8 waves = 64
// VGPRs spills 68 bytes per lane and is slower again)
#ifndef FY_FORCE_ATTR
#define FY_FORCE_ATTR __attribute__((amdgpu_waves_per_eu(6)))
#endif
// gather + force law + back-scatter in one kernel, one lane per particle (LDS aggregation table per workgroup, flushed to the tile buckets).
// (As two kernels -- gathers without LDS, then the back-scatter -- it measured 1.01 + 1.02 ms against 1.50 fused; timing-only variants of this
// kernel are built from a copy with tools/build_variant.sh, the shipped source carries none.)
#ifndef FY_FORCE_THREADS
#define FY_FORCE_THREADS 512
#endif
#ifndef FY_FORCE_LOG2
#define FY_FORCE_LOG2 10
#endif
constexpr int kForceThreads = FY_FORCE_THREADS, kForceLog2 = FY_FORCE_LOG2;
// One instantiation per (drag law, "any opt-in model on"): the launcher picks, the lane's loops carry no branch on either.  k_force_gaussian<FY_DRAG_REFERENCE>
// is the shipped kernel less the models' cold branch (62 registers where that kernel needed the budget's 80); the opt-in models' gathers and the lift do not fit its 80 registers with every law, so their kernels (k_force_gaussian_models) leave the
// budget to the compiler instead of spilling.
template <int LAW, bool MODELS>
__device__ __forceinline__ void force_gaussian_body(
        ParticleSoA p, int64_t n, const ForceParams& fp, CellWindow cw, const double* __restrict__ vol, const double* __restrict__ R,
        const double* __restrict__ vGrad, const double* __restrict__ ddtU, const double* __restrict__ rec,
        double* __restrict__ drag_acc, double* __restrict__ uSource, double* __restrict__ force_out, const TileBuckets& tb) {
    constexpr int kSlots = 1 << kForceLog2;
    __shared__ uint32_t keys[kSlots];
    __shared__ double vals[kSlots * 4];
    __shared__ TileMapLds tmap;
    table_clear<kSlots, kForceThreads, 4>(keys, vals);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kForceThreads + threadIdx.x;
    if (i < n) {
        const StencilSpan sp = stencil_span(p.chain_len[i]);      // the loops below walk it oldest first (stencil_ring.hpp)
        const int k = sp.k, first = sp.first;
        ParticleForce pf{0.0, 0.0, 0.0, 0.0};
        const int32_t orig = p.orig[i];
        double* F = force_out + 6 * (size_t)orig;
        if (k == 0) {                                   // zeros for particles nobody located (FoamYade.C:142)
            F[0] = F[1] = F[2] = 0.0;
            if (!fp.torque_prezeroed) { F[3] = F[4] = F[5] = 0.0; }
        } else {
            const double dia = 2 * p.rad[i];
            const double volp = M_PI * cube3(dia) / 6.0;
            // hydroDragForce FoamYade.C:358-365 and archimedesForce FoamYade.C:416-424 share one gather pass over the cell records
            Interp s{0, 0, 0, 0, 0, 0, 0, 0};
            ModelSums ms{0, 0, 0, 0, 0, 0, 0};
            {
                // the next entry's id and weight are fetched while this entry's record gathers are in flight: one memory round trip per entry instead of
                // two dependent ones (id -> record); same operations in the same order (round 5: 1.11 -> 1.03 ms).  One stage deeper -- the NEXT entry's
                // record gathers in flight as well -- was measured too and loses (1.15 ms): not used
                size_t slot = stencil_slot(p, i, first);
                int32_t id_n = p.ids[slot];
                double w_n = p.w[slot];
                for (int t = 0; t < k; ++t) {
                    const int64_t cl = (int64_t)id_n - cw.base;
                    const double w = w_n;
                    if (t + 1 < k) {
                        slot = stencil_slot(p, i, first + t + 1);
                        id_n = p.ids[slot]; w_n = p.w[slot];
                    }
                    if (cl < 0 || cl >= cw.n_field) continue;
                    interp_add(s, R, cl, w, volp);
                }
            }
            if constexpr (MODELS)                       // off in the shipped reference
                for (int t = 0; t < k; ++t) {
                    const size_t slot = stencil_slot(p, i, first + t);
                    const int64_t cl = (int64_t)p.ids[slot] - cw.base;
                    if (cl < 0 || cl >= cw.n_field) continue;
                    model_add(ms, fp, vGrad, ddtU, cl, p.w[slot], volp);
                }
            pf = force_law<LAW, MODELS>(fp, s, ms, k, dia, p.vx[i], p.vy[i], p.vz[i], rec + 10 * (size_t)orig, F);
            const double irho = 1 / fp.rhoF;
            // a uniform block's cell volume is a constant, not a gather
            const double ooUniform = fp.uniform_vol > 0 ? 1. / (fp.uniform_vol * fp.rhoF) : 0.0;
            size_t slot_b = stencil_slot(p, i, first);
            int32_t idb_n = p.ids[slot_b];
            double wb_n = p.w[slot_b];
            for (int t = 0; t < k; ++t) {
                const int64_t cl = (int64_t)idb_n - cw.base;
                const double w = wb_n;
                if (t + 1 < k) {                         // (prefetched as in the gather loop)
                    slot_b = stencil_slot(p, i, first + t + 1);
                    idb_n = p.ids[slot_b]; wb_n = p.w[slot_b];
                }
                if (cl < 0 || cl >= cw.n_field) continue;
                const int32_t c = (int32_t)cl;
                const double ooCellVol = fp.uniform_vol > 0 ? ooUniform : 1. / (vol[c] * fp.rhoF);  // FoamYade.C:432
                const double c0 = (-pf.coeff * w) * irho;                                      // FoamYade.C:385 (and, times uParticle[c], :386)
                const double c1 = (-pf.bx * w) * ooCellVol, c2 = (-pf.by * w) * ooCellVol, c3 = (-pf.bz * w) * ooCellVol;   // FoamYade.C:433, 406-411
                const int h = agg_slot<kForceLog2>(keys, (uint32_t)c);
                if (h >= 0) {
                    lds_add_f64(&vals[agg_at<kSlots>(h, 0)], c0); lds_add_f64(&vals[agg_at<kSlots>(h, 1)], c1);
                    lds_add_f64(&vals[agg_at<kSlots>(h, 2)], c2); lds_add_f64(&vals[agg_at<kSlots>(h, 3)], c3);
                } else {
                    atomic_add_f64(&drag_acc[c], c0);
                    atomic_add_f64(&uSource[3 * (size_t)c + 0], c1);
                    atomic_add_f64(&uSource[3 * (size_t)c + 1], c2);
                    atomic_add_f64(&uSource[3 * (size_t)c + 2], c3);
                }
            }
        }
    }
    __syncthreads();
    flush_table<kSlots, kForceThreads, 4>(keys, vals, tmap, tb, drag_acc, uSource, nullptr);
}

template <int LAW>
__global__ __launch_bounds__(kForceThreads) FY_FORCE_ATTR void k_force_gaussian(
        ParticleSoA p, int64_t n, ForceParams fp, CellWindow cw, const double* __restrict__ vol, const double* __restrict__ R,
        const double* __restrict__ vGrad, const double* __restrict__ ddtU, const double* __restrict__ rec,
        double* __restrict__ drag_acc, double* __restrict__ uSource, double* __restrict__ force_out, TileBuckets tb) {
    force_gaussian_body<LAW, false>(p, n, fp, cw, vol, R, vGrad, ddtU, rec, drag_acc, uSource, force_out, tb);
}
template <int LAW>
__global__ __launch_bounds__(kForceThreads) void k_force_gaussian_models(
        ParticleSoA p, int64_t n, ForceParams fp, CellWindow cw, const double* __restrict__ vol, const double* __restrict__ R,
        const double* __restrict__ vGrad, const double* __restrict__ ddtU, const double* __restrict__ rec,
        double* __restrict__ drag_acc, double* __restrict__ uSource, double* __restrict__ force_out, TileBuckets tb) {
    force_gaussian_body<LAW, true>(p, n, fp, cw, vol, R, vGrad, ddtU, rec, drag_acc, uSource, force_out, tb);
}

// ------------------------------------------------------------------------------------------------ point force
// index q with f[q] <= x < f[q + 1] by bisection over the n + 1 face planes of one axis (x inside [f[0], f[n]] is the caller's business)
__device__ __forceinline__ int axis_cell(const double* __restrict__ f, int n, double x) {
    int lo = 0, hi = n;                        // invariant: f[lo] <= x, and x < f[hi] or hi == n
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (f[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}
// SCHILLER_NAUMANN = false: the reference's Stokes drag; true: the same with the finite-Reynolds-number factor f (fy_set_drag_law)
template <bool SCHILLER_NAUMANN>
__global__ __launch_bounds__(256) void k_point_force(const double* __restrict__ rec, int64_t n, BlockGeom g, ForceParams fp, CellWindow cw,
                                                     const double* __restrict__ vol, const double* __restrict__ U,
                                                     const double* __restrict__ vGrad, double* __restrict__ uSource,
                                                     double* __restrict__ force_out, int32_t* __restrict__ found_out,
                                                     int32_t* __restrict__ incell_out, SlabOwn own) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* r = rec + 10 * i;
    const double x = r[0], y = r[1], z = r[2];
    double* F = force_out + 6 * (size_t)i;
    int cglob;
    if (g.cell_of) {
        // general mesh: mesh.findCell (FoamYade.C:251) was answered by the nearest centre + a walk to the cell whose face-fan tetrahedra hold the point (k_ldu_find_cell)
        cglob = g.cell_of[i];
        if (cglob < 0) {
            F[0] = F[1] = F[2] = F[3] = F[4] = F[5] = 0.0;
            found_out[i] = -1;
            incell_out[i] = -1;
            return;
        }
    } else {
        // uniform-block stand-in for mesh.findCell (FoamYade.C:251): inside the closed bounding box, floor((p-min)/dx) clamped
        const bool outside = (x < g.bbmin[0] || y < g.bbmin[1] || z < g.bbmin[2] || x > g.bbmax[0] || y > g.bbmax[1] || z > g.bbmax[2]);
        if (outside || !(x == x) || !(y == y) || !(z == z)) {
            F[0] = F[1] = F[2] = F[3] = F[4] = F[5] = 0.0;
            found_out[i] = -1;
            incell_out[i] = -1;
            return;
        }
        int ci, cj, ck;
        if (g.faces[0]) {              // graded block: the cell whose [low, high) face planes hold the coordinate (the last cell takes its high plane too)
            ci = axis_cell(g.faces[0], g.nx, x); cj = axis_cell(g.faces[1], g.ny, y); ck = axis_cell(g.faces[2], g.nz, z);
        } else {
            ci = min(g.nx - 1, (int)((x - g.bbmin[0]) / g.dx));
            cj = min(g.ny - 1, (int)((y - g.bbmin[1]) / g.dx));
            ck = min(g.nz - 1, (int)((z - g.bbmin[2]) / g.dx));
        }
        if (own.active && !own_planes(own, (int)i, ck, x, y, z)) {           // in another slab's (or wire piece's) planes: that one owns it
            F[0] = F[1] = F[2] = F[3] = F[4] = F[5] = 0.0;
            found_out[i] = -1;
            incell_out[i] = -1;
            return;
        }
        cglob = ci + g.nx * (cj + g.ny * ck);
    }
    found_out[i] = 1;
    incell_out[i] = cglob;
    const int64_t cl = (int64_t)cglob - cw.base;
    if (cl < 0 || cl >= cw.n_field) { F[0] = F[1] = F[2] = F[3] = F[4] = F[5] = 0.0; return; }   // not in this slab's window
    const int c = (int)cl;
    const double dia = 2 * r[9];
    const double rhoF = fp.rhoF, nu = fp.nu;
    // stokesDragForce FoamYade.C:437-444
    double coeff = 3 * M_PI * (dia)*nu * rhoF;
    const double ooCellVol = 1. / (vol[c] * rhoF);
    const double* u = U + 3 * (size_t)c;
    if constexpr (SCHILLER_NAUMANN) {
        const double urx = u[0] - r[3], ury = u[1] - r[4], urz = u[2] - r[5];
        const double Re = fp.small + ((sqrt(urx * urx + ury * ury + urz * urz) * dia) / nu);
        coeff = coeff * (Re < 1000 ? 1 + 0.15 * pow(Re, 0.687) : 0.44 * Re / 24);
    }
    const double hx = coeff * (u[0] - r[3]), hy = coeff * (u[1] - r[4]), hz = coeff * (u[2] - r[5]);
    const double m = -1 * ooCellVol;
    atomic_add_f64(&uSource[3 * (size_t)c + 0], m * hx);
    atomic_add_f64(&uSource[3 * (size_t)c + 1], m * hy);
    atomic_add_f64(&uSource[3 * (size_t)c + 2], m * hz);
    F[0] = hx; F[1] = hy; F[2] = hz;
    // stokesDragTorque FoamYade.C:446-453: wfluid = (zy - yz, zx - xz, yx - xy)
    const double* G = vGrad + 9 * (size_t)c;
    const double s1 = G[7] - G[5], s2 = G[6] - G[2], s3 = G[3] - G[1];
    const double pd3 = M_PI * (pow(dia, 3.0));
    F[3] = ((pd3 * (s1 - r[6])) * nu) * rhoF;
    F[4] = ((pd3 * (s2 - r[7])) * nu) * rhoF;
    F[5] = ((pd3 * (s3 - r[8])) * nu) * rhoF;
}

// setSourceZero FoamYade.C:556-564
__global__ __launch_bounds__(256) void k_set_source_zero(int32_t n_cells, int gaussian, double* __restrict__ uSourceDrag,
                                                         double* __restrict__ alpha, double* __restrict__ uSource,
                                                         double* __restrict__ uParticle) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cells) return;
    double* s = uSource + 3 * (size_t)c;
    s[0] = 0.0; s[1] = 0.0; s[2] = 0.0;
    if (gaussian) {
        alpha[c] = 1.0;
        uSourceDrag[c] = 0.0;
        double* u = uParticle + 3 * (size_t)c;
        u[0] = 0.0; u[1] = 0.0; u[2] = 0.0;
    }
}

}  // namespace

int launch_pack_cells(hipStream_t s, int64_t n_field, const double* U, const double* alpha, const double* gradP, const double* divT, const double* vol,
                      double nu, double rhoF, double* R) {
    return launch_n(s, k_pack_cells, n_field, 256, n_field, U, alpha, gradP, divT, vol, 2.0 * nu, rhoF, R);
}

int launch_patch_rec_alpha(hipStream_t s, int64_t c0, int64_t n, const double* alpha, double* R) { return launch_n(s, k_patch_rec_alpha, n, 256, c0, n, alpha, R); }

int launch_force_gaussian(hipStream_t s, ParticleSoA p, int64_t n, ForceParams fp, CellWindow cw, const double* vol, const double* R,
                          const double* vGrad, const double* ddtU, const double* rec, double* drag_acc, double* uSource,
                          double* force_out, TileBuckets tb) {
    if (n <= 0) return FY_OK;
    using Kernel = void (*)(ParticleSoA, int64_t, ForceParams, CellWindow, const double*, const double*, const double*, const double*, const double*, double*, double*, double*,
                            TileBuckets);
    static const Kernel table[4][2] = {{k_force_gaussian<FY_DRAG_REFERENCE>, k_force_gaussian_models<FY_DRAG_REFERENCE>},
                                       {k_force_gaussian<FY_DRAG_DI_FELICE>, k_force_gaussian_models<FY_DRAG_DI_FELICE>},
                                       {k_force_gaussian<FY_DRAG_KOCH_HILL>, k_force_gaussian_models<FY_DRAG_KOCH_HILL>},
                                       {k_force_gaussian<FY_DRAG_BEETSTRA>, k_force_gaussian_models<FY_DRAG_BEETSTRA>}};
    if (fp.drag_law < FY_DRAG_REFERENCE || fp.drag_law > FY_DRAG_BEETSTRA) return fail(FY_ERR_INVALID, "launch_force_gaussian: drag law %d has no Gaussian-mode kernel", fp.drag_law);
    hipLaunchKernelGGL(table[fp.drag_law][fp.models ? 1 : 0], dim3(div_up(n, kForceThreads)), dim3(kForceThreads), 0, s, p, n, fp, cw, vol, R, vGrad, ddtU, rec, drag_acc,
                       uSource, force_out, tb);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

int launch_point_force(hipStream_t s, const double* rec, int64_t n, BlockGeom g, ForceParams fp, CellWindow cw, const double* vol,
                       const double* U, const double* vGrad, double* uSource, double* force_out, int32_t* found_out,
                       int32_t* incell_out, SlabOwn own) {
    if (n <= 0) return FY_OK;
    if (fp.drag_law != FY_DRAG_REFERENCE && fp.drag_law != FY_DRAG_SCHILLER_NAUMANN) return fail(FY_ERR_INVALID, "launch_point_force: drag law %d has no point-mode kernel", fp.drag_law);
    return launch_n(s, fp.drag_law == FY_DRAG_SCHILLER_NAUMANN ? k_point_force<true> : k_point_force<false>, n, 256, rec, n, g, fp, cw, vol, U, vGrad, uSource, force_out,
                    found_out, incell_out, own);
}

int launch_set_source_zero(hipStream_t s, int32_t n_cells, int gaussian, double* uSourceDrag, double* alpha, double* uSource,
                           double* uParticle) {
    hipLaunchKernelGGL(k_set_source_zero, dim3(div_up(n_cells, 256)), dim3(256), 0, s, n_cells, gaussian, uSourceDrag, alpha, uSource, uParticle);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

}  // namespace fy
