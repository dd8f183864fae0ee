// fy_ldu_solver: the time-loop body of icoFoamYade (icoFoamYade/icoFoamYade.C:65-149) on a general polyhedral mesh (ldu.hpp), sequencing the
// kernels of ldu_kernels.hip, with the coupling engine (fy_ctx, point force) sharing the device fields and the stream.  Control flow follows the
// reference line by line; the pressure solver is PCG.C's loop [OF-6] in the single-reduction form of fv_pressure.cpp with the diagonal
// preconditioner, the momentum predictor Jacobi sweeps with lduMatrix::solver's residual control (the stand-in for smoothSolver, as in fv_solver.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "coupling.hpp"
#include "field_average.hpp"
#include "fv_kernels.hpp"
#include "fv_linalg_kernels.hpp"
#include "heat_exchange.hpp"
#include "inlets.hpp"
#include "solid_stats.hpp"
#include "ldu.hpp"
#include "ldu_amg.hpp"
#include "open_boundary.hpp"

namespace fy {

struct LduSolver {
    LduHostMesh hm;
    fy_ldu_case cs{};
    LduGeo g{};
    int device = 0;
    hipStream_t stream = nullptr, side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_fields = nullptr;
    fy_ctx* cpl = nullptr;
    int nc = 0, nf = 0, ni = 0;
    // geometry + addressing on the device
    DevBuf<int32_t> d_own, d_nei, d_patch_of, d_cf_off, d_cf_face, d_ubc, d_pbc, d_ef, d_en;
    DevBuf<double> d_Cf, d_Sf, d_magSf, d_C, d_V, d_w, d_dcNO, d_kvec, d_uval, d_pval, d_recon;
    // mesh.findCell's tetrahedra (point-force mode only): points, the faces' point lists, the cells' balls
    DevBuf<int32_t> d_fp_off, d_fp_pts, d_bin_off, d_bin_cell;
    DevBuf<double> d_pts, d_cell_r2;
    LduFans fans{};
    // fields
    DevBuf<double> U, Uold, p, phi, phiOld, uSource, uSourceExt, uSourceSum, vGrad, gradp, dummy3, dummy1;
    DevBuf<double> mdiag, mlower, mupper, mb, fcorr, xscr, rAU, HbyA, rAUf, phiHbyA, pcoef, pcorr, pdiag, prhs, pr, pu, pw, pp, ps;
    DevBuf<double> partials, sc, xsum, adj;
    // pimpleFoamYade: the coupling's fields and the alpha-weighted equations' face fields
    bool pimple = false, hold_sources = false, sources_pending = false;
    DevBuf<double> alpha, alphaf, uSourceDrag, uParticle, gradP, divT, ddtU, fstress, phiForces, psn, arAUf, phiA, ssf, bmom, pPrev;
    DevBuf<double> nut, d_nutval, gradL;
    DevBuf<int32_t> d_nutbc;
    bool les = false;
    bool keqn = false, nut_live = false;
    long long k_iters_total = 0;
    bool keps = false;
    DevBuf<double> kturb, d_kval, gradk, epsturb, d_epsval;
    DevBuf<int32_t> d_kbc, d_epsbc;
    // wall functions: nearWallDist per boundary face (host: ywall, zeros without a wall-function patch), the epsilonWallFunction cells (LduWallCells) and what
    // k_ldu_wall_functions forms for them once per correct(); nutBnd: the "nut_boundary" read-out
    std::vector<double> ywall;
    DevBuf<double> d_ywall, wall_eps, wall_G, nutBnd;
    DevBuf<int32_t> d_wc_cell, d_wc_off, d_wc_face, d_wall_of;
    int n_wall_cells = 0;
    double wf_yplam = 0.0;
    LduWallCells WC() const { return LduWallCells{n_wall_cells, d_wc_cell.p, d_wc_off.p, d_wc_face.p, std::pow(cs.ras_cmu, 0.75)}; }
    // heat exchange (fy_ldu_case.thermal; DESIGN.md section 3 "heat exchange", DESIGN_FV.md "T equation"): the fluid's T with its sources and per-patch conditions, the
    // Gauss gradient of T_old for the explicit non-orthogonal part, the buoyancy a and uSource + a (what the momentum equations then read in uSource's place), and the
    // particles' half, which fy_solver holds too.  Off: nothing allocated, nothing launched
    struct Thermal {
        bool on = false, buoyant = false;
        fy_thermal_desc d{};
        LduTEqn eq{};
        DevBuf<double> T, Sp, Su, gradT, buoy, usrc_sum, d_val;
        DevBuf<int32_t> d_bc;
        HeatExchange part;
        int iters = 0;
        double res0 = 0.0;
    } th;
    LduPim P() const {
        return LduPim{alpha.p, alpha.p, alphaf.p, uSourceDrag.p, th.buoyant ? th.usrc_sum.p : uSource.p, {cs.g[0], cs.g[1], cs.g[2]}, les ? nut.p : nullptr, d_nutbc.p, d_nutval.p,
                      (keqn || keps) ? kturb.p : nullptr, d_kbc.p, d_kval.p, nut_live ? 1 : 0, cs.les_ck, cs.les_delta_coeff,
                      keps ? epsturb.p : nullptr, d_epsbc.p, d_epsval.p, cs.ras_cmu,
                      d_ywall.p, std::pow(cs.ras_cmu, 0.25), cs.wf_kappa, cs.wf_E, wf_yplam};
    }      // alphac.oldTime() == alphac
    DevBuf<int> adj_err;
    bool need_ref = true, ext_source = false, has_slip = false;
    std::vector<double> orig_face_d;      // hm.orig_face as doubles (the field read-out's type); empty without a cyclic pair
    DevBuf<double> d_gB, d_gG0, d_rT;      // the per-slot coefficients of the scalar gradient and of fvc::reconstruct (LduGeo)
    DevBuf<double> pt;           // per face: -phiHbyA + the corrected laplacian's explicit flux (what the pressure equation's cell part sums)
    DevBuf<double> d_sep;        // folded cyclic faces: the neighbour image's offset per internal face
    DevBuf<double> mbdiag;       // symmetry patches: the momentum matrix's per-component boundary diagonal
    LduAmg amg;                  // the pressure matrix in ELL form; with p_solver = FY_PSOLVER_PCG_MG also the agglomeration hierarchy
    fy_step_stats st{};
    double cumulative = 0.0, total_volume = 0.0;
    EventTimer tim[2];
    // fieldAverage (field_average.hpp), sampled where runTime.write() stands: after the last corrector and the turbulence correction, before setSourceZero
    FieldAverage avg;
    const double* avg_source(const std::string& name, int* comp) const {      // the field as it lies NOW (U and its scratch buffer trade places)
        const struct { const char* nm; const double* p; int comp; bool have; } tab[] = {
            {"U", U.p, 3, true}, {"p", p.p, 1, true}, {"alpha", alpha.p, 1, pimple}, {"uParticle", uParticle.p, 3, pimple}, {"uSource", uSource.p, 3, true},
            {"nut", nut.p, 1, les}, {"k", kturb.p, 1, keqn || keps}, {"epsilon", epsturb.p, 1, keps}, {"T", th.T.p, 1, th.on}};
        for (const auto& e : tab)
            if (name == e.nm && e.have && e.p) { *comp = e.comp; return e.p; }
        return ss.source(name, comp);
    }
    // solid-phase statistics (solid_stats.hpp), formed once per step after the T equation's pass B and before fieldAverage and the monitors sample; a general mesh has
    // no tiles, so the Gaussian scatter's table flushes as global atomics
    SolidStats ss;
    int set_solid_statistics(int on) {
        FY_HIP(hipSetDevice(device));
        ss.who = "fy_ldu_solver";
        return ss.set(on != 0, (size_t)nc, th.on, stream);
    }
    int set_field_average(const fy_average_desc* d) {
        FY_HIP(hipSetDevice(device));
        return avg.configure(d, (size_t)nc, stream, "fy_ldu_solver_set_field_average", [this](const std::string& nm, int* comp) { return avg_source(nm, comp); });
    }
    // run-time monitors (monitors.hpp), sampled where fieldAverage is; the boundary read-outs "p_boundary" / "U_boundary" / "T_boundary", formed on request
    Monitors mon;
    DevBuf<double> bndP, bndU, bndT;
    int set_monitors(const fy_monitor_desc* d) {
        FY_HIP(hipSetDevice(device));
        return mon.configure(d, (size_t)nc, (size_t)(nf - ni), th.on, stream, "fy_ldu_solver_set_monitors", [this](const std::string& nm, int* comp) { return avg_source(nm, comp); },
                             [this](int pa, std::string* why) {
                                 if (pa < 0 || pa >= hm.nPatches) { *why = "patch " + std::to_string(pa) + " does not exist (the mesh has " + std::to_string(hm.nPatches) + ")"; return 0; }
                                 if (hm.psize[(size_t)pa] == 0) *why = "patch " + std::to_string(pa) + " has no faces (a cyclic patch is folded into internal faces)";
                                 return (int)hm.psize[(size_t)pa];
                             });
    }

    // wall loads (wall_loads.hpp), sampled where the monitors are.  A patch set is a list of patch indices; nearWallDist (ywall) is then formed for the selected patches
    // as well as for the wall-function patches (wf_on: what setup_wall_functions switched on)
    WallLoads wl;
    std::vector<char> wf_on;
    int set_wall_loads(const fy_wall_loads_desc* d) {
        FY_HIP(hipSetDevice(device));
        std::vector<char> sel = wf_on;
        sel.resize((size_t)hm.nPatches, 0);
        FY_TRY(wl.configure(d, (size_t)(nf - ni), cs.nu > 0 || les, stream, "fy_ldu_solver_set_wall_loads",
                            [this](const fy_wall_patch_set& set, const char* on, int* patches, int* np, std::vector<std::string>* names) {
                                const char* who = "fy_ldu_solver_set_wall_loads";
                                if (set.n_patches == 0) return fail(FY_ERR_INVALID, "%s: object '%s': the patch set is empty (patches)", who, on);
                                if (set.n_patches < 0 || set.n_patches > FY_WALL_LOADS_MAX_PATCHES)
                                    return fail(FY_ERR_INVALID, "%s: object '%s': %d patches (1 to FY_WALL_LOADS_MAX_PATCHES = %d)", who, on, set.n_patches, FY_WALL_LOADS_MAX_PATCHES);
                                for (int q = 0; q < set.n_patches; ++q) {
                                    const int pa = set.patches[q];
                                    if (pa < 0 || pa >= hm.nPatches) return fail(FY_ERR_INVALID, "%s: object '%s': patch %d does not exist (the mesh has %d)", who, on, pa, hm.nPatches);
                                    if (hm.psize[(size_t)pa] == 0) return fail(FY_ERR_INVALID, "%s: object '%s': patch %d is a cyclic patch or has no faces (a cyclic patch is folded into internal faces)", who, on, pa);
                                    for (int r = 0; r < q; ++r) if (set.patches[r] == pa) return fail(FY_ERR_INVALID, "%s: object '%s': patch %d is listed twice", who, on, pa);
                                    patches[q] = pa; names->push_back("patch" + std::to_string(pa));
                                }
                                *np = set.n_patches;
                                return (int)FY_OK;
                            }));
        for (int q = 0; q < wl.tab.n; ++q)                                    // yPlus reads y on its patches
            if (wl.tab.o[q].kind == WL_YPLUS) for (int r = 0; r < wl.tab.o[q].np; ++r) sel[(size_t)wl.tab.o[q].patch[r]] = 1;
        // nearWallDist follows from the CURRENT configuration alone: the wall-function patches plus the yPlus object's, whatever was configured before
        std::vector<char> now_on((size_t)hm.nPatches, 0);
        for (size_t b = 0; b < ywall.size(); ++b) if (ywall[b] != 0.0) now_on[(size_t)hm.patch_of[b]] = 1;
        if (sel != now_on) {                                        // (the wall-function patches' distances come out as they were: the same statement on the same data)
            FY_HIP(hipStreamSynchronize(stream));
            hm.near_wall_dist(sel, &ywall);
            FY_TRY(up(d_ywall, ywall));
        }
        return FY_OK;
    }

    // porous zones (porous.hpp; DESIGN.md section 3 "Porous zones"): the two momentum assemblies read por.dev() (null: none); a solver with a zone holds mbdiag as one
    // with a symmetry patch does (allocated for the zones alone without one, freed with them).  Off: nothing allocated, nothing launched
    Porous por;
    int set_porous_zones(const fy_porous_desc* d) {
        FY_HIP(hipSetDevice(device));
        // (the per-component diagonal first: a call that fails, here or in configure, leaves the solver as it was)
        bool fresh = false;
        if (d && d->n_zones != 0 && !mbdiag.p) { FY_TRY(mbdiag.alloc_exact(3 * (size_t)nc)); fresh = true; const int zrc = zero(mbdiag); if (zrc != FY_OK) { mbdiag.release(); return zrc; } }
        const int rc = por.configure(d, nc, stream, "fy_ldu_solver_set_porous_zones", [this](int c) { return hm.V[(size_t)c]; });
        if (rc != FY_OK) { if (fresh) { FY_HIP(hipStreamSynchronize(stream)); mbdiag.release(); } return rc; }
        if (!por.on() && !has_slip) mbdiag.release();
        return FY_OK;
    }
    int porous_stats(int32_t* nz, int64_t* cnt, double* volume, double* void_volume, double* force) {
        FY_HIP(hipSetDevice(device));
        return por.stats(stream, "fy_ldu_solver_get_porous_stats", g.nu, U.p, pimple ? alpha.p : nullptr, nz, cnt, volume, void_volume, force);
    }

    // flow-rate control (fy_flow_control_desc; ldu_flow_control.hip; DESIGN.md section 3 "Flow-rate control").  Off: nothing allocated, nothing launched.  The host
    // keeps no value of the state: `cur` says which of the two records the step reads now, and flips at each momentum assembly
    struct Flow {
        bool on = false;
        fy_flow_control_desc d{};
        double dir[3] = {0, 0, 0}, mag = 0.0;
        DevBuf<double> st, sums, usrc;         // [2][FLOW_RECORD], the two folded sums, the effective external source [3 nc]
        DevBuf<unsigned long long> count;
        int cur = 0;
        KernelClock clock;
        double* rec(int which) { return st.p + (size_t)which * FLOW_RECORD; }
    } fc;
    int set_flow_control(const fy_flow_control_desc* d, const char* who) {
        if (d && d->on) {
            const double m2 = d->ubar[0] * d->ubar[0] + d->ubar[1] * d->ubar[1] + d->ubar[2] * d->ubar[2];
            if (!std::isfinite(m2) || !(m2 > 0)) return fail(FY_ERR_INVALID, "%s: flow_control.ubar must be finite with |ubar| > 0", who);
            if (!std::isfinite(d->relaxation) || d->relaxation < 0 || d->relaxation > 1) return fail(FY_ERR_INVALID, "%s: flow_control.relaxation %g must lie in [0, 1]", who, d->relaxation);
            if (!std::isfinite(d->gradient0)) return fail(FY_ERR_INVALID, "%s: flow_control.gradient0 must be finite", who);
            if (d->superficial && !pimple) return fail(FY_ERR_INVALID, "%s: flow_control.superficial needs pimpleFoamYade (icoFoamYade has no void fraction)", who);
        }
        FY_HIP(hipSetDevice(device));
        FY_HIP(hipStreamSynchronize(stream));
        if (!d || !d->on) {
            fc.on = false; fc.d = fy_flow_control_desc{};
            fc.st.release(); fc.sums.release(); fc.usrc.release(); fc.count.release();
            fc.clock.reset();
            return FY_OK;
        }
        fc.d = *d;
        fc.mag = std::sqrt(d->ubar[0] * d->ubar[0] + d->ubar[1] * d->ubar[1] + d->ubar[2] * d->ubar[2]);
        for (int a = 0; a < 3; ++a) fc.dir[a] = d->ubar[a] / fc.mag;
        if (!fc.st.p) {
            FY_TRY(fc.st.alloc_exact(2 * FLOW_RECORD)); FY_TRY(fc.sums.alloc_exact(2)); FY_TRY(fc.usrc.alloc_exact(3 * (size_t)nc)); FY_TRY(fc.count.alloc_exact(1));
        }
        const double h[2 * FLOW_RECORD] = {d->gradient0, 0, 0, 0, d->gradient0, 0, 0, 0};
        FY_HIP(hipMemcpyAsync(fc.st.p, h, sizeof(h), hipMemcpyHostToDevice, stream));
        FY_HIP(hipMemsetAsync(fc.sums.p, 0, 2 * sizeof(double), stream));
        FY_HIP(hipMemsetAsync(fc.count.p, 0, sizeof(unsigned long long), stream));
        FY_HIP(hipStreamSynchronize(stream));                  // (set-up only: h dies with this scope)
        fc.cur = 0;
        fc.clock.per_collect = (size_t)1 << 20;                // every launch is timed and counted while timing is on: the count is the launch budget's check
        fc.clock.on = ss.clock.on;
        fc.on = true;
        return FY_OK;
    }
    // constrain + addSup at a momentum assembly: the state's update and the effective external source, what the equations then read where they read uSourceExt
    // (increment_into: a later PIMPLE outer iteration, whose uSource already holds the source of the assembly before -- it gains flowDir times the last dGradP)
    int flow_source(double* increment_into = nullptr) {
        fc.clock.begin(stream);
        FY_TRY(launch_ldu_flow_source(stream, nc, fc.rec(fc.cur), fc.rec(1 - fc.cur), ext_source ? uSourceExt.p : nullptr, fc.dir, increment_into != nullptr,
                                      increment_into ? increment_into : fc.usrc.p));
        fc.clock.end(stream);
        fc.cur = 1 - fc.cur;
        return FY_OK;
    }
    // correct(U) after a corrector's velocity update: two sums, their fold, the correction
    int flow_correct() {
        fc.clock.begin(stream);
        FY_TRY(launch_ldu_flow_sums(stream, nc, U.p, rAU.p, d_V.p, fc.d.superficial ? alpha.p : nullptr, fc.dir, partials.p));
        fc.clock.end(stream);
        fc.clock.begin(stream);
        FY_TRY(launch_reduce_finalize(stream, partials.p, nc, 2, nullptr, fc.sums.p, nullptr, 0));
        fc.clock.end(stream);
        fc.clock.begin(stream);
        FY_TRY(launch_ldu_flow_apply(stream, nc, fc.sums.p, fc.rec(fc.cur), fc.count.p, fc.mag, fc.d.relaxation, total_volume, fc.dir, rAU.p, U.p));
        fc.clock.end(stream);
        return FY_OK;
    }
    int get_flow_control(double* gradient, double* ubar_unc, double* rau_ave, double* dgradp, int64_t* corrections) {
        if (!fc.on) return fail(FY_ERR_INVALID, "fy_ldu_solver_get_flow_control: flow control is off (fy_ldu_case.flow_control, fy_ldu_solver_set_flow_control)");
        FY_HIP(hipSetDevice(device));
        double h[FLOW_RECORD];
        unsigned long long n = 0;
        FY_HIP(hipMemcpyAsync(h, fc.rec(fc.cur), sizeof(h), hipMemcpyDeviceToHost, stream));
        FY_HIP(hipMemcpyAsync(&n, fc.count.p, sizeof(n), hipMemcpyDeviceToHost, stream));
        FY_HIP(hipStreamSynchronize(stream));
        if (gradient) *gradient = h[FLOW_GRADP0] + h[FLOW_DGRADP];
        if (ubar_unc) *ubar_unc = h[FLOW_UBAR];
        if (rau_ave) *rau_ave = h[FLOW_RAUAVE];
        if (dgradp) *dgradp = h[FLOW_DGRADP];
        if (corrections) *corrections = (int64_t)n;
        return FY_OK;
    }

    // inlets (inlets.hpp; DESIGN.md section 3 "Inlets").  Off: nothing allocated, nothing launched, g.u_face null.  uFace [nb][3] holds the value of every face of an
    // inlet patch (the other faces' entries are never read); dInlet flags the inlet patches
    Inlets inl;
    DevBuf<double> uFace;
    DevBuf<int32_t> dInlet;
    bool stepped = false;
    std::vector<int32_t> h_ubc;               // the patches' velocity conditions as the solver was created with them
    int set_inlets(const fy_inlets_desc* d, const char* who) {
        if (stepped) return fail(FY_ERR_INVALID, "%s: the solver has stepped already; inlets are set at create or before the first step", who);
        FY_HIP(hipSetDevice(device));
        if ((!d || d->n == 0) && !inl.on()) return FY_OK;                   // nothing to set and nothing was set
        FY_HIP(hipStreamSynchronize(stream));
        Inlets fresh;
        FY_TRY(fresh.configure(d, stream, who, [this, who](int pa, InletPatch* out) {
            if (pa < 0 || pa >= hm.nPatches) return fail(FY_ERR_INVALID, "%s: patch %d does not exist (the mesh has %d)", who, pa, hm.nPatches);
            if (hm.psize[(size_t)pa] == 0) return fail(FY_ERR_INVALID, "%s: patch %d is a cyclic patch or has no faces (a cyclic patch is folded into internal faces): no inlet there", who, pa);
            if (h_ubc[(size_t)pa] != FY_BC_U_FIXED_VALUE) return fail(FY_ERR_INVALID, "%s: patch %d is not a fixedValue velocity patch (FY_BC_U_FIXED_VALUE): no inlet there", who, pa);
            out->n_faces = hm.psize[(size_t)pa]; out->base = hm.pstart[(size_t)pa] - ni;
            out->Sf.assign(hm.Sf.begin() + 3 * (size_t)hm.pstart[(size_t)pa], hm.Sf.begin() + 3 * ((size_t)hm.pstart[(size_t)pa] + (size_t)hm.psize[(size_t)pa]));
            return (int)FY_OK;
        }));
        if (fresh.on() && need_ref && !fresh.flux_free()) {               // adjustPhi's precondition, as fy_solver_create states it for the block
            bool adjustable = false;
            for (int pa = 0; pa < hm.nPatches; ++pa) adjustable = adjustable || (hm.psize[(size_t)pa] > 0 && (h_ubc[(size_t)pa] == FY_BC_U_ZERO_GRADIENT || h_ubc[(size_t)pa] >= FY_BC_U_INLET_OUTLET));      // (an open patch is adjustable)
            if (!adjustable)
                return fail(FY_ERR_UNSUPPORTED, "%s: no patch fixes the pressure and the fixed-value velocity patches do not balance (an inlet's shape carries a net normal flux and no "
                                                "velocity patch is adjustable): OpenFOAM's adjustPhi ends such a run with 'Continuity error cannot be removed by adjusting the outflow'", who);
        }
        inl.take(fresh);
        if (!inl.on()) {
            uFace.release(); dInlet.release();
            g.u_face = nullptr; g.u_inlet = nullptr;
        } else {
            std::vector<int32_t> flag((size_t)hm.nPatches, 0);
            for (const Inlets::One& o : inl.in) flag[(size_t)o.patch] = 1;
            FY_TRY(up(dInlet, flag));
            if (!uFace.p) { FY_TRY(uFace.alloc_exact(3 * std::max<size_t>((size_t)(nf - ni), 1))); FY_TRY(zero(uFace)); }
            g.u_face = uFace.p; g.u_inlet = dInlet.p;
            FY_TRY(inl.update(stream, inl.start_time, uFace.p));           // the start time's value, as the 0/U file would hold it
        }
        FY_TRY(create_phi());                                              // createPhi with the boundary values as they are now
        FY_HIP(hipStreamSynchronize(stream));
        return FY_OK;
    }

    // open boundaries (open_boundary.hpp; DESIGN.md section 3 "Open boundaries").  Off (no patch carries an open code): nothing allocated, nothing launched,
    // g.u_inflow null.  mask [nb]: the inflow byte per boundary face; patch [nPatches]: which patches are open for U, k, epsilon or T; sums: the last renewal's
    // three folded sums (OPEN_SUMS), its own partials so that a renewal never touches a reduction in flight
    struct Open {
        bool on = false;
        DevBuf<uint8_t> mask;
        DevBuf<int32_t> patch;
        DevBuf<double> partials, sums, f64;
        KernelClock clock;
    } ob;
    int open_setup(const std::vector<int32_t>& open_patch) {
        const size_t nb = (size_t)(nf - ni);
        FY_TRY(up(ob.patch, open_patch));
        FY_TRY(ob.mask.alloc_exact(std::max<size_t>(nb, 1)));
        FY_HIP(hipMemsetAsync(ob.mask.p, 0, std::max<size_t>(nb, 1), stream));
        FY_TRY(ob.partials.alloc_exact((size_t)OPEN_SUMS * (size_t)ldu_red_blocks((int)nb))); FY_TRY(zero(ob.partials));
        FY_TRY(ob.sums.alloc_exact(OPEN_SUMS)); FY_TRY(zero(ob.sums));
        ob.clock.per_collect = (size_t)1 << 20;                // every launch is timed and counted while timing is on
        ob.on = true;
        g.u_inflow = ob.mask.p;
        return FY_OK;
    }
    // the renewal: the mask from phi as it stands, and the fold of its three sums (no host synchronisation)
    int open_renew() {
        if (!ob.on || nf == ni) return FY_OK;
        ob.clock.begin(stream);
        FY_TRY(launch_ldu_open_faces(stream, g, ob.patch.p, phi.p, ob.mask.p, ob.partials.p));
        ob.clock.end(stream);
        ob.clock.begin(stream);
        FY_TRY(launch_reduce_finalize(stream, ob.partials.p, nf - ni, OPEN_SUMS, nullptr, ob.sums.p, nullptr, 0));
        ob.clock.end(stream);
        return FY_OK;
    }
    // createPhi: phi = fvc::flux(U) with every open face evaluated as zeroGradient (the mask cleared first), then the mask of that flux
    int create_phi() {
        if (ob.on) FY_HIP(hipMemsetAsync(ob.mask.p, 0, std::max<size_t>((size_t)(nf - ni), 1), stream));
        FY_TRY(launch_ldu_flux_of(stream, g, U.p, phi.p));
        return open_renew();
    }
    int get_open_stats(int64_t* inflow_faces, double* inflow_flux, double* outflow_flux) {
        if (!ob.on) return fail(FY_ERR_INVALID, "fy_ldu_solver_get_open_boundary_stats: no patch carries an open code (FY_BC_U_INLET_OUTLET, FY_BC_U_PRESSURE_INLET_OUTLET, FY_BC_NUT_INLET_OUTLET, FY_BC_T_INLET_OUTLET)");
        FY_HIP(hipSetDevice(device));
        double h[OPEN_SUMS];
        FY_HIP(hipMemcpyAsync(h, ob.sums.p, sizeof(h), hipMemcpyDeviceToHost, stream));
        FY_HIP(hipStreamSynchronize(stream));
        if (inflow_faces) *inflow_faces = (int64_t)h[OPEN_INFLOW_FACES];
        if (inflow_flux) *inflow_flux = h[OPEN_INFLOW_FLUX];
        if (outflow_flux) *outflow_flux = h[OPEN_OUTFLOW_FLUX];
        return FY_OK;
    }

    ~LduSolver() {
        ob.clock.destroy();
        fc.clock.destroy();
        inl.clock.destroy();
        if (cpl) fy_destroy(cpl);
        for (auto& t : tim) t.destroy();
        if (side) (void)hipStreamDestroy(side);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_fields) (void)hipEventDestroy(ev_fields);
        if (stream) (void)hipStreamDestroy(stream);
    }
    template <class T> int up(DevBuf<T>& d, const std::vector<T>& h) {
        FY_TRY(d.alloc_exact(std::max<size_t>(h.size(), 1)));
        if (!h.empty()) { FY_HIP(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, stream)); FY_HIP(hipStreamSynchronize(stream)); }      // (set-up only; the source may die with its scope)
        return FY_OK;
    }
    int zero(DevBuf<double>& b) { if (b.n) FY_HIP(hipMemsetAsync(b.p, 0, b.n * sizeof(double), stream)); return FY_OK; }
    LduMom M() { return LduMom{mdiag.p, mlower.p, mupper.p, mb.p, (has_slip || por.on()) ? mbdiag.p : nullptr}; }

    int create(const fy_poly_mesh* m, const fy_ldu_case* c, const fy_transport* tr, int dev) {
        th.part.who = "fy_ldu_solver"; th.part.desc = "fy_ldu_case";
        if (!c || !(c->dt > 0) || !(c->nu >= 0) || !c->u_bc || !c->u_value || !c->p_bc || !c->p_value) return fail(FY_ERR_INVALID, "fy_ldu_solver_create: bad case (dt, nu, the per-patch arrays)");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(FY_ERR_NO_DEVICE, "no HIP device visible: libfoamyade_hip has no CPU path");
        if (dev < 0 || dev >= ndev) return fail(FY_ERR_INVALID, "device ordinal out of range");
        FY_TRY(hm.build(m));
        cs = *c; device = dev;
        pimple = c->solver == FY_SOLVER_PIMPLE;
        if (c->solver != FY_SOLVER_ICO && !pimple) return fail(FY_ERR_INVALID, "fy_ldu_solver: solver %d (FY_SOLVER_ICO, FY_SOLVER_PIMPLE)", c->solver);
        if (pimple && c->n_outer_correctors < 1) cs.n_outer_correctors = 1;
        if (c->adjust_time_step && !pimple) cs.adjust_time_step = 0;                      // (icoFoamYade's loop never includes setDeltaT.H: icoFoamYade.C:65-70)
        if (cs.adjust_time_step && !(c->max_co > 0 && c->max_delta_t > 0)) return fail(FY_ERR_INVALID, "fy_ldu_solver: adjustTimeStep needs maxCo > 0 and maxDeltaT > 0");
        if (c->turbulence_model != FY_TURBULENCE_LAMINAR && !(pimple && (c->turbulence_model == FY_TURBULENCE_SMAGORINSKY || c->turbulence_model == FY_TURBULENCE_KEQN || c->turbulence_model == FY_TURBULENCE_KEPSILON)))
            return fail(FY_ERR_UNSUPPORTED, "fy_ldu_solver: turbulence model %d (laminar; LES Smagorinsky, LES kEqn or RAS kEpsilon with pimpleFoamYade)", c->turbulence_model);
        keps = pimple && c->turbulence_model == FY_TURBULENCE_KEPSILON;
        if (keps && !(c->ras_cmu > 0 && c->ras_sigmak > 0 && c->ras_sigmaeps > 0 && c->eps_initial > 0 && c->k_initial > 0 && c->eps_tol >= 0 && c->eps_max_iter >= 0 &&
                      (c->eps_convection_scheme == FY_CONVECTION_LINEAR || c->eps_convection_scheme == FY_CONVECTION_UPWIND) &&
                      (c->k_convection_scheme == FY_CONVECTION_LINEAR || c->k_convection_scheme == FY_CONVECTION_UPWIND)))
            return fail(FY_ERR_INVALID, "fy_ldu_solver: kEpsilon needs Cmu, sigmak, sigmaEps, k and epsilon of the start time positive, and Gauss linear or Gauss upwind for their convection");
        les = pimple && c->turbulence_model != FY_TURBULENCE_LAMINAR;
        keqn = pimple && c->turbulence_model == FY_TURBULENCE_KEQN;
        if (keqn && !(c->k_initial >= 0 && c->k_tol >= 0 && c->k_max_iter >= 0 && (c->k_convection_scheme == FY_CONVECTION_LINEAR || c->k_convection_scheme == FY_CONVECTION_UPWIND)))
            return fail(FY_ERR_INVALID, "fy_ldu_solver: kEqn needs k_initial >= 0, solver controls for k and Gauss linear or Gauss upwind for div(alphaPhic,k)");
        if (c->convection_scheme < FY_CONVECTION_LINEAR || c->convection_scheme > FY_CONVECTION_QUICK)
            return fail(FY_ERR_UNSUPPORTED, "fy_ldu_solver: convection scheme %d (FY_CONVECTION_LINEAR .. FY_CONVECTION_QUICK)", c->convection_scheme);
        if (c->convection_scheme == FY_CONVECTION_LIMITED_LINEAR && !(c->convection_limiter_k >= 0 && c->convection_limiter_k <= 1)) return fail(FY_ERR_INVALID, "fy_ldu_solver: limitedLinear takes a coefficient in [0, 1]");
        if (les && !(c->les_ck > 0 && c->les_ce > 0 && c->les_delta_coeff > 0)) return fail(FY_ERR_INVALID, "fy_ldu_solver: Smagorinsky needs Ck, Ce and the delta coefficient positive");
        nc = hm.nCells; nf = hm.nFaces; ni = hm.nInt;
        ywall.assign((size_t)(nf - ni), 0.0);
        std::vector<int32_t> ubc(c->u_bc, c->u_bc + hm.nPatches), pbc(c->p_bc, c->p_bc + hm.nPatches);
        std::vector<double> uval(c->u_value, c->u_value + 3 * (size_t)hm.nPatches), pval(c->p_value, c->p_value + hm.nPatches);
        need_ref = true;
        h_ubc = ubc;
        std::vector<int32_t> open_patch((size_t)hm.nPatches, 0);      // the patches that carry an open code for U, k, epsilon or T
        for (int pa = 0; pa < hm.nPatches; ++pa) {
            if (ubc[(size_t)pa] != FY_BC_U_FIXED_VALUE && ubc[(size_t)pa] != FY_BC_U_ZERO_GRADIENT && ubc[(size_t)pa] != FY_BC_U_SLIP && ubc[(size_t)pa] != FY_BC_U_INLET_OUTLET &&
                ubc[(size_t)pa] != FY_BC_U_PRESSURE_INLET_OUTLET)
                return fail(FY_ERR_UNSUPPORTED, "fy_ldu_solver: velocity patch type %d (fixedValue, zeroGradient, symmetry / slip, inletOutlet, pressureInletOutletVelocity)", ubc[(size_t)pa]);
            has_slip = has_slip || ubc[(size_t)pa] == FY_BC_U_SLIP || ubc[(size_t)pa] == FY_BC_U_PRESSURE_INLET_OUTLET;      // (the transform-patch form: a per-component boundary diagonal)
            if (ubc[(size_t)pa] >= FY_BC_U_INLET_OUTLET) open_patch[(size_t)pa] = 1;
            if (pbc[(size_t)pa] != FY_BC_P_ZERO_GRADIENT && pbc[(size_t)pa] != FY_BC_P_FIXED_VALUE && !(pimple && pbc[(size_t)pa] == FY_BC_P_FIXED_FLUX))
                return fail(FY_ERR_UNSUPPORTED, "fy_ldu_solver: pressure patch type %d (zeroGradient, fixedValue; fixedFluxPressure with pimpleFoamYade)", pbc[(size_t)pa]);
            if (pbc[(size_t)pa] == FY_BC_P_FIXED_VALUE) need_ref = false;
        }
        if (need_ref && (c->p_ref_cell < 0 || c->p_ref_cell >= nc)) return fail(FY_ERR_INVALID, "fy_ldu_solver: pRefCell out of range");
        std::vector<int32_t> tbc((size_t)hm.nPatches, FY_BC_T_ZERO_GRADIENT);
        std::vector<double> tval((size_t)hm.nPatches, 0.0);
        if (c->thermal.on) {                                                  // (what Solver::thermal_create checks, with the patches of this mesh in the six sides' place)
            FY_TRY(HeatExchange::validate(c->thermal, pimple, c->rho_particle, "fy_ldu_solver_create"));
            for (int pa = 0; pa < hm.nPatches; ++pa) {
                if (c->T_bc) tbc[(size_t)pa] = c->T_bc[pa];
                if (c->T_value) tval[(size_t)pa] = c->T_value[pa];
                if (tbc[(size_t)pa] != FY_BC_T_ZERO_GRADIENT && tbc[(size_t)pa] != FY_BC_T_FIXED_VALUE && tbc[(size_t)pa] != FY_BC_T_INLET_OUTLET)
                    return fail(FY_ERR_UNSUPPORTED, "fy_ldu_solver_create: unknown T_bc %d on patch %d (FY_BC_T_ZERO_GRADIENT, FY_BC_T_FIXED_VALUE, FY_BC_T_INLET_OUTLET)", tbc[(size_t)pa], pa);
                if (tbc[(size_t)pa] == FY_BC_T_INLET_OUTLET) open_patch[(size_t)pa] = 1;
            }
        }
        cs.T_bc = nullptr; cs.T_value = nullptr;
        if (c->p_solver != FY_PSOLVER_PCG_JACOBI && c->p_solver != FY_PSOLVER_PCG_MG) return fail(FY_ERR_INVALID, "fy_ldu_solver: p_solver %d (FY_PSOLVER_PCG_JACOBI, FY_PSOLVER_PCG_MG)", c->p_solver);
        cs.u_bc = nullptr; cs.u_value = nullptr; cs.p_bc = nullptr; cs.p_value = nullptr;      // (copied; the caller's arrays are not kept)
        FY_HIP(hipSetDevice(device));
        FY_HIP(hipStreamCreate(&stream));
        FY_TRY(up(d_own, hm.own)); FY_TRY(up(d_nei, hm.nei)); FY_TRY(up(d_patch_of, hm.patch_of)); FY_TRY(up(d_cf_off, hm.cf_off)); FY_TRY(up(d_cf_face, hm.cf_face)); FY_TRY(up(d_ef, hm.ef)); FY_TRY(up(d_en, hm.en));
        FY_TRY(up(d_Cf, hm.Cf)); FY_TRY(up(d_Sf, hm.Sf)); FY_TRY(up(d_magSf, hm.magSf)); FY_TRY(up(d_C, hm.C)); FY_TRY(up(d_V, hm.V)); FY_TRY(up(d_w, hm.w));
        FY_TRY(up(d_dcNO, hm.dcNO)); FY_TRY(up(d_kvec, hm.kvec)); FY_TRY(up(d_ubc, ubc)); FY_TRY(up(d_pbc, pbc)); FY_TRY(up(d_uval, uval)); FY_TRY(up(d_pval, pval));
        FY_TRY(up(d_recon, hm.recon));
        if (pimple) { FY_TRY(psn.alloc_exact(std::max<size_t>((size_t)(nf - ni), 1))); FY_TRY(zero(psn)); }
        g = LduGeo{nc, nf, ni, hm.nPatches, d_own.p, d_nei.p, d_patch_of.p, d_cf_off.p, d_cf_face.p, hm.Wall, d_ef.p, d_en.p, d_Cf.p, d_Sf.p, d_magSf.p, d_C.p, d_V.p, d_w.p, d_dcNO.p, d_kvec.p,
                   d_ubc.p, d_pbc.p, d_uval.p, d_pval.p, d_recon.p, pimple ? psn.p : nullptr, cs.dt, cs.nu, cs.convection_scheme, 2.0 / std::max(cs.convection_limiter_k, 1e-15), nullptr, need_ref ? 1 : 0, cs.p_ref_cell, cs.p_ref_value};
        FY_TRY(d_gB.alloc_exact(3 * (size_t)hm.Wall * nc)); FY_TRY(d_gG0.alloc_exact(3 * (size_t)nc)); FY_TRY(d_rT.alloc_exact(3 * (size_t)hm.Wall * nc));
        FY_TRY(launch_ldu_slot_coefs(stream, g, d_gB.p, d_gG0.p, d_rT.p));
        g.gB = d_gB.p; g.gG0 = d_gG0.p; g.rT = d_rT.p;
        if (!hm.sep.empty()) { FY_TRY(up(d_sep, hm.sep)); g.sep = d_sep.p; }
        g.nIntReal = hm.n_real_internal;
        orig_face_d.assign(hm.orig_face.begin(), hm.orig_face.end());
        total_volume = 0.0;
        for (double v : hm.V) total_volume += v;
        const size_t n = (size_t)nc;
        DevBuf<double>* v3[] = {&U, &Uold, &uSource, &uSourceExt, &uSourceSum, &gradp, &mb, &xscr, &HbyA, &dummy3};
        for (auto* b : v3) { FY_TRY(b->alloc_exact(3 * n)); FY_TRY(zero(*b)); }
        DevBuf<double>* v1[] = {&p, &mdiag, &rAU, &pdiag, &prhs, &pr, &pu, &pw, &pp, &ps, &dummy1};
        for (auto* b : v1) { FY_TRY(b->alloc_exact(n)); FY_TRY(zero(*b)); }
        FY_TRY(vGrad.alloc_exact(9 * n)); FY_TRY(zero(vGrad));
        if (has_slip) { FY_TRY(mbdiag.alloc_exact(3 * n)); FY_TRY(zero(mbdiag)); }
        DevBuf<double>* vf[] = {&phi, &phiOld, &rAUf, &phiHbyA, &pcoef, &pt};
        for (auto* b : vf) { FY_TRY(b->alloc_exact((size_t)nf)); FY_TRY(zero(*b)); }
        DevBuf<double>* vi[] = {&mlower, &mupper, &pcorr};
        for (auto* b : vi) { FY_TRY(b->alloc_exact(std::max<size_t>((size_t)ni, 1))); FY_TRY(zero(*b)); }
        FY_TRY(fcorr.alloc_exact(3 * std::max<size_t>((size_t)ni, 1))); FY_TRY(zero(fcorr));
        FY_TRY(partials.alloc_exact(8 * (size_t)ldu_red_blocks(std::max(nc, nf)))); FY_TRY(zero(partials));
        FY_TRY(sc.alloc_exact(8)); FY_TRY(zero(sc)); FY_TRY(xsum.alloc_exact(4)); FY_TRY(zero(xsum)); FY_TRY(adj.alloc_exact(4)); FY_TRY(zero(adj));
        FY_TRY(adj_err.alloc_exact(1)); FY_HIP(hipMemsetAsync(adj_err.p, 0, sizeof(int), stream));
        rb.init(MappedReadback::kFlags);
        if (pimple) {
            DevBuf<double>* p3[] = {&uParticle, &gradP, &divT, &ddtU, &bmom};
            for (auto* b : p3) { FY_TRY(b->alloc_exact(3 * n)); FY_TRY(zero(*b)); }
            DevBuf<double>* p1[] = {&alpha, &uSourceDrag, &pPrev};
            for (auto* b : p1) { FY_TRY(b->alloc_exact(n)); FY_TRY(zero(*b)); }
            DevBuf<double>* pf[] = {&alphaf, &phiForces, &arAUf, &phiA, &ssf};
            for (auto* b : pf) { FY_TRY(b->alloc_exact((size_t)nf)); FY_TRY(zero(*b)); }
            FY_TRY(fstress.alloc_exact(3 * (size_t)nf)); FY_TRY(zero(fstress));
            FY_TRY(launch_fill_f64(stream, alpha.p, n, 1.0));                 // alpha = 1.0 (FoamYade.C:68)
            FY_TRY(launch_fill_f64(stream, alphaf.p, (size_t)nf, 1.0));
            if (les) {                                                        // nut of the start time: the file's values (eddyViscosity: MUST_READ; no validate() in createFields.H)
                std::vector<int32_t> nb((size_t)hm.nPatches, FY_BC_NUT_ZERO_GRADIENT);
                std::vector<double> nv((size_t)hm.nPatches, 0.0);
                for (int pa = 0; pa < hm.nPatches; ++pa) {
                    if (c->nut_bc) nb[(size_t)pa] = c->nut_bc[pa];
                    if (c->nut_value) nv[(size_t)pa] = c->nut_value[pa];
                    if (nb[(size_t)pa] != FY_BC_NUT_ZERO_GRADIENT && nb[(size_t)pa] != FY_BC_NUT_FIXED_VALUE && !((keqn || keps) && (nb[(size_t)pa] == FY_BC_NUT_CALCULATED || nb[(size_t)pa] == FY_BC_WALL_FUNCTION)))
                        return fail(FY_ERR_UNSUPPORTED, "fy_ldu_solver: nut patch type %d (zeroGradient, fixedValue; calculated or nutkWallFunction with kEqn / kEpsilon)", nb[(size_t)pa]);
                }
                FY_TRY(up(d_nutbc, nb)); FY_TRY(up(d_nutval, nv));
                FY_TRY(nut.alloc_exact(n));
                FY_TRY(launch_fill_f64(stream, nut.p, n, c->nut_initial));
            }
            std::vector<char> wf_eps((size_t)hm.nPatches, 0);
            if (keps) {                                                       // epsilon of the start time, its patches (an epsilonWallFunction patch is a zero-gradient one wherever its face value is asked for)
                std::vector<int32_t> eb((size_t)hm.nPatches, FY_BC_NUT_ZERO_GRADIENT);
                std::vector<double> ev((size_t)hm.nPatches, 0.0);
                for (int pa = 0; pa < hm.nPatches; ++pa) {
                    if (c->eps_bc) eb[(size_t)pa] = c->eps_bc[pa];
                    if (c->eps_value) ev[(size_t)pa] = c->eps_value[pa];
                    if (eb[(size_t)pa] != FY_BC_NUT_ZERO_GRADIENT && eb[(size_t)pa] != FY_BC_NUT_FIXED_VALUE && eb[(size_t)pa] != FY_BC_WALL_FUNCTION && eb[(size_t)pa] != FY_BC_NUT_INLET_OUTLET)
                        return fail(FY_ERR_UNSUPPORTED, "fy_ldu_solver: epsilon patch type %d (zeroGradient, fixedValue, epsilonWallFunction, inletOutlet)", eb[(size_t)pa]);
                    if (eb[(size_t)pa] == FY_BC_NUT_INLET_OUTLET) open_patch[(size_t)pa] = 1;
                    wf_eps[(size_t)pa] = eb[(size_t)pa] == FY_BC_WALL_FUNCTION;
                }
                FY_TRY(up(d_epsbc, eb)); FY_TRY(up(d_epsval, ev));
                FY_TRY(epsturb.alloc_exact(n));
                FY_TRY(launch_fill_f64(stream, epsturb.p, n, c->eps_initial));
                cs.eps_bc = nullptr; cs.eps_value = nullptr;
            }
            if (keqn || keps) {                                               // k of the start time (kEqn / kEpsilon: k_ is MUST_READ), its patches
                std::vector<int32_t> kb((size_t)hm.nPatches, FY_BC_NUT_ZERO_GRADIENT);
                std::vector<double> kv((size_t)hm.nPatches, 0.0);
                for (int pa = 0; pa < hm.nPatches; ++pa) {
                    if (c->k_bc) kb[(size_t)pa] = c->k_bc[pa];
                    if (c->k_value) kv[(size_t)pa] = c->k_value[pa];
                    if (kb[(size_t)pa] != FY_BC_NUT_ZERO_GRADIENT && kb[(size_t)pa] != FY_BC_NUT_FIXED_VALUE && kb[(size_t)pa] != FY_BC_NUT_INLET_OUTLET)
                        return fail(FY_ERR_UNSUPPORTED, "fy_ldu_solver: k patch type %d (zeroGradient, fixedValue, inletOutlet)", kb[(size_t)pa]);
                    if (kb[(size_t)pa] == FY_BC_NUT_INLET_OUTLET) open_patch[(size_t)pa] = 1;
                }
                FY_TRY(up(d_kbc, kb)); FY_TRY(up(d_kval, kv));
                FY_TRY(kturb.alloc_exact(n)); FY_TRY(gradk.alloc_exact(3 * n));
                FY_TRY(launch_fill_f64(stream, kturb.p, n, c->k_initial));
                cs.k_bc = nullptr; cs.k_value = nullptr;
            }
            FY_TRY(setup_wall_functions(c, wf_eps));
        }
        for (auto& t : tim) FY_TRY(t.init());
        if (cs.convection_scheme >= FY_CONVECTION_LIMITED_LINEAR) { FY_TRY(gradL.alloc_exact(3 * n)); FY_TRY(zero(gradL)); g.gradL = gradL.p; }
        amg.passes = options().amg_passes;
        FY_TRY(amg.build(stream, nc, ni, hm.own.data(), hm.nei.data(), hm.cf_off, hm.cf_face, hm.magSf.data(), need_ref ? cs.p_ref_cell : -1, cs.p_solver == FY_PSOLVER_PCG_MG));
        // the coupling object on this mesh (icoFoamYade.C:54: point force): its tree over the cell centres, its fields the solver's device arrays
        {
            fy_mesh_desc md{};
            md.n_cells = nc; md.centres = hm.C.data(); md.volumes = hm.V.data();
            md.nx = md.ny = md.nz = 0; md.dx = 0.0;
            for (int a = 0; a < 3; ++a) { md.bbox_min[a] = hm.bbox_min[a]; md.bbox_max[a] = hm.bbox_max[a]; md.origin[a] = hm.bbox_min[a]; }
            fy_field_ptrs fp{};
            fp.location = FY_MEM_DEVICE;
            fp.U = U.p; fp.gradP = pimple ? gradP.p : dummy3.p; fp.vGrad = vGrad.p; fp.divT = pimple ? divT.p : dummy3.p; fp.ddtU = pimple ? ddtU.p : dummy3.p;
            fp.uSourceDrag = pimple ? uSourceDrag.p : dummy1.p; fp.alpha = pimple ? alpha.p : dummy1.p; fp.uSource = uSource.p; fp.uParticle = pimple ? uParticle.p : dummy3.p;
            cpl = new (std::nothrow) fy_ctx();
            if (!cpl) return fail(FY_ERR_INVALID, "out of host memory");
            cpl->c.ext_stream = stream;
            cpl->c.ldu_geo = &g;
            if (!pimple) {
                FY_TRY(up(d_pts, hm.pts)); FY_TRY(up(d_fp_off, hm.fp_off)); FY_TRY(up(d_fp_pts, hm.fp_pts)); FY_TRY(up(d_cell_r2, hm.cell_r2));
                fans.pts = d_pts.p; fans.fp_off = d_fp_off.p; fans.fp_pts = d_fp_pts.p; fans.cell_r2 = d_cell_r2.p;
                FY_TRY(up(d_bin_off, hm.bin_off)); FY_TRY(up(d_bin_cell, hm.bin_cell));
                fans.bin_off = d_bin_off.p; fans.bin_cell = d_bin_cell.p;
                for (int a = 0; a < 3; ++a) { fans.bbmin[a] = hm.bbox_min[a]; fans.bbmax[a] = hm.bbox_max[a]; fans.bin_n[a] = hm.bin_n[a]; fans.bin_inv[a] = hm.bin_inv[a]; }
                cpl->c.ldu_fans = &fans;
            }
            FY_TRY(cpl->c.create(&md, &fp, pimple ? 1 : 0, tr, device));        // gaussianInterp: false in icoFoamYade (icoFoamYade.C:53), true in pimpleFoamYade (pimpleFoamYade.C:52)
            cpl->c.rhoP = c->rho_particle; cpl->c.rhoF = c->rho_fluid; cpl->c.nu = c->nu;      // setScalarProperties (icoFoamYade.C:55)
            if (c->drag_law != FY_DRAG_REFERENCE) FY_TRY(cpl->c.set_drag_law(c->drag_law));                  // constant/couplingProperties
            if (c->force_models) FY_TRY(cpl->c.set_force_models(c->force_models));
        }
        if (std::find(open_patch.begin(), open_patch.end(), 1) != open_patch.end()) {      // (before the coupling takes &g is fine: it reads g through the pointer)
            FY_TRY(open_setup(open_patch));
            ob.clock.on = ss.clock.on;
        }
        FY_TRY(create_phi());                                                 // createPhi
        if (c->thermal.on) FY_TRY(thermal_create(c, tbc, tval));              // (before fieldAverage, which may ask for T)
        FY_HIP(hipStreamSynchronize(stream));
        if (c->solid_stats) FY_TRY(set_solid_statistics(1));                  // couplingProperties solidStatistics (before fieldAverage and the monitors, which may ask for its fields)
        if (c->average.n_items) FY_TRY(set_field_average(&c->average));       // controlDict functions: fieldAverage
        if (c->monitors.n_objects) FY_TRY(set_monitors(&c->monitors));        // volFieldValue / surfaceFieldValue
        cs.flow_control = fy_flow_control_desc{};
        if (c->flow_control.on) FY_TRY(set_flow_control(&c->flow_control, "fy_ldu_solver_create"));      // couplingProperties meanVelocityForce
        if (!WallLoads::empty(&c->wall_loads)) FY_TRY(set_wall_loads(&c->wall_loads));                   // forces / wallShearStress / yPlus
        cs.inlets = fy_inlets_desc{};
        if (c->inlets.n) FY_TRY(set_inlets(&c->inlets, "fy_ldu_solver_create"));                          // (the caller's arrays are copied, not kept)
        return FY_OK;
    }

    int thermal_create(const fy_ldu_case* c, const std::vector<int32_t>& tbc, const std::vector<double>& tval) {
        const fy_thermal_desc& d = c->thermal;
        const size_t n = (size_t)nc;
        th.d = d;
        FY_TRY(up(th.d_bc, tbc)); FY_TRY(up(th.d_val, tval));
        DevBuf<double>* bs[] = {&th.T, &th.Sp, &th.Su};
        for (auto* b : bs) { FY_TRY(b->alloc_exact(n)); FY_TRY(zero(*b)); }
        FY_TRY(th.gradT.alloc_exact(3 * n)); FY_TRY(zero(th.gradT));
        FY_TRY(launch_fill_f64(stream, th.T.p, n, d.T_initial));
        th.eq = LduTEqn{th.T.p, th.d_bc.p, th.d_val.p, d.T_convection_scheme == FY_CONVECTION_UPWIND ? 1 : 0, d.kappa / (c->rho_fluid * d.cp), 1.0 / (d.prt > 0 ? d.prt : 1.0),
                        1.0 / (c->rho_fluid * d.cp)};
        th.part.configure(d, c->nu, c->rho_fluid, c->rho_particle, c->dt, "fy_ldu_solver", "fy_ldu_case");
        th.buoyant = d.beta != 0.0 && (c->g[0] != 0.0 || c->g[1] != 0.0 || c->g[2] != 0.0);
        if (th.buoyant) { FY_TRY(th.buoy.alloc_exact(3 * n)); FY_TRY(zero(th.buoy)); FY_TRY(th.usrc_sum.alloc_exact(3 * n)); FY_TRY(zero(th.usrc_sum)); }
        th.on = true;
        return FY_OK;
    }
    // pass A on the solver's stream, right after setParticleAction returned (pimpleFoamYade: and after the side stream's sweeps, whose alphaf the later kernels read): a
    // general mesh has no tiles, so the Gaussian scatter's table flushes as global atomics
    int heat_coefficients() {
        FY_TRY(zero(th.Sp)); FY_TRY(zero(th.Su));
        return th.part.coefficients(cpl->c, stream, CellWindow{0, (int64_t)nc}, U.p, th.Sp.p, th.Su.p, cs.dt, false);
    }
    // the T equation, once per step with the step's final phi and nut, into the momentum matrix's storage as {T, 0, 0}; then pass B with the new T
    int solve_temperature() {
        LduMom Mt = M();
        Mt.bdiag = nullptr;
        const LduPim Pt = pimple ? P() : LduPim{};                // (icoFoamYade: alpha = alphaf = 1, nut = 0)
        FY_TRY(launch_ldu_grad_T(stream, g, th.eq, th.gradT.p));
        FY_TRY(launch_ldu_T_assemble(stream, g, Pt, th.eq, phi.p, th.gradT.p, th.Sp.p, th.Su.p, Mt, fcorr.p, HbyA.p));
        FY_TRY(solve_vec3(&th.iters, Mt, mb.p, nullptr, &HbyA.p, &xscr.p, th.d.T_tol, th.d.T_rel_tol, th.d.T_max_iter, &th.res0));
        FvGeo flat{};                                             // (k_scalar_finish reads the cell count and the first cell only)
        flat.Nc = nc; flat.c0 = 0;
        FY_TRY(launch_scalar_finish(stream, flat, HbyA.p, th.T.p));
        return th.part.fluxes(cpl->c, stream, CellWindow{0, (int64_t)nc}, th.T.p);
    }

    // nearWallDist on the patches with a wall-function nut or epsilon, and the list of the cells with epsilonWallFunction faces (what k_ldu_wall_functions runs over)
    int setup_wall_functions(const fy_ldu_case* c, const std::vector<char>& wf_eps) {
        const int nb = nf - ni;
        std::vector<char> on((size_t)hm.nPatches, 0);
        bool any = false;
        for (int pa = 0; pa < hm.nPatches; ++pa) {
            on[(size_t)pa] = wf_eps[(size_t)pa] || (les && c->nut_bc && c->nut_bc[pa] == FY_BC_WALL_FUNCTION);
            any = any || on[(size_t)pa];
        }
        if (!any) return FY_OK;
        if (!(c->wf_kappa > 0 && c->wf_E > 0)) return fail(FY_ERR_INVALID, "fy_ldu_solver: wall-function constants kappa, E must be positive");
        wf_yplam = wall_yplus_lam(c->wf_kappa, c->wf_E);
        hm.near_wall_dist(on, &ywall);
        wf_on = on;
        FY_TRY(up(d_ywall, ywall));
        std::vector<int32_t> cnt((size_t)nc, 0), wall_of((size_t)nc, -1), cell, off(1, 0), face;
        for (int b = 0; b < nb; ++b) if (wf_eps[(size_t)hm.patch_of[(size_t)b]]) ++cnt[(size_t)hm.own[(size_t)(ni + b)]];
        for (int q = 0; q < nc; ++q) if (cnt[(size_t)q]) { wall_of[(size_t)q] = (int32_t)cell.size(); cell.push_back(q); off.push_back(off.back() + cnt[(size_t)q]); }
        n_wall_cells = (int)cell.size();
        if (n_wall_cells == 0) return FY_OK;
        face.assign((size_t)off.back(), 0);
        std::vector<int32_t> fill(off.begin(), off.end() - 1);
        for (int b = 0; b < nb; ++b) if (wf_eps[(size_t)hm.patch_of[(size_t)b]]) { const int w = wall_of[(size_t)hm.own[(size_t)(ni + b)]]; face[(size_t)fill[(size_t)w]++] = ni + b; }
        FY_TRY(up(d_wc_cell, cell)); FY_TRY(up(d_wc_off, off)); FY_TRY(up(d_wc_face, face)); FY_TRY(up(d_wall_of, wall_of));
        FY_TRY(wall_eps.alloc_exact((size_t)n_wall_cells)); FY_TRY(wall_G.alloc_exact((size_t)n_wall_cells));
        return FY_OK;
    }

    // fold `nslots` of the block partials of an n-cell reduction and read them back
    // through mapped pinned host memory and its arrival flags (common.hpp: MappedReadback); without them the fold lands on the device and is copied
    MappedReadback rb;
    int reduce_read(int n, int nslots, const int* ops_dev, double* h, double* dev_land = nullptr) {      // dev_land: where the copy path lets the fold land (default: sc)
        if (rb.flagged(nslots)) {
            FY_TRY(launch_reduce_finalize(stream, partials.p, n, nslots, ops_dev, rb.dev, rb.flag_dev, ++rb.seq));
            return rb.wait(stream, nslots, h);
        }
        double* land = dev_land ? dev_land : sc.p;
        FY_TRY(launch_reduce_finalize(stream, partials.p, n, nslots, ops_dev, land, nullptr, 0));
        FY_HIP(hipMemcpyAsync(h, land, nslots * sizeof(double), hipMemcpyDeviceToHost, stream));
        FY_HIP(hipStreamSynchronize(stream));
        return FY_OK;
    }
    DevBuf<int> ops_courant;

    int solve_momentum(int* iters, const double* rhs, const double* gp) {
        FY_TRY(solve_vec3(iters, M(), rhs, gp, &U.p, &xscr.p, cs.u_tol, cs.u_rel_tol, cs.u_max_iter));
        if (cpl) cpl->c.dU = U.p;
        return FY_OK;
    }
    // Jacobi passes on a three-component system with lduMatrix::solver's L1 residual control per component; the converged iterate ends up in *x (the two buffers may trade places)
    int solve_vec3(int* iters, LduMom Mx, const double* rhs, const double* gp, double** x, double** scratch, double tol, double rel_tol, int max_iter, double* res0_out = nullptr) {
        FY_TRY(launch_ldu_sum(stream, *x, nc, 3, partials.p));
        FY_TRY(launch_reduce_finalize(stream, partials.p, nc, 3, nullptr, xsum.p, nullptr, 0));
        double* xc = *x; double* xn = *scratch;
        double norm[3] = {1, 1, 1}, res0[3] = {0, 0, 0}, h[6];
        int it = 0;
        for (;;) {
            FY_TRY(launch_ldu_mom_pass(stream, g, Mx, rhs, gp, xc, xn, xsum.p, partials.p));
            FY_TRY(reduce_read(nc, 6, nullptr, h));
            if (vec3_converged(it, h, tol, rel_tol, norm, res0) || it >= max_iter) break;
            std::swap(xc, xn);
            ++it;
        }
        if (xc != *x) std::swap(*x, *scratch);            // the converged iterate sits in the scratch buffer: the two trade places
        *iters = it;
        if (res0_out) *res0_out = res0[0];
        return FY_OK;
    }

    // OpenFOAM PCG.C with the diagonal preconditioner and lduMatrix::solver::normFactor, in the single-reduction form (fv_pressure.cpp, k_pcg_cg_update)
    int solve_pressure(bool final_iter) {
        const double tol = final_iter ? cs.p_final_tol : cs.p_tol, rel = final_iter ? cs.p_final_rel_tol : cs.p_rel_tol;
        double h[2];
        FY_TRY(launch_ldu_sum(stream, p.p, nc, 1, partials.p));
        FY_TRY(launch_reduce_finalize(stream, partials.p, nc, 1, nullptr, xsum.p, nullptr, 0));
        { const EllMat A0 = amg.lev[0]->mat(); FY_TRY(launch_ldu_p_init(stream, g, pdiag.p, A0.W, A0.nbr, A0.coef, prhs.p, p.p, xsum.p, 1.0 / (double)nc, pr.p, partials.p)); }
        FY_TRY(reduce_read(nc, 2, nullptr, h));
        const double norm = h[1] + 1e-20;
        double res = h[0] / norm;
        const double res0 = res;
        st.p_initial_residual = res0;
        auto converged = [&](double r) { return r < tol || (rel > 0 && r < rel * res0); };
        int it = 0;
        if (!converged(res)) {
            do {
                if (amg.has_hierarchy()) FY_TRY(amg.vcycle(stream, pr.p, pu.p));                                  // u = M^-1 r
                else FY_TRY(launch_ell_jacobi(stream, nc, pdiag.p, pr.p, pu.p));
                EllMat A = amg.lev[0]->mat();
                A.diag = pdiag.p;
                FY_TRY(launch_ell_apply_dot(stream, A, pu.p, pr.p, pw.p, partials.p));                            // w = A u; gamma = u.r, delta = u.w
                FY_TRY(launch_reduce_finalize(stream, partials.p, nc, 2, nullptr, sc.p, nullptr, 0));
                FY_TRY(launch_pcg_cg_update(stream, nc, 0, pu.p, pw.p, pp.p, ps.p, p.p, pr.p, sc.p, it, partials.p));
                if (it == 0) { std::swap(pp.p, pu.p); std::swap(ps.p, pw.p); }      // p = u, s = w without a pass
                FY_TRY(reduce_read(nc, 2, nullptr, h, sc.p + 6));      // (the copy path must not touch the iteration's scalars in sc[0 .. 5])
                res = h[0] / norm;
            } while (++it < cs.p_max_iter && !converged(res));
        }
        st.p_final_residual = res;
        st.p_iters_total += it; st.p_solves += 1;
        return FY_OK;
    }

    int corrector(bool final_corr) {
        FY_TRY(launch_ldu_HbyA(stream, g, M(), U.p, rAU.p, HbyA.p));                                              // icoFoamYade.C:99-100
        FY_TRY(launch_ldu_phiHbyA(stream, g, HbyA.p, rAU.p, Uold.p, phiOld.p, nullptr, rAUf.p, phiHbyA.p));      // :101-106
        if (need_ref) FY_TRY(launch_ldu_adjust_phi(stream, g, phiHbyA.p, adj.p, adj_err.p, partials.p));                      // :108
        for (int no = 0; no <= cs.n_non_orth_correctors; ++no) {                                                   // :114-131
            FY_TRY(launch_ldu_grad_scalar(stream, g, p.p, gradp.p));
            FY_TRY(launch_ldu_assemble_pressure(stream, g, rAUf.p, phiHbyA.p, gradp.p, pcoef.p, pcorr.p, pt.p, pdiag.p, prhs.p));
            if (no == 0) FY_TRY(amg.setup(stream, pcoef.p, pdiag.p));          // (the non-orthogonal passes renew the right-hand side only)
            FY_TRY(solve_pressure(final_corr && no == cs.n_non_orth_correctors));
            if (no == cs.n_non_orth_correctors) FY_TRY(launch_ldu_flux_correct(stream, g, p.p, phiHbyA.p, pcoef.p, pcorr.p, phi.p));
        }
        FY_TRY(open_renew());                                                                                      // open boundaries: the mask of the new flux, before U is corrected
        FY_TRY(launch_ldu_U_correct(stream, g, HbyA.p, rAU.p, p.p, phi.p, U.p, partials.p));                     // :134-137
        double h[2];
        FY_TRY(reduce_read(nc, 2, nullptr, h));
        st.cont_err_sum_local = cs.dt * h[0] / total_volume; st.cont_err_global = cs.dt * h[1] / total_volume;
        cumulative += st.cont_err_global; st.cont_err_cumulative = cumulative;
        if (fc.on) FY_TRY(flow_correct());                                                                        // fvOptions.correct(U), after the continuity sums have left the partials
        return FY_OK;
    }


    // pEqn.H, one pass of the PISO loop inside a PIMPLE outer corrector
    int corrector_pimple(bool final_corr, double p_relax_now) {
        FY_TRY(launch_ldu_HbyA(stream, g, M(), U.p, rAU.p, HbyA.p));                                              // pEqn.H:2
        FY_TRY(launch_ldu_phiHbyA(stream, g, HbyA.p, rAU.p, Uold.p, phiOld.p, alphaf.p, rAUf.p, phiHbyA.p));    // :4-11
        if (need_ref) FY_TRY(launch_ldu_adjust_phi(stream, g, phiHbyA.p, adj.p, adj_err.p, partials.p));          // :13-16 (before phicForces are added)
        FY_TRY(launch_ldu_add_forces_constrain(stream, g, phiForces.p, rAUf.p, U.p, phiHbyA.p, psn.p));          // :18-21
        FY_TRY(launch_ldu_pim_pfaces(stream, g, alphaf.p, rAUf.p, phiHbyA.p, psn.p, arAUf.p, phiA.p));
        for (int no = 0; no <= cs.n_non_orth_correctors; ++no) {                                                   // :24-47
            FY_TRY(launch_ldu_grad_scalar(stream, g, p.p, gradp.p));
            FY_TRY(launch_ldu_assemble_pressure(stream, g, arAUf.p, phiA.p, gradp.p, pcoef.p, pcorr.p, pt.p, pdiag.p, prhs.p));
            // (fvc::ddt(alphac), :30, is zero: alphac.oldTime() == alphac -- P())
            if (no == 0) FY_TRY(amg.setup(stream, pcoef.p, pdiag.p));
            FY_TRY(solve_pressure(final_corr && no == cs.n_non_orth_correctors));
            if (no == cs.n_non_orth_correctors) {
                FY_TRY(launch_ldu_pim_flux(stream, g, p.p, phiHbyA.p, pcoef.p, pcorr.p, alphaf.p, rAUf.p, phiForces.p, psn.p, phi.p, ssf.p, pt.p));      // :39
                if (p_relax_now > 0 && p_relax_now < 1) FY_TRY(launch_relax_field(stream, p.p, pPrev.p, p_relax_now, (size_t)nc));                  // :41
            }
        }
        FY_TRY(open_renew());                                                                                      // open boundaries: the mask of the new flux, before U is reconstructed
        FY_TRY(launch_ldu_reconstruct(stream, g, ssf.p, HbyA.p, rAU.p, U.p));                                     // :43-46
        if (fc.on) FY_TRY(flow_correct());                                                                        // fvOptions.correct(Uc) (the continuity sums below read the flux, not U)
        FY_TRY(launch_ldu_pim_continuity(stream, g, pt.p, alpha.p, alpha.p, partials.p));             // :50
        double h[2];
        FY_TRY(reduce_read(nc, 2, nullptr, h));
        st.cont_err_sum_local = cs.dt * h[0] / total_volume; st.cont_err_global = cs.dt * h[1] / total_volume;
        cumulative += st.cont_err_global; st.cont_err_cumulative = cumulative;
        return FY_OK;
    }

    // pimpleFoamYade.C:60-114
    int step_pimple() {
        // The pre-coupling sweeps (1.3 ms at 4.1 M cells, bandwidth bound) on a side stream, beside the coupling's tree walk and deposit (4.3 + 1.2 ms, latency bound,
        // no fluid field read): the coupling waits for them where it first gathers a fluid field (Coupling::run_batch, pack_records: fields_event), as on z-slabs
        const bool beside = cpl->c.gaussian;
        if (beside && !side) {
            FY_HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
            FY_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming)); FY_HIP(hipEventCreateWithFlags(&ev_fields, hipEventDisableTiming));
        }
        hipStream_t ps = beside ? side : stream;
        if (beside) { FY_HIP(hipEventRecord(ev_fork, stream)); FY_HIP(hipStreamWaitEvent(side, ev_fork, 0)); }
        FY_TRY(launch_ldu_alphaf(ps, g, alpha.p, alphaf.p));
        FY_TRY(launch_ldu_pre_coupling(ps, g, phi.p, U.p, vGrad.p, alphaf.p, ddtU.p, divT.p));                  // :73, :75 (vGrad: :76, by the caller)
        FY_TRY(launch_ldu_grad_scalar(ps, g, p.p, gradP.p));                                                      // :74
        if (beside) { FY_HIP(hipEventRecord(ev_fields, side)); cpl->c.slab.fields_event = ev_fields; }
        tim[0].start(stream);
        FY_TRY(cpl->c.set_particle_action(cs.dt));                                                                // :78
        tim[0].stop(stream);
        if (beside) FY_HIP(hipStreamWaitEvent(stream, ev_fields, 0));                                             // (whatever the coupling did: the sweeps below read alphaf)
        FY_TRY(launch_ldu_alphaf(stream, g, alpha.p, alphaf.p));                                                  // :83-85
        if (th.on) FY_TRY(heat_coefficients());                                                                   // (the stencils, the cell records and U are still what the force pass saw)
        if (fc.on) FY_TRY(flow_source());                                                                         // (the first outer iteration's assembly: gradP0 += dGradP, ext + flowDir gradP0)
        if (ext_source || fc.on) FY_TRY(launch_add_f64(stream, uSource.p, fc.on ? fc.usrc.p : uSourceExt.p, 3 * (size_t)nc));
        if (th.buoyant) FY_TRY(launch_buoyancy(stream, (size_t)nc, th.T.p, th.d.beta, th.d.T_ref, cs.g, uSource.p, th.buoy.p, th.usrc_sum.p));      // P().uSource: the sum
        const int nOuter = std::max(cs.n_outer_correctors, 1);
        for (int outer = 0; outer < nOuter; ++outer) {                                                             // :90
            const bool final_outer = outer == nOuter - 1;
            const double u_relax_now = (final_outer && cs.u_relax_final > 0) ? cs.u_relax_final : cs.u_relax;
            const double p_relax_now = (final_outer && cs.p_relax_final > 0) ? cs.p_relax_final : cs.p_relax;
            if (p_relax_now > 0 && p_relax_now < 1) FY_TRY(launch_copy_f64(stream, pPrev.p, p.p, (size_t)nc));  // storePrevIterFields()
            if (outer > 0) FY_TRY(launch_ldu_grad_vec(stream, g, U.p, vGrad.p));
            if (outer > 0 && fc.on) {                                                                             // this assembly's gradP0 = the last one's + the last corrector's dGradP
                FY_TRY(flow_source(uSource.p));
                if (th.buoyant) FY_TRY(launch_buoyancy(stream, (size_t)nc, th.T.p, th.d.beta, th.d.T_ref, cs.g, uSource.p, th.buoy.p, th.usrc_sum.p));
            }
            if (g.gradL) FY_TRY(launch_ldu_grad_magsqr(stream, g, U.p, gradL.p));
            FY_TRY(launch_ldu_assemble_momentum_pimple(stream, g, P(), phi.p, Uold.p, U.p, vGrad.p, M(), pt.p, fstress.p, u_relax_now, rAU.p, por.dev()));      // UcEqn.H:3-13
            FY_TRY(launch_ldu_forces(stream, g, P(), rAU.p, rAUf.p, phiForces.p));                               // UcEqn.H:15-20
            if (cs.momentum_predictor) {                                                                          // UcEqn.H:22-33
                // (first outer iteration: p and its patches' gradients stand as when the coupling's gradP was formed, pimpleFoamYade.C:74 -- the same field, not formed again)
                if (outer > 0) FY_TRY(launch_ldu_grad_scalar(stream, g, p.p, gradp.p));
                FY_TRY(launch_ldu_ssf_predictor(stream, g, phiForces.p, rAUf.p, p.p, outer > 0 ? gradp.p : gradP.p, ssf.p));
                FY_TRY(launch_ldu_reconstruct(stream, g, ssf.p, mb.p, d_V.p, bmom.p));
                int it = 0;
                FY_TRY(solve_momentum(&it, bmom.p, nullptr));
                st.u_iters_total += it;
            }
            for (int corr = 0; corr < cs.n_correctors; ++corr) FY_TRY(corrector_pimple(final_outer && corr == cs.n_correctors - 1, p_relax_now));
            if (les && final_outer) {                                                                             // pimple.turbCorr(): pimpleFoamYade.C:101-104
                FY_TRY(launch_ldu_grad_vec(stream, g, U.p, vGrad.p));
                if (keqn || keps) {                                                                               // kEqn::correct() / kEpsilon::correct(): epsilon first, then k with the new epsilon
                    LduMom Mk = M();
                    Mk.bdiag = nullptr;
                    if (n_wall_cells) FY_TRY(launch_ldu_wall_functions(stream, g, P(), WC(), U.p, wall_eps.p, wall_G.p));       // epsilon_.boundaryFieldRef().updateCoeffs(): G and eps_w, once
                    const int modes[2] = {keps ? 1 : 0, 2};                                                       // (LduKEqn::mode) kEqn: k; kEpsilon: epsilon, then k
                    for (int mi = 0; mi < (keps ? 2 : 1); ++mi) {
                        const int mode = modes[mi];
                        LduKEqn K{};
                        K.mode = mode; K.ce = cs.les_ce; K.c1 = cs.ras_c1; K.c2 = cs.ras_c2; K.c3 = cs.ras_c3;
                        double tol, rel; int maxit;
                        if (mode == 1) { K.relax = cs.eps_relax; K.upwind = cs.eps_convection_scheme == FY_CONVECTION_UPWIND; K.sigma = cs.ras_sigmaeps; K.X = epsturb.p; K.x_bc = d_epsbc.p; K.x_val = d_epsval.p; tol = cs.eps_tol; rel = cs.eps_rel_tol; maxit = cs.eps_max_iter; }
                        else { K.relax = cs.k_relax; K.upwind = cs.k_convection_scheme == FY_CONVECTION_UPWIND; K.sigma = mode == 0 ? 1.0 : cs.ras_sigmak; K.X = kturb.p; K.x_bc = d_kbc.p; K.x_val = d_kval.p; tol = cs.k_tol; rel = cs.k_rel_tol; maxit = cs.k_max_iter; }
                        if (n_wall_cells) { K.wall_of = d_wall_of.p; K.wall_eps = wall_eps.p; K.wall_G = wall_G.p; }
                        FY_TRY(launch_ldu_grad_k(stream, g, P(), K, gradk.p));
                        FY_TRY(launch_ldu_k_assemble(stream, g, P(), K, phi.p, vGrad.p, gradk.p, Mk, fcorr.p, HbyA.p));
                        if (n_wall_cells && mode == 1) FY_TRY(launch_ldu_wall_set_values(stream, g, WC(), Mk));
                        int it = 0;
                        FY_TRY(solve_vec3(&it, Mk, mb.p, nullptr, &HbyA.p, &xscr.p, tol, rel, maxit));
                        k_iters_total += it;
                        FY_TRY(launch_ldu_k_bound_nut(stream, g, P(), K, HbyA.p, mode == 1 ? epsturb.p : kturb.p, nut.p));
                    }
                    nut_live = true;
                } else
                FY_TRY(launch_ldu_smagorinsky_nut(stream, g, vGrad.p, cs.les_ck, cs.les_ce, cs.les_delta_coeff, nut.p));
            }
        }
        return FY_OK;
    }

    int step() {
        FY_HIP(hipSetDevice(device));
        if (th.on && cpl->c.fibre)          // (before the particle phase: a refused step leaves nothing half done)
            return fail(FY_ERR_UNSUPPORTED, "fy_ldu_solver_step: heat transfer (fy_ldu_case.thermal.on) is not available with fibre coupling (fy_set_fibre_coupling): switch one of them off");
        if (ss.on && cpl->c.fibre)
            return fail(FY_ERR_UNSUPPORTED, "fy_ldu_solver_step: solid statistics (fy_ldu_solver_set_solid_statistics) are not available with fibre coupling (fy_set_fibre_coupling): switch one of them off");
        st = fy_step_stats{}; st.cont_err_cumulative = cumulative; st.delta_t = cs.dt;
        if (sources_pending) { FY_TRY(cpl->c.set_source_zero()); sources_pending = false; }      // the previous step's deferred setSourceZero
        tim[1].start(stream);
        if (!ops_courant.p) { FY_TRY(ops_courant.alloc_exact(2)); const int o[2] = {1, 0}; FY_HIP(hipMemcpyAsync(ops_courant.p, o, sizeof(o), hipMemcpyHostToDevice, stream)); FY_HIP(hipStreamSynchronize(stream)); }
        double h[2];
        FY_TRY(launch_ldu_courant(stream, g, phi.p, partials.p));                                                   // icoFoamYade.C:68
        FY_TRY(reduce_read(nc, 2, ops_courant.p, h));
        st.courant_max = 0.5 * h[0] * cs.dt; st.courant_mean = 0.5 * (h[1] / total_volume) * cs.dt;
        if (cs.adjust_time_step) {                                                                                  // setDeltaT.H (common.hpp: next_delta_t): Co from the current flux at the OLD step
            cs.dt = next_delta_t(cs.dt, st.courant_max, cs.max_co, cs.max_delta_t);
            g.dt = cs.dt;
        }
        st.delta_t = cs.dt;
        if (inl.on()) FY_TRY(inl.update(stream, (inl.start_time + mon.elapsed) + cs.dt, uFace.p));                  // the inlets' value at the time this step advances to, before any kernel reads it
        stepped = true;                    // (from here on the fields move: set_inlets refuses)
        FY_HIP(hipMemcpyAsync(Uold.p, U.p, 3 * (size_t)nc * sizeof(double), hipMemcpyDeviceToDevice, stream));    // runTime++: old-time fields
        FY_HIP(hipMemcpyAsync(phiOld.p, phi.p, (size_t)nf * sizeof(double), hipMemcpyDeviceToDevice, stream));
        FY_TRY(open_renew());                                                                                      // open boundaries: the mask of the old time's flux, before any kernel reads it
        FY_TRY(launch_ldu_grad_vec(stream, g, U.p, vGrad.p));                                                      // :71
        if (pimple) FY_TRY(step_pimple());
        else {
            tim[0].start(stream);
            FY_TRY(cpl->c.set_particle_action(cs.dt));                                                                // :74
            tim[0].stop(stream);
            if (th.on) FY_TRY(heat_coefficients());
            // the momentum source: what the coupling left (+ an external one, fy_ldu_solver_write_field_host("uSource", ...)) (+ the buoyancy of the T the step found)
            const double* src = uSource.p;
            if (fc.on) FY_TRY(flow_source());                                                                         // gradP0 += dGradP, ext + flowDir gradP0
            if (ext_source || fc.on) { FY_TRY(launch_copy_f64(stream, uSourceSum.p, uSource.p, 3 * (size_t)nc)); FY_TRY(launch_add_f64(stream, uSourceSum.p, fc.on ? fc.usrc.p : uSourceExt.p, 3 * (size_t)nc)); src = uSourceSum.p; }
            if (th.buoyant) { FY_TRY(launch_buoyancy(stream, (size_t)nc, th.T.p, th.d.beta, th.d.T_ref, cs.g, src, th.buoy.p, th.usrc_sum.p)); src = th.usrc_sum.p; }
            if (g.gradL) FY_TRY(launch_ldu_grad_magsqr(stream, g, Uold.p, gradL.p));
            FY_TRY(launch_ldu_assemble_momentum(stream, g, phi.p, Uold.p, src, vGrad.p, M(), fcorr.p, por.dev()));     // :79-85 (grad U of the iterate it is assembled from = vGrad)
            if (cs.momentum_predictor) {
                FY_TRY(launch_ldu_grad_scalar(stream, g, p.p, gradp.p));
                int it = 0;
                FY_TRY(solve_momentum(&it, mb.p, gradp.p));                                                          // :91-94
                st.u_iters_total += it;
            }
            for (int corr = 0; corr < cs.n_correctors; ++corr) FY_TRY(corrector(corr == cs.n_correctors - 1));         // :97-140
        }
        if (th.on) FY_TRY(solve_temperature());                                                                   // after the last corrector and the turbulence model's correct()
        if (ss.on) FY_TRY(ss.pass(cpl->c, stream, CellWindow{0, (int64_t)nc}, d_V.p, th.on ? &th.part : nullptr, false));      // Tp: the end-of-step temperatures
        avg.elapsed += cs.dt;
        if (avg.on()) FY_TRY(avg.sample(stream, cs.dt, [this](const std::string& nm, int* comp) { return avg_source(nm, comp); }));
        mon.elapsed += cs.dt;
        if (mon.on()) FY_TRY(mon.sample(stream, g.V, 0.0, [this](const std::string& nm, int* comp) { return avg_source(nm, comp); },
                                        [this](const MonFaceTable& t, double* pf, int nblk) { return launch_ldu_monitor_faces(stream, g, t, p.p, U.p, th.eq, phi.p, pf, nblk); }));
        if (wl.on()) FY_TRY(wl.sample(stream, wl.start_time + mon.elapsed, [this](const WlTable& t, double* pf, int nblk, double* wss, double* yplus) {
            return launch_ldu_wall_loads(stream, g, pimple ? P() : LduPim{}, t, p.p, U.p, d_ywall.p, wss, yplus, pf, nblk); }));
        if (hold_sources) sources_pending = true;                                                                 // runTime.write() comes before setSourceZero (icoFoamYade.C:142-147)
        else FY_TRY(cpl->c.set_source_zero());                                                                    // :147
        tim[1].stop(stream);
        FY_HIP(hipStreamSynchronize(stream));
        if (need_ref) {
            int e = 0;
            FY_HIP(hipMemcpy(&e, adj_err.p, sizeof(int), hipMemcpyDeviceToHost));
            if (e) return fail(FY_ERR_UNSUPPORTED, "adjustPhi: continuity error cannot be removed by adjusting the outflow -- OpenFOAM stops here too");
        }
        st.ms_particle = tim[0].ms(); st.ms_total = tim[1].ms();
        if (ss.on) ss.clock.collect();
        if (fc.on) fc.clock.collect();
        if (wl.on()) wl.m.clock.collect();
        if (inl.on()) inl.clock.collect();
        if (ob.on) ob.clock.collect();
        return FY_OK;
    }

    int field(const char* name, double** ptr, size_t* count, const std::vector<double>** host) {
        const std::string s = name ? name : "";
        *host = nullptr;
        const size_t n = (size_t)nc;
        struct E { const char* nm; double* p; size_t c; };
        const E tab[] = {{"U", U.p, 3 * n}, {"p", p.p, n}, {"phi", phi.p, (size_t)nf}, {"uSource", uSourceExt.p, 3 * n}, {"rAU", rAU.p, n}, {"HbyA", HbyA.p, 3 * n},
                         {"phiHbyA", phiHbyA.p, (size_t)nf}, {"p_diag", pdiag.p, n}, {"p_coef", pcoef.p, (size_t)nf}, {"p_rhs", prhs.p, n}, {"vGrad", vGrad.p, 9 * n},
                         {"mom_diag", mdiag.p, n}, {"mom_lower", mlower.p, (size_t)ni}, {"mom_upper", mupper.p, (size_t)ni}, {"mom_b", mb.p, 3 * n},
                         {"alpha", alpha.p, pimple ? n : 0}, {"uSourceDrag", uSourceDrag.p, pimple ? n : 0}, {"uParticle", uParticle.p, pimple ? 3 * n : 0}, {"gradP", gradP.p, pimple ? 3 * n : 0},
                         {"divT", divT.p, pimple ? 3 * n : 0}, {"ddtU", ddtU.p, pimple ? 3 * n : 0}, {"phiForces", phiForces.p, pimple ? (size_t)nf : 0}, {"alphaf", alphaf.p, pimple ? (size_t)nf : 0},
                         {"rAUf", rAUf.p, (size_t)nf}, {"uSourceCoupling", uSource.p, 3 * n}, {"nut", nut.p, les ? n : 0}, {"k", kturb.p, (keqn || keps) ? n : 0}, {"epsilon", epsturb.p, keps ? n : 0}};
        for (const E& e : tab) if (s == e.nm) { *ptr = e.p; *count = e.c; return FY_OK; }
        if (avg.lookup(s, ptr, count)) return FY_OK;                           // <field>Mean, <field>Prime2Mean
        if (ss.on && SolidStats::is_name(s)) {                                 // solidMoments and the six fields (read-only); unknown names while the feature is off
            FY_HIP(hipSetDevice(device));
            return ss.field(s, stream, ptr, count);
        }
        if (s == "T" || s == "heatSp" || s == "heatSu") {
            if (!th.on) return fail(FY_ERR_INVALID, "fy_ldu_solver field '%s' does not exist in this case (fy_ldu_case.thermal is off)", s.c_str());
            *ptr = s == "T" ? th.T.p : s == "heatSp" ? th.Sp.p : th.Su.p; *count = n;
            return FY_OK;
        }
        if (s == "buoyancy") {
            if (!th.buoyant) return fail(FY_ERR_INVALID, "fy_ldu_solver field 'buoyancy' does not exist in this case (fy_ldu_case.thermal.beta or g is zero)");
            *ptr = th.buoy.p; *count = 3 * n;
            return FY_OK;
        }
        if (s == "p_boundary" || s == "U_boundary" || s == "T_boundary") {         // formed on request: the boundary values as pbv / Ub / ldu_T_b give them now
            if (s == "T_boundary" && !th.on) return fail(FY_ERR_INVALID, "fy_ldu_solver field 'T_boundary' does not exist in this case (fy_ldu_case.thermal is off)");
            const size_t nb = (size_t)(nf - ni);
            DevBuf<double>& b = s == "p_boundary" ? bndP : s == "U_boundary" ? bndU : bndT;
            *count = s == "U_boundary" ? 3 * nb : nb;
            FY_HIP(hipSetDevice(device));
            if (!b.p) FY_TRY(b.alloc_exact(std::max<size_t>(*count, 1)));
            FY_TRY(launch_ldu_boundary_values(stream, g, p.p, U.p, th.eq, s == "p_boundary" ? b.p : nullptr, s == "U_boundary" ? b.p : nullptr, s == "T_boundary" ? b.p : nullptr));
            *ptr = b.p;
            return FY_OK;
        }
        if (s == "U_open_inflow") {                                                // the inflow mask as doubles (0 | 1), as the last renewal left it
            if (!ob.on) return fail(FY_ERR_INVALID, "fy_ldu_solver field 'U_open_inflow' does not exist in this case (no patch carries an open code)");
            *count = (size_t)(nf - ni);
            FY_HIP(hipSetDevice(device));
            if (!ob.f64.p) FY_TRY(ob.f64.alloc_exact(std::max<size_t>(*count, 1)));
            FY_TRY(launch_ldu_open_mask_f64(stream, nf - ni, ob.mask.p, ob.f64.p));
            *ptr = ob.f64.p;
            return FY_OK;
        }
        if (por.on() && (s == "porousZone" || s == "mom_bd")) {                     // read-only; unknown names without a zone
            FY_HIP(hipSetDevice(device));
            if (s == "porousZone") return por.zone_field(stream, nc, ptr, count);
            *ptr = mbdiag.p; *count = 3 * n;                                       // symmetry patches + zones, as the last assembly left it
            return FY_OK;
        }
        if (wl.lookup(s, ptr, count)) return FY_OK;                                // wallShearStress_boundary, yPlus_boundary as the last sample left them
        if (s == "nut_boundary") {                                                 // formed on request: nut_b as ldu_nut_b gives it now
            *count = les ? (size_t)(nf - ni) : 0;
            if (*count) {
                FY_HIP(hipSetDevice(device));
                if (!nutBnd.p) FY_TRY(nutBnd.alloc_exact(*count));
                FY_TRY(launch_ldu_nut_boundary(stream, g, P(), nutBnd.p));
            }
            *ptr = nutBnd.p;
            return FY_OK;
        }
        const struct { const char* nm; const std::vector<double>* v; } geo[] = {{"C", &hm.C}, {"V", &hm.V}, {"Cf", &hm.Cf}, {"Sf", &hm.Sf}, {"magSf", &hm.magSf}, {"w", &hm.w},
                                                                                  {"dcNO", &hm.dcNO}, {"kvec", &hm.kvec}, {"sep", &hm.sep}, {"orig_face", &orig_face_d},
                                                                                  {"nearWallDist", &ywall}};
        for (const auto& e : geo) if (s == e.nm) { *host = e.v; *count = e.v->size(); *ptr = nullptr; return FY_OK; }
        return fail(FY_ERR_INVALID, "unknown fy_ldu_solver field '%s'", s.c_str());
    }
};

}  // namespace fy

struct fy_ldu_solver { fy::LduSolver s; };

extern "C" {

void fy_ldu_case_defaults(fy_ldu_case* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->dt = 0.005; c->nu = 0.01; c->rho_fluid = 1000.0; c->rho_particle = 2650.0;
    c->n_correctors = 2; c->n_non_orth_correctors = 0; c->momentum_predictor = 1; c->p_ref_cell = 0; c->p_ref_value = 0.0;
    c->p_tol = 1e-6; c->p_rel_tol = 0.05; c->p_final_tol = 1e-6; c->p_final_rel_tol = 0.0; c->p_max_iter = 1000;
    c->u_tol = 1e-5; c->u_rel_tol = 0.0; c->u_max_iter = 1000;
    c->p_solver = FY_PSOLVER_PCG_JACOBI;
    c->solver = FY_SOLVER_ICO; c->n_outer_correctors = 1;
    c->adjust_time_step = 0; c->max_co = 1.0; c->max_delta_t = 1e300;
    c->turbulence_model = FY_TURBULENCE_LAMINAR; c->les_ck = 0.094; c->les_ce = 1.048; c->les_delta_coeff = 1.0; c->nut_initial = 0.0;
    c->convection_scheme = FY_CONVECTION_LINEAR; c->convection_limiter_k = 1.0;
    c->ras_cmu = 0.09; c->ras_c1 = 1.44; c->ras_c2 = 1.92; c->ras_c3 = 0.0; c->ras_sigmak = 1.0; c->ras_sigmaeps = 1.3;
    c->eps_initial = 0.0; c->eps_bc = nullptr; c->eps_value = nullptr; c->eps_convection_scheme = FY_CONVECTION_LINEAR; c->eps_tol = 1e-6; c->eps_rel_tol = 0.0; c->eps_max_iter = 1000; c->eps_relax = 0.0;
    c->k_initial = 0.0; c->k_bc = nullptr; c->k_value = nullptr; c->k_convection_scheme = FY_CONVECTION_LINEAR; c->k_tol = 1e-6; c->k_rel_tol = 0.0; c->k_max_iter = 1000; c->k_relax = 0.0;
    c->wf_kappa = 0.41; c->wf_E = 9.8;
}

int fy_ldu_solver_create(const fy_poly_mesh* m, const fy_ldu_case* c, const fy_transport* tr, int device_ordinal, fy_ldu_solver** out) {
    if (!out) return fy::fail(FY_ERR_INVALID, "null out");
    *out = nullptr;
    fy_ldu_solver* s = new (std::nothrow) fy_ldu_solver();
    if (!s) return fy::fail(FY_ERR_INVALID, "out of host memory");
    const int rc = s->s.create(m, c, tr, device_ordinal);
    if (rc != FY_OK) { delete s; return rc; }
    *out = s;
    return FY_OK;
}
#define FY_LS(s) if (!(s)) return fy::fail(FY_ERR_INVALID, "null fy_ldu_solver")
int fy_ldu_solver_step(fy_ldu_solver* s) { FY_LS(s); return s->s.step(); }
int fy_ldu_solver_get_stats(fy_ldu_solver* s, fy_step_stats* out) { FY_LS(s); if (!out) return fy::fail(FY_ERR_INVALID, "null out"); *out = s->s.st; return FY_OK; }
fy_ctx* fy_ldu_solver_coupling(fy_ldu_solver* s) { return s ? s->s.cpl : nullptr; }
int fy_ldu_solver_field_count(fy_ldu_solver* s, const char* name, int64_t* count) {
    FY_LS(s);
    if (!count) return fy::fail(FY_ERR_INVALID, "null count");
    double* p; size_t n; const std::vector<double>* h;
    FY_TRY(s->s.field(name, &p, &n, &h));
    *count = (int64_t)n;
    return FY_OK;
}
int fy_ldu_solver_read_field_host(fy_ldu_solver* s, const char* name, double* out) {
    FY_LS(s);
    double* p; size_t n; const std::vector<double>* h;
    FY_TRY(s->s.field(name, &p, &n, &h));
    if (h) { std::memcpy(out, h->data(), n * sizeof(double)); return FY_OK; }
    FY_HIP(hipSetDevice(s->s.device));
    FY_HIP(hipMemcpyAsync(out, p, n * sizeof(double), hipMemcpyDeviceToHost, s->s.stream));
    FY_HIP(hipStreamSynchronize(s->s.stream));
    return FY_OK;
}
int fy_ldu_solver_write_field_host(fy_ldu_solver* s, const char* name, const double* in) {
    FY_LS(s);
    double* p; size_t n; const std::vector<double>* h;
    FY_TRY(s->s.field(name, &p, &n, &h));
    const std::string nm = name;
    {
        double* ap; size_t an;
        if (!h && s->s.avg.lookup(nm, &ap, &an)) {             // a restart loading an average: a plain copy, nothing of the solver's state follows from it
            FY_HIP(hipSetDevice(s->s.device));
            FY_HIP(hipMemcpyAsync(p, in, n * sizeof(double), hipMemcpyHostToDevice, s->s.stream));
            FY_HIP(hipStreamSynchronize(s->s.stream));
            return FY_OK;
        }
    }
    const bool pim_in = (s->s.pimple && (nm == "alpha" || nm == "uSourceDrag")) || (s->s.les && nm == "nut") || ((s->s.keqn || s->s.keps) && nm == "k") || (s->s.keps && nm == "epsilon") || (s->s.th.on && nm == "T");      // (what setParticleAction would leave: for tests that feed the equations a given void fraction)
    if (h || (nm != "U" && nm != "p" && nm != "uSource" && !pim_in)) return fy::fail(FY_ERR_INVALID, "fy_ldu_solver_write_field_host: '%s' cannot be written (U, p, uSource; alpha, uSourceDrag with pimpleFoamYade; T with heat transfer on)", nm.c_str());
    FY_HIP(hipSetDevice(s->s.device));
    FY_HIP(hipMemcpyAsync(p, in, n * sizeof(double), hipMemcpyHostToDevice, s->s.stream));
    if (nm == "uSource") s->s.ext_source = true;
    if (nm == "U") FY_TRY(s->s.create_phi());      // createPhi
    FY_HIP(hipStreamSynchronize(s->s.stream));
    return FY_OK;
}
int fy_ldu_solver_apply(fy_ldu_solver* s, const char* op, const double* in, double* out) {
    FY_LS(s);
    if (!op || !in || !out) return fy::fail(FY_ERR_INVALID, "fy_ldu_solver_apply: null argument");
    fy::LduSolver& S = s->s;
    const std::string o = op;
    const bool mat = o == "p_matrix", pre = o == "p_precondition";
    if (!mat && !pre) return fy::fail(FY_ERR_INVALID, "fy_ldu_solver_apply: unknown operator '%s' (p_matrix, p_precondition)", op);
    if (!S.amg.diag0_) return fy::fail(FY_ERR_INVALID, "fy_ldu_solver_apply: no pressure matrix yet (step first)");
    FY_HIP(hipSetDevice(S.device));
    const size_t bytes = (size_t)S.nc * sizeof(double);
    FY_HIP(hipMemcpyAsync(S.pr.p, in, bytes, hipMemcpyHostToDevice, S.stream));
    if (mat) {
        fy::EllMat A = S.amg.lev[0]->mat();
        A.diag = S.pdiag.p;
        FY_TRY(fy::launch_ell_apply_dot(S.stream, A, S.pr.p, S.pr.p, S.pw.p, S.partials.p));
    } else if (S.amg.has_hierarchy()) FY_TRY(S.amg.vcycle(S.stream, S.pr.p, S.pw.p));
    else FY_TRY(fy::launch_ell_jacobi(S.stream, S.nc, S.pdiag.p, S.pr.p, S.pw.p));
    FY_HIP(hipMemcpyAsync(out, S.pw.p, bytes, hipMemcpyDeviceToHost, S.stream));
    FY_HIP(hipStreamSynchronize(S.stream));
    return FY_OK;
}
int fy_ldu_solver_set_field_average(fy_ldu_solver* s, const fy_average_desc* d) { FY_LS(s); return s->s.set_field_average(d); }
int fy_ldu_solver_get_average_state(fy_ldu_solver* s, int item, int64_t* samples, double* time_averaged) { FY_LS(s); return s->s.avg.get_state(item, samples, time_averaged); }
int fy_ldu_solver_set_average_state(fy_ldu_solver* s, int item, int64_t samples, double time_averaged) { FY_LS(s); return s->s.avg.set_state(item, samples, time_averaged); }
int fy_ldu_solver_set_solid_statistics(fy_ldu_solver* s, int on) { FY_LS(s); return s->s.set_solid_statistics(on); }
int fy_ldu_solver_enable_kernel_timing(fy_ldu_solver* s, int on) {
    FY_LS(s);
    s->s.ss.clock.reset(); s->s.ss.clock.on = on != 0;
    s->s.fc.clock.reset(); s->s.fc.clock.on = on != 0;
    s->s.wl.m.clock.reset(); s->s.wl.m.clock.on = on != 0;
    s->s.inl.clock.reset(); s->s.inl.clock.on = on != 0;
    s->s.ob.clock.reset(); s->s.ob.clock.on = on != 0;
    s->s.por.clock.reset(); s->s.por.clock.on = on != 0;
    return FY_OK;
}
int fy_ldu_solver_get_kernel_timing(fy_ldu_solver* s, const char* kernel, double* total_ms, int64_t* launches) {
    FY_LS(s);
    const std::string k = kernel ? kernel : "";
    if (k == "wall_loads" && s->s.wl.on() && total_ms && launches) { *total_ms = s->s.wl.m.clock.total_ms; *launches = s->s.wl.m.clock.launches; return FY_OK; }
    if (k == "open_boundary" && total_ms && launches) { *total_ms = s->s.ob.clock.total_ms; *launches = s->s.ob.clock.launches; return FY_OK; }      // (no open patch: no launch)
    if (k == "porous_force" && total_ms && launches) { *total_ms = s->s.por.clock.total_ms; *launches = s->s.por.clock.launches; return FY_OK; }      // (no zone: no launch)
    if (k == "inlets" && s->s.inl.on() && total_ms && launches) { *total_ms = s->s.inl.clock.total_ms; *launches = s->s.inl.clock.launches; return FY_OK; }
    const bool flow = k == "flow_control" && s->s.fc.on;
    if ((k != "solid_stats" && !flow) || !total_ms || !launches) return fy::fail(FY_ERR_INVALID, "unknown kernel clock '%s' (solid_stats, open_boundary%s%s%s)", k.c_str(), s->s.fc.on ? ", flow_control" : "", s->s.wl.on() ? ", wall_loads" : "", s->s.inl.on() ? ", inlets" : "");
    const fy::KernelClock& c = flow ? s->s.fc.clock : s->s.ss.clock;
    *total_ms = c.total_ms; *launches = c.launches;
    return FY_OK;
}
int fy_ldu_solver_set_flow_control(fy_ldu_solver* s, const fy_flow_control_desc* d) { FY_LS(s); return s->s.set_flow_control(d, "fy_ldu_solver_set_flow_control"); }
int fy_ldu_solver_get_flow_control(fy_ldu_solver* s, double* gradient, double* ubar_uncorrected, double* rAU_ave, double* dGradP, int64_t* corrections) {
    FY_LS(s);
    return s->s.get_flow_control(gradient, ubar_uncorrected, rAU_ave, dGradP, corrections);
}
int fy_ldu_solver_set_porous_zones(fy_ldu_solver* s, const fy_porous_desc* d) { FY_LS(s); return s->s.set_porous_zones(d); }
int fy_ldu_solver_get_porous_stats(fy_ldu_solver* s, int32_t* n_zones, int64_t* cells, double* volume, double* void_volume, double* force) {
    FY_LS(s);
    return s->s.porous_stats(n_zones, cells, volume, void_volume, force);
}
int fy_ldu_solver_get_open_boundary_stats(fy_ldu_solver* s, int64_t* inflow_faces, double* inflow_flux, double* outflow_flux) { FY_LS(s); return s->s.get_open_stats(inflow_faces, inflow_flux, outflow_flux); }
int fy_ldu_solver_set_monitors(fy_ldu_solver* s, const fy_monitor_desc* d) { FY_LS(s); return s->s.set_monitors(d); }
int fy_ldu_solver_monitor_layout(fy_ldu_solver* s, int object, int32_t* n_values, char* labels, int cap) { FY_LS(s); return s->s.mon.layout(object, n_values, labels, cap); }
int fy_ldu_solver_get_monitor_rows(fy_ldu_solver* s, int object, int64_t first_row, int64_t max_rows, double* times, double* values, int64_t* n_rows) {
    FY_LS(s);
    FY_HIP(hipSetDevice(s->s.device));
    return s->s.mon.get_rows(s->s.stream, object, first_row, max_rows, times, values, n_rows);
}
int fy_ldu_solver_set_wall_loads(fy_ldu_solver* s, const fy_wall_loads_desc* d) { FY_LS(s); return s->s.set_wall_loads(d); }
int fy_ldu_solver_set_inlets(fy_ldu_solver* s, const fy_inlets_desc* d) { FY_LS(s); return s->s.set_inlets(d, "fy_ldu_solver_set_inlets"); }
int fy_ldu_solver_wall_loads_layout(fy_ldu_solver* s, int object, int32_t* n_values, char* labels, int cap) { FY_LS(s); return s->s.wl.m.layout(object, n_values, labels, cap); }
int fy_ldu_solver_get_wall_load_rows(fy_ldu_solver* s, int object, int64_t first_row, int64_t max_rows, double* times, double* values, int64_t* n_rows) {
    FY_LS(s);
    FY_HIP(hipSetDevice(s->s.device));
    return s->s.wl.m.get_rows(s->s.stream, object, first_row, max_rows, times, values, n_rows);
}
int fy_ldu_solver_set_particle_temperatures_host(fy_ldu_solver* s, int batch, const double* Tp) { FY_LS(s); return s->s.th.part.set_temperatures(s->s.cpl->c, s->s.device, s->s.stream, batch, Tp, false); }
int fy_ldu_solver_set_particle_temperatures_device(fy_ldu_solver* s, int batch, const double* d_Tp) { FY_LS(s); return s->s.th.part.set_temperatures(s->s.cpl->c, s->s.device, s->s.stream, batch, d_Tp, true); }
int fy_ldu_solver_get_particle_heat_host(fy_ldu_solver* s, int batch, double* q) { FY_LS(s); return s->s.th.part.get_heat(s->s.device, s->s.stream, batch, q); }
int fy_ldu_solver_get_particle_thermal_state(fy_ldu_solver* s, int batch, double* Tp, int64_t* resets) { FY_LS(s); return s->s.th.part.get_state(s->s.cpl->c, s->s.device, s->s.stream, batch, Tp, resets); }
int fy_ldu_solver_get_thermal_stats(fy_ldu_solver* s, int32_t* iterations, double* initial_residual, double* heat_to_particles_W) {
    FY_LS(s);
    fy::LduSolver& S = s->s;
    if (!S.th.on) return S.th.part.refuse_off("get_thermal_stats");
    if (iterations) *iterations = S.th.iters;
    if (initial_residual) *initial_residual = S.th.res0;
    if (heat_to_particles_W) FY_TRY(S.th.part.total_heat(S.device, S.stream, heat_to_particles_W));
    return FY_OK;
}
int fy_ldu_solver_get_particle_cells_host(fy_ldu_solver* s, int32_t* out_cells) {
    FY_LS(s);
    FY_HIP(hipSetDevice(s->s.device));
    return s->s.cpl->c.get_particle_cells_host(0, out_cells, "fy_ldu_solver_get_particle_cells_host");
}
int fy_ldu_solver_hold_sources(fy_ldu_solver* s, int on) { FY_LS(s); s->s.hold_sources = on != 0; return FY_OK; }
int fy_ldu_solver_mg_levels(fy_ldu_solver* s, int cap, int32_t* cells, int32_t* slots, int* n_levels) {
    FY_LS(s);
    if (!n_levels) return fy::fail(FY_ERR_INVALID, "fy_ldu_solver_mg_levels: null n_levels");
    const fy::LduAmg& A = s->s.amg;
    *n_levels = A.has_hierarchy() ? (int)A.lev.size() : 0;
    for (int l = 0; l < *n_levels && l < cap; ++l) { if (cells) cells[l] = A.lev[(size_t)l]->n; if (slots) slots[l] = A.lev[(size_t)l]->W; }
    return FY_OK;
}
int fy_ldu_solver_mg_level_read(fy_ldu_solver* s, int level, const char* what, int64_t cap, double* out, int64_t* count) {
    FY_LS(s);
    if (!what || !count) return fy::fail(FY_ERR_INVALID, "fy_ldu_solver_mg_level_read: null argument");
    fy::LduSolver& S = s->s;
    const fy::LduAmg& A = S.amg;
    if (!A.has_hierarchy() || level < 0 || (size_t)level >= A.lev.size()) return fy::fail(FY_ERR_INVALID, "fy_ldu_solver_mg_level_read: no level %d (the hierarchy has %d)", level, A.has_hierarchy() ? (int)A.lev.size() : 0);
    const fy::AmgLevel& L = *A.lev[(size_t)level];
    const bool last = (size_t)level + 1 == A.lev.size();
    const std::string w = what;
    const double* dp = nullptr; const int32_t* ip = nullptr; size_t n = 0;
    if (w == "diag") { dp = level == 0 ? S.pdiag.p : L.diag.p; n = (size_t)L.n; }
    else if (w == "coef") { dp = L.coef.p; n = (size_t)L.W * L.n; }
    else if (w == "inv") { dp = A.coarse_inv.p; n = last ? (size_t)L.n * L.n : 0; }
    else if (w == "nbr") { ip = L.nbr.p; n = (size_t)L.W * L.n; }
    else if (w == "agg") { ip = L.agg.p; n = last ? 0 : (size_t)L.n; }
    else return fy::fail(FY_ERR_INVALID, "fy_ldu_solver_mg_level_read: unknown array '%s' (diag, coef, nbr, agg, inv)", what);
    *count = (int64_t)n;
    if (!out || n == 0) return FY_OK;
    if (cap < (int64_t)n) return fy::fail(FY_ERR_INVALID, "fy_ldu_solver_mg_level_read: '%s' of level %d holds %lld values, the buffer %lld", what, level, (long long)n, (long long)cap);
    if (dp && !A.diag0_) return fy::fail(FY_ERR_INVALID, "fy_ldu_solver_mg_level_read: no pressure matrix yet (step first)");
    FY_HIP(hipSetDevice(S.device));
    if (dp) {
        FY_HIP(hipMemcpyAsync(out, dp, n * sizeof(double), hipMemcpyDeviceToHost, S.stream));
        FY_HIP(hipStreamSynchronize(S.stream));
    } else {
        std::vector<int32_t> h(n);
        FY_HIP(hipMemcpyAsync(h.data(), ip, n * sizeof(int32_t), hipMemcpyDeviceToHost, S.stream));
        FY_HIP(hipStreamSynchronize(S.stream));
        for (size_t q = 0; q < n; ++q) out[q] = (double)h[q];
    }
    return FY_OK;
}
int fy_ldu_solver_destroy(fy_ldu_solver* s) { delete s; return FY_OK; }

}  // extern "C"
