// fy::Solver's heat exchange: the fluid temperature equation and the particles' share of it (fy_thermal_desc, Thermal in fv_solver.hpp).  Not in the
// reference; DESIGN.md section 3 "heat exchange", DESIGN_FV.md "T equation".  Host code only sequences the kernels of particle_heat.hip (k_heat_coeff_*,
// k_heat_flux_*) and fv_kernels.hip (k_assemble_scalar) on the solver's stream.
#include "fv_solver.hpp"

namespace fy {

int Solver::thermal_create(const fy_case_desc* c) {
    const fy_thermal_desc& d = c->thermal;
    if (!(d.cp > 0) || !(d.kappa > 0)) return fail(FY_ERR_INVALID, "fy_solver_create: thermal needs cp > 0 and kappa > 0 (got %g, %g)", d.cp, d.kappa);
    if (d.prt < 0) return fail(FY_ERR_INVALID, "fy_solver_create: thermal.prt must not be negative");
    if (d.nusselt_law != FY_NUSSELT_RANZ_MARSHALL && d.nusselt_law != FY_NUSSELT_GUNN)
        return fail(FY_ERR_UNSUPPORTED, "fy_solver_create: unknown thermal.nusselt_law %d (FY_NUSSELT_RANZ_MARSHALL, FY_NUSSELT_GUNN)", d.nusselt_law);
    if (d.nusselt_law == FY_NUSSELT_GUNN && !pimple)
        return fail(FY_ERR_UNSUPPORTED, "fy_solver_create: thermal.nusselt_law FY_NUSSELT_GUNN needs the void fraction of the Gaussian mode (pimpleFoamYade); "
                                        "point-force mode (icoFoamYade) takes FY_NUSSELT_RANZ_MARSHALL");
    if (d.T_convection_scheme != FY_CONVECTION_LINEAR && d.T_convection_scheme != FY_CONVECTION_UPWIND)
        return fail(FY_ERR_UNSUPPORTED, "fy_solver_create: thermal.T_convection_scheme must be FY_CONVECTION_LINEAR or FY_CONVECTION_UPWIND");
    // (with both tolerances zero the residual test `res < tol` never holds -- the two idle components' residuals are exactly 0 -- and every step would run T_max_iter passes;
    //  with no pass allowed T would never move)
    if (!(d.T_tol >= 0) || !(d.T_rel_tol >= 0) || !(d.T_tol > 0 || d.T_rel_tol > 0) || d.T_max_iter < 1)
        return fail(FY_ERR_INVALID, "fy_solver_create: thermal needs T_tol >= 0 and T_rel_tol >= 0 with at least one of them positive, and T_max_iter >= 1 (got %g, %g, %d)", d.T_tol, d.T_rel_tol,
                    d.T_max_iter);
    if (!(d.particle_cp >= 0)) return fail(FY_ERR_INVALID, "fy_solver_create: thermal.particle_cp must not be negative (got %g; 0: the caller owns the particle temperatures)", d.particle_cp);
    if (d.particle_cp > 0 && !(c->rho_particle > 0))
        return fail(FY_ERR_INVALID, "fy_solver_create: thermal.particle_cp %g needs rho_particle > 0 for the particles' heat capacity (got %g)", d.particle_cp, c->rho_particle);
    if (!std::isfinite(d.beta) || !std::isfinite(d.T_ref)) return fail(FY_ERR_INVALID, "fy_solver_create: thermal.beta and thermal.T_ref must be finite (got %g, %g)", d.beta, d.T_ref);
    th.d = d;
    th.eq = ScalarEqn{};
    th.eq.upwind = d.T_convection_scheme == FY_CONVECTION_UPWIND ? 1 : 0;
    for (int q = 0; q < 6; ++q) {
        if (d.T_bc[q] != FY_BC_T_ZERO_GRADIENT && d.T_bc[q] != FY_BC_T_FIXED_VALUE)
            return fail(FY_ERR_UNSUPPORTED, "fy_solver_create: unknown thermal.T_bc %d on side %d (FY_BC_T_ZERO_GRADIENT, FY_BC_T_FIXED_VALUE)", d.T_bc[q], q);
        th.eq.bc[q] = d.T_bc[q]; th.eq.val[q] = d.T_value[q];
    }
    th.eq.D = d.kappa / (c->rho_fluid * d.cp);
    th.eq.rPrt = 1.0 / (d.prt > 0 ? d.prt : 1.0);
    th.eq.rRhoCp = 1.0 / (c->rho_fluid * d.cp);
    const double Pr = c->nu * c->rho_fluid * d.cp / d.kappa;
    th.own_tp = d.particle_cp > 0;
    th.hp = HeatParams{c->nu, 1e-09, d.kappa, std::cbrt(Pr), d.particle_temperature, d.nusselt_law, c->dt, c->rho_particle * d.particle_cp};      // (small: the force laws', ForceParams)
    DevBuf<double>* bs[] = {&th.T, &th.Sp, &th.Su};
    for (auto* b : bs) { FY_TRY(b->alloc_exact(nstore)); FY_TRY(zero(*b)); }
    FY_TRY(launch_fill_f64(stream, th.T.p, nstore, d.T_initial));
    th.buoyant = d.beta != 0.0 && (c->g[0] != 0.0 || c->g[1] != 0.0 || c->g[2] != 0.0);
    if (th.buoyant) { FY_TRY(th.buoy.alloc_exact(3 * nstore)); FY_TRY(zero(th.buoy)); FY_TRY(th.usrc_sum.alloc_exact(3 * nstore)); FY_TRY(zero(th.usrc_sum)); }
    FY_HIP(hipStreamSynchronize(stream));
    th.on = true;
    return FY_OK;
}

// pass A, once per batch, on the solver's stream right after setParticleAction returned
int Solver::heat_coefficients() {
    Coupling& C = cpl->c;
    FY_TRY(zero(th.Sp)); FY_TRY(zero(th.Su));
    const CellWindow cw{0, (int64_t)nstore};
    th.hp.dt = cs.dt;                                          // (the step's own delta_t: adjust_time_step)
    for (size_t bi = (size_t)C.n_batches; bi < th.pb.size(); ++bi) th.pb[bi]->n = 0;      // (batches that are gone)
    th.clk_coeff.begin(stream);
    for (int bi = 0; bi < C.n_batches; ++bi) {
        Batch& b = *C.batches[(size_t)bi];
        Thermal::PerBatch& t = th.batch((size_t)bi);
        t.n = b.n;
        if (b.n == 0) continue;
        FY_TRY(t.hA.reserve((size_t)b.n)); FY_TRY(t.q.reserve((size_t)b.n));
        sync_particle_temperatures((size_t)bi, b.n);           // another population: the uniform temperature again
        if (th.own_tp && !t.has_tp) {                          // the batch's first step: the array the library advances from here on
            FY_TRY(t.Tp.reserve((size_t)b.n));
            FY_TRY(launch_fill_f64(stream, t.Tp.p, (size_t)b.n, th.hp.tp_uniform));
            t.has_tp = true; t.tp_n = b.n;
        }
        const double* tp = t.has_tp ? t.Tp.p : nullptr;
        if (C.gaussian) {
            // the momentum back-scatter's buckets, with the capacities formed from the demand its pass has just counted (k_tile_caps on the side stream at the end of
            // run_batch, demand counters back at zero): the heat scatter has the same (workgroup, cell) pattern, so it fits -- from a population's first step on.  Every
            // Gaussian batch of a structured block has them (Coupling::ensure_batch, the side stream of Coupling::create); anything else is a state this pass was not
            // written for, and flushing into capacities of unknown age would corrupt the next momentum pass: refuse
            const TileBuckets tb = C.buckets_of(b, 1);
            if (!tb.cell || !b.caps_ready || !b.ev_caps || b.caps_key != (const void*)C.buckets_of(b, 0).off)
                return fail(FY_ERR_INVALID, "fy_solver_step: heat exchange: batch %d has no tile-bucket capacities of this step (a Gaussian batch on a structured block always has)", bi);
            FY_HIP(hipStreamWaitEvent(stream, b.ev_caps, 0));
            FY_TRY(launch_heat_coeff_gaussian(stream, C.soa_of(b), b.n, th.hp, cw, C.d_cellrec.p, tp, t.hA.p, th.Sp.p, th.Su.p, tb));
        } else {
            FY_TRY(launch_heat_coeff_point(stream, b.d_rec, b.n, b.incell.p, th.hp, cw, U.p, tp, t.hA.p, th.Sp.p, th.Su.p));
        }
    }
    th.clk_coeff.end(stream);
    return FY_OK;
}

// the T equation, once per step: assembled into the momentum matrix's storage (free after the correctors and the turbulence model's equations) as {T, 0, 0}
int Solver::solve_temperature() {
    Comm::Tag tag(comm, "temperature");
    th.clk_asm.begin(stream);
    FY_TRY(FVK(launch_assemble_scalar, stream, g, th.eq, th.T.p, pimple ? alpha.p : nullptr, phi_now(), th.Sp.p, th.Su.p, M7(false), bmom.p, HbyA.p));
    th.clk_asm.end(stream);
    hbya_ready = false;
    FY_TRY(solve_vec3(HbyA, bmom.p, th.d.T_tol, th.d.T_rel_tol, th.d.T_max_iter, &th.iters, false, &th.res0));
    return FVK(launch_scalar_finish, stream, g, HbyA.p, th.T.p);
}

// pass B: what each particle received, with the T just solved
int Solver::heat_fluxes() {
    Coupling& C = cpl->c;
    const CellWindow cw{0, (int64_t)nstore};
    th.clk_flux.begin(stream);
    for (int bi = 0; bi < C.n_batches; ++bi) {
        Batch& b = *C.batches[(size_t)bi];
        Thermal::PerBatch& t = th.batch((size_t)bi);
        if (b.n == 0) continue;
        double* tp = t.has_tp ? t.Tp.p : nullptr;              // (own_tp: heat_coefficients made it)
        if (th.own_tp && (!tp || t.tp_n != b.n)) return fail(FY_ERR_INVALID, "fy_solver_step: heat exchange: batch %d has no temperature array of this step", bi);
        if (C.gaussian) FY_TRY(launch_heat_flux_gaussian(stream, C.soa_of(b), b.n, cw, th.T.p, th.hp, tp, t.hA.p, t.q.p));
        else FY_TRY(launch_heat_flux_point(stream, b.d_rec, b.n, b.incell.p, cw, th.T.p, th.hp, tp, t.hA.p, t.q.p));
    }
    th.clk_flux.end(stream);
    return FY_OK;
}

// Boussinesq buoyancy, once per step: a from T as the step found it, kept for all outer correctors, and the sum the momentum equations read in uSource's place
int Solver::buoyancy() {
    th.clk_buoy.begin(stream);
    FY_TRY(launch_buoyancy(stream, nstore, th.T.p, th.d.beta, th.d.T_ref, cs.g, uSource.p, th.buoy.p, th.usrc_sum.p));
    th.clk_buoy.end(stream);
    return FY_OK;
}

void Solver::sync_particle_temperatures(size_t bi, int64_t n) {
    Thermal::PerBatch& t = th.batch(bi);
    if (!t.has_tp || t.tp_n == n) return;
    t.has_tp = false;
    ++th.tp_resets;
}

int Solver::get_particle_thermal_state(int batch, double* tp, int64_t* resets) {
    if (!th.on) return fail(FY_ERR_INVALID, "fy_solver_get_particle_thermal_state: this solver has no heat transfer (fy_case_desc.thermal is off)");
    Coupling& C = cpl->c;
    if (!tp) { if (resets) *resets = th.tp_resets; return FY_OK; }      // (the counter alone: no batch is looked at)
    if (batch < 0 || batch >= C.n_batches) return fail(FY_ERR_INVALID, "fy_solver_get_particle_thermal_state: batch %d of %d", batch, C.n_batches);
    const int64_t n = C.batches[(size_t)batch]->n;
    sync_particle_temperatures((size_t)batch, n);
    if (n > 0) {
        Thermal::PerBatch& t = th.batch((size_t)batch);
        if (t.has_tp) {
            FY_HIP(hipSetDevice(device));
            FY_HIP(hipMemcpyAsync(tp, t.Tp.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
            FY_HIP(hipStreamSynchronize(stream));
        } else {
            std::fill(tp, tp + n, th.hp.tp_uniform);
        }
    }
    if (resets) *resets = th.tp_resets;
    return FY_OK;
}

int Solver::set_particle_temperatures(int batch, const double* tp, bool on_device) {
    if (!th.on) return fail(FY_ERR_INVALID, "fy_solver_set_particle_temperatures: this solver has no heat transfer (fy_case_desc.thermal is off)");
    Coupling& C = cpl->c;
    if (batch < 0 || batch >= C.n_batches) return fail(FY_ERR_INVALID, "fy_solver_set_particle_temperatures: batch %d of %d", batch, C.n_batches);
    Thermal::PerBatch& t = th.batch((size_t)batch);
    const int64_t n = C.batches[(size_t)batch]->n;
    if (!tp || n == 0) { t.has_tp = false; return FY_OK; }
    FY_HIP(hipSetDevice(device));
    FY_TRY(t.Tp.reserve((size_t)n));
    FY_HIP(hipMemcpyAsync(t.Tp.p, tp, (size_t)n * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    FY_HIP(hipStreamSynchronize(stream));
    t.has_tp = true; t.tp_n = n;
    return FY_OK;
}

int Solver::get_particle_heat(int batch, double* q) {
    if (!th.on) return fail(FY_ERR_INVALID, "fy_solver_get_particle_heat_host: this solver has no heat transfer (fy_case_desc.thermal is off)");
    if (batch < 0 || (size_t)batch >= th.pb.size()) return fail(FY_ERR_INVALID, "fy_solver_get_particle_heat_host: batch %d of %zu (after a step)", batch, th.pb.size());
    Thermal::PerBatch& t = *th.pb[(size_t)batch];
    if (t.n == 0) return FY_OK;
    if (!q) return fail(FY_ERR_INVALID, "fy_solver_get_particle_heat_host: null array");
    FY_HIP(hipSetDevice(device));
    FY_HIP(hipMemcpyAsync(q, t.q.p, (size_t)t.n * sizeof(double), hipMemcpyDeviceToHost, stream));
    FY_HIP(hipStreamSynchronize(stream));
    return FY_OK;
}

int Solver::thermal_stats(int32_t* iterations, double* initial_residual, double* heat_to_particles_W) {
    if (!th.on) return fail(FY_ERR_INVALID, "fy_solver_get_thermal_stats: this solver has no heat transfer (fy_case_desc.thermal is off)");
    if (iterations) *iterations = th.iters;
    if (initial_residual) *initial_residual = th.res0;
    if (heat_to_particles_W) {
        // summed on the device (k_dot's block partials, folded in a fixed order): one double per batch comes back, not the batch's q array
        FY_HIP(hipSetDevice(device));
        double sum = 0.0;
        for (size_t bi = 0; bi < th.pb.size(); ++bi) {
            const int64_t n = th.pb[bi]->n;
            if (n == 0) continue;
            if (n > 0x7fffffff) return fail(FY_ERR_UNSUPPORTED, "fy_solver_get_thermal_stats: batch %zu holds more than 2^31 particles", bi);
            FY_TRY(th.red.reserve((size_t)red_blocks((int)n) + 1));
            double* out = th.red.p + red_blocks((int)n);
            FY_TRY(launch_dot(stream, (int)n, 0, th.pb[bi]->q.p, nullptr, th.red.p));
            FY_TRY(launch_reduce_finalize(stream, th.red.p, (int)n, 1, nullptr, out));
            double h = 0.0;
            FY_HIP(hipMemcpyAsync(&h, out, sizeof(double), hipMemcpyDeviceToHost, stream));
            FY_HIP(hipStreamSynchronize(stream));
            sum += h;
        }
        *heat_to_particles_W = sum;
    }
    return FY_OK;
}

}  // namespace fy
