// fy::Solver's heat exchange: the fluid temperature equation and the particles' share of it (fy_thermal_desc, Thermal in fv_solver.hpp).  Not in the
// reference; DESIGN.md section 3 "heat exchange", DESIGN_FV.md "T equation".  Host code only sequences the fluid's kernels of fv_kernels.hip (k_assemble_scalar) on the solver's stream; the
// particle passes and the per-batch temperature bookkeeping are fy::HeatExchange's (heat_exchange.hpp), which fy_ldu_solver holds too.
#include "fv_solver.hpp"

namespace fy {

int Solver::thermal_create(const fy_case_desc* c) {
    const fy_thermal_desc& d = c->thermal;
    FY_TRY(HeatExchange::validate(d, pimple, c->rho_particle, "fy_solver_create"));
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
    th.part.configure(d, c->nu, c->rho_fluid, c->rho_particle, c->dt, "fy_solver", "fy_case_desc");
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
    FY_TRY(zero(th.Sp)); FY_TRY(zero(th.Su));
    th.clk_coeff.begin(stream);
    FY_TRY(th.part.coefficients(cpl->c, stream, CellWindow{0, (int64_t)nstore}, U.p, th.Sp.p, th.Su.p, cs.dt, true));      // (a structured block: through the tile buckets)
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
    th.clk_flux.begin(stream);
    FY_TRY(th.part.fluxes(cpl->c, stream, CellWindow{0, (int64_t)nstore}, th.T.p));
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

int Solver::get_particle_thermal_state(int batch, double* tp, int64_t* resets) { return th.part.get_state(cpl->c, device, stream, batch, tp, resets); }
int Solver::set_particle_temperatures(int batch, const double* tp, bool on_device) { return th.part.set_temperatures(cpl->c, device, stream, batch, tp, on_device); }
int Solver::get_particle_heat(int batch, double* q) { return th.part.get_heat(device, stream, batch, q); }

int Solver::thermal_stats(int32_t* iterations, double* initial_residual, double* heat_to_particles_W) {
    if (!th.on) return th.part.refuse_off("get_thermal_stats");
    if (iterations) *iterations = th.iters;
    if (initial_residual) *initial_residual = th.res0;
    if (heat_to_particles_W) FY_TRY(th.part.total_heat(device, stream, heat_to_particles_W));
    return FY_OK;
}

}  // namespace fy
