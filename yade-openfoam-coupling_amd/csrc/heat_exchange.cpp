// fy::HeatExchange (heat_exchange.hpp): host code that sequences the kernels of particle_heat.hip and keeps the per-batch temperature bookkeeping, for both solvers.
#include "heat_exchange.hpp"

#include <algorithm>
#include <cmath>

#include "fv_linalg_kernels.hpp"
#include "particle_kernels.hpp"

namespace fy {

int HeatExchange::validate(const fy_thermal_desc& d, bool pimple, double rho_particle, const char* fn) {
    if (!(d.cp > 0) || !(d.kappa > 0)) return fail(FY_ERR_INVALID, "%s: thermal needs cp > 0 and kappa > 0 (got %g, %g)", fn, d.cp, d.kappa);
    if (d.prt < 0) return fail(FY_ERR_INVALID, "%s: thermal.prt must not be negative", fn);
    if (d.nusselt_law != FY_NUSSELT_RANZ_MARSHALL && d.nusselt_law != FY_NUSSELT_GUNN)
        return fail(FY_ERR_UNSUPPORTED, "%s: unknown thermal.nusselt_law %d (FY_NUSSELT_RANZ_MARSHALL, FY_NUSSELT_GUNN)", fn, d.nusselt_law);
    if (d.nusselt_law == FY_NUSSELT_GUNN && !pimple)
        return fail(FY_ERR_UNSUPPORTED, "%s: thermal.nusselt_law FY_NUSSELT_GUNN needs the void fraction of the Gaussian mode (pimpleFoamYade); "
                                        "point-force mode (icoFoamYade) takes FY_NUSSELT_RANZ_MARSHALL", fn);
    if (d.T_convection_scheme != FY_CONVECTION_LINEAR && d.T_convection_scheme != FY_CONVECTION_UPWIND)
        return fail(FY_ERR_UNSUPPORTED, "%s: thermal.T_convection_scheme must be FY_CONVECTION_LINEAR or FY_CONVECTION_UPWIND", fn);
    // (with both tolerances zero the residual test `res < tol` never holds -- the two idle components' residuals are exactly 0 -- and every step would run T_max_iter passes;
    //  with no pass allowed T would never move)
    if (!(d.T_tol >= 0) || !(d.T_rel_tol >= 0) || !(d.T_tol > 0 || d.T_rel_tol > 0) || d.T_max_iter < 1)
        return fail(FY_ERR_INVALID, "%s: thermal needs T_tol >= 0 and T_rel_tol >= 0 with at least one of them positive, and T_max_iter >= 1 (got %g, %g, %d)", fn, d.T_tol, d.T_rel_tol,
                    d.T_max_iter);
    if (!(d.particle_cp >= 0)) return fail(FY_ERR_INVALID, "%s: thermal.particle_cp must not be negative (got %g; 0: the caller owns the particle temperatures)", fn, d.particle_cp);
    if (d.particle_cp > 0 && !(rho_particle > 0))
        return fail(FY_ERR_INVALID, "%s: thermal.particle_cp %g needs rho_particle > 0 for the particles' heat capacity (got %g)", fn, d.particle_cp, rho_particle);
    if (!std::isfinite(d.beta) || !std::isfinite(d.T_ref)) return fail(FY_ERR_INVALID, "%s: thermal.beta and thermal.T_ref must be finite (got %g, %g)", fn, d.beta, d.T_ref);
    return FY_OK;
}

void HeatExchange::configure(const fy_thermal_desc& d, double nu, double rho_fluid, double rho_particle, double dt, const char* solver, const char* descriptor) {
    who = solver; desc = descriptor;
    const double Pr = nu * rho_fluid * d.cp / d.kappa;
    own_tp = d.particle_cp > 0;
    hp = HeatParams{nu, 1e-09, d.kappa, std::cbrt(Pr), d.particle_temperature, d.nusselt_law, dt, rho_particle * d.particle_cp};      // (small: the force laws', ForceParams)
    on = true;
}

int HeatExchange::refuse_off(const char* fn) const { return fail(FY_ERR_INVALID, "%s_%s: this solver has no heat transfer (%s.thermal is off)", who, fn, desc); }

int HeatExchange::coefficients(Coupling& C, hipStream_t stream, CellWindow cw, const double* U, double* Sp, double* Su, double dt, bool bucketed) {
    hp.dt = dt;                                                // (the step's own delta_t: adjust_time_step)
    for (size_t bi = (size_t)C.n_batches; bi < pb.size(); ++bi) pb[bi]->n = 0;      // (batches that are gone)
    for (int bi = 0; bi < C.n_batches; ++bi) {
        Batch& b = *C.batches[(size_t)bi];
        PerBatch& t = batch((size_t)bi);
        t.n = b.n;
        if (b.n == 0) continue;
        FY_TRY(t.hA.reserve((size_t)b.n)); FY_TRY(t.q.reserve((size_t)b.n));
        sync((size_t)bi, b.n);                                 // another population: the uniform temperature again
        if (own_tp && !t.has_tp) {                             // the batch's first step: the array the library advances from here on
            FY_TRY(t.Tp.reserve((size_t)b.n));
            FY_TRY(launch_fill_f64(stream, t.Tp.p, (size_t)b.n, hp.tp_uniform));
            t.has_tp = true; t.tp_n = b.n;
        }
        const double* tp = t.has_tp ? t.Tp.p : nullptr;
        if (C.gaussian) {
            TileBuckets tb{};
            if (bucketed) {
                // the momentum back-scatter's buckets, with the capacities formed from the demand its pass has just counted (k_tile_caps on the side stream at the end of
                // run_batch, demand counters back at zero): the heat scatter has the same (workgroup, cell) pattern, so it fits -- from a population's first step on.  Every
                // Gaussian batch of a structured block has them (Coupling::ensure_batch, the side stream of Coupling::create); anything else is a state this pass was not
                // written for, and flushing into capacities of unknown age would corrupt the next momentum pass: refuse
                tb = C.buckets_of(b, 1);
                if (!tb.cell || !b.caps_ready || !b.ev_caps || b.caps_key != (const void*)C.buckets_of(b, 0).off)
                    return fail(FY_ERR_INVALID, "%s_step: heat exchange: batch %d has no tile-bucket capacities of this step (a Gaussian batch on a structured block always has)", who, bi);
                FY_HIP(hipStreamWaitEvent(stream, b.ev_caps, 0));
            }
            // (no buckets -- a general mesh has no 8^3 tiles: flush_table's tb.cell == nullptr path adds every table entry with global atomics and reads none of tb's arrays)
            FY_TRY(launch_heat_coeff_gaussian(stream, C.soa_of(b), b.n, hp, cw, C.d_cellrec.p, tp, t.hA.p, Sp, Su, tb));
        } else {
            FY_TRY(launch_heat_coeff_point(stream, b.d_rec, b.n, b.incell.p, hp, cw, U, tp, t.hA.p, Sp, Su));
        }
    }
    return FY_OK;
}

int HeatExchange::fluxes(Coupling& C, hipStream_t stream, CellWindow cw, const double* T) {
    for (int bi = 0; bi < C.n_batches; ++bi) {
        Batch& b = *C.batches[(size_t)bi];
        PerBatch& t = batch((size_t)bi);
        if (b.n == 0) continue;
        double* tp = t.has_tp ? t.Tp.p : nullptr;              // (own_tp: coefficients() made it)
        if (own_tp && (!tp || t.tp_n != b.n)) return fail(FY_ERR_INVALID, "%s_step: heat exchange: batch %d has no temperature array of this step", who, bi);
        if (C.gaussian) FY_TRY(launch_heat_flux_gaussian(stream, C.soa_of(b), b.n, cw, T, hp, tp, t.hA.p, t.q.p));
        else FY_TRY(launch_heat_flux_point(stream, b.d_rec, b.n, b.incell.p, cw, T, hp, tp, t.hA.p, t.q.p));
    }
    return FY_OK;
}

void HeatExchange::sync(size_t bi, int64_t n) {
    PerBatch& t = batch(bi);
    if (!t.has_tp || t.tp_n == n) return;
    t.has_tp = false;
    ++tp_resets;
}

int HeatExchange::get_state(Coupling& C, int device, hipStream_t stream, int batch_i, double* tp, int64_t* resets) {
    if (!on) return refuse_off("get_particle_thermal_state");
    if (!tp) { if (resets) *resets = tp_resets; return FY_OK; }      // (the counter alone: no batch is looked at)
    if (batch_i < 0 || batch_i >= C.n_batches) return fail(FY_ERR_INVALID, "%s_get_particle_thermal_state: batch %d of %d", who, batch_i, C.n_batches);
    const int64_t n = C.batches[(size_t)batch_i]->n;
    sync((size_t)batch_i, n);
    if (n > 0) {
        PerBatch& t = batch((size_t)batch_i);
        if (t.has_tp) {
            FY_HIP(hipSetDevice(device));
            FY_HIP(hipMemcpyAsync(tp, t.Tp.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
            FY_HIP(hipStreamSynchronize(stream));
        } else {
            std::fill(tp, tp + n, hp.tp_uniform);
        }
    }
    if (resets) *resets = tp_resets;
    return FY_OK;
}

int HeatExchange::set_temperatures(Coupling& C, int device, hipStream_t stream, int batch_i, const double* tp, bool on_device) {
    if (!on) return refuse_off("set_particle_temperatures");
    if (batch_i < 0 || batch_i >= C.n_batches) return fail(FY_ERR_INVALID, "%s_set_particle_temperatures: batch %d of %d", who, batch_i, C.n_batches);
    PerBatch& t = batch((size_t)batch_i);
    const int64_t n = C.batches[(size_t)batch_i]->n;
    if (!tp || n == 0) { t.has_tp = false; return FY_OK; }
    FY_HIP(hipSetDevice(device));
    FY_TRY(t.Tp.reserve((size_t)n));
    FY_HIP(hipMemcpyAsync(t.Tp.p, tp, (size_t)n * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    FY_HIP(hipStreamSynchronize(stream));
    t.has_tp = true; t.tp_n = n;
    return FY_OK;
}

int HeatExchange::get_heat(int device, hipStream_t stream, int batch_i, double* q) {
    if (!on) return refuse_off("get_particle_heat_host");
    if (batch_i < 0 || (size_t)batch_i >= pb.size()) return fail(FY_ERR_INVALID, "%s_get_particle_heat_host: batch %d of %zu (after a step)", who, batch_i, pb.size());
    PerBatch& t = *pb[(size_t)batch_i];
    if (t.n == 0) return FY_OK;
    if (!q) return fail(FY_ERR_INVALID, "%s_get_particle_heat_host: null array", who);
    FY_HIP(hipSetDevice(device));
    FY_HIP(hipMemcpyAsync(q, t.q.p, (size_t)t.n * sizeof(double), hipMemcpyDeviceToHost, stream));
    FY_HIP(hipStreamSynchronize(stream));
    return FY_OK;
}

int HeatExchange::total_heat(int device, hipStream_t stream, double* out_sum) {
    // summed on the device (k_dot's block partials, folded in a fixed order): one double per batch comes back, not the batch's q array
    FY_HIP(hipSetDevice(device));
    double sum = 0.0;
    for (size_t bi = 0; bi < pb.size(); ++bi) {
        const int64_t n = pb[bi]->n;
        if (n == 0) continue;
        if (n > 0x7fffffff) return fail(FY_ERR_UNSUPPORTED, "%s_get_thermal_stats: batch %zu holds more than 2^31 particles", who, bi);
        FY_TRY(red.reserve((size_t)red_blocks((int)n) + 1));
        double* out = red.p + red_blocks((int)n);
        FY_TRY(launch_dot(stream, (int)n, 0, pb[bi]->q.p, nullptr, red.p));
        FY_TRY(launch_reduce_finalize(stream, red.p, (int)n, 1, nullptr, out));
        double h = 0.0;
        FY_HIP(hipMemcpyAsync(&h, out, sizeof(double), hipMemcpyDeviceToHost, stream));
        FY_HIP(hipStreamSynchronize(stream));
        sum += h;
    }
    *out_sum = sum;
    return FY_OK;
}

}  // namespace fy
