// fy::HeatExchange: the particles' half of the heat exchange (fy_thermal_desc) as the host sees it -- per batch the arrays hA, q and Tp (wire order), who owns Tp and
// for how many particles it stands, the reset counter, the two particle passes around the fluid's T solve, and the entry points' set / get.  One object serves
// fy_solver and fy_ldu_solver (as fy::FieldAverage does): the solver hands it its coupling object, its stream, its cell window and the fields the kernels of
// particle_heat.hip read (U, T) and add to (Sp, Su).  The fluid's equation, its sources' storage and the buoyancy stay with each solver.
#pragma once
#include <memory>
#include <vector>

#include "coupling.hpp"

namespace fy {

struct HeatExchange {
    bool on = false;
    const char* who = "fy_solver";       // the entry points' prefix and the descriptor's name in error texts ("fy_ldu_solver", "fy_ldu_case")
    const char* desc = "fy_case_desc";
    HeatParams hp{};
    struct PerBatch {
        DevBuf<double> hA, Tp, q;        // wire order
        int64_t n = 0;                   // particles hA / q were formed for (the last step's count)
        // Tp holds temperatures for tp_n particles: the caller's, or (own_tp) the ones the library integrates; otherwise hp.tp_uniform
        bool has_tp = false;
        int64_t tp_n = 0;
    };
    std::vector<std::unique_ptr<PerBatch> > pb;
    bool own_tp = false;                 // particle_cp > 0: k_heat_coeff_* / k_heat_flux_*<true> advance each batch's Tp
    int64_t tp_resets = 0;               // batches whose Tp array was dropped because their particle count changed
    DevBuf<double> red;                  // block partials + result of the device-side sum of q (total_heat)
    PerBatch& batch(size_t bi) { while (pb.size() <= bi) pb.emplace_back(new PerBatch()); return *pb[bi]; }

    // what fy_solver_create and fy_ldu_solver_create check alike (`fn`: the function's name): everything of fy_thermal_desc but the patch conditions
    static int validate(const fy_thermal_desc& d, bool pimple, double rho_particle, const char* fn);
    // hp and own_tp from a validated descriptor; `solver`, `descriptor`: the names the error texts carry
    void configure(const fy_thermal_desc& d, double nu, double rho_fluid, double rho_particle, double dt, const char* solver, const char* descriptor);
    // pass A, once per step right after setParticleAction returned: per batch hA and Sp[c] += w hA, Su[c] += w hA Tp (the caller has cleared Sp / Su).  bucketed: a
    // structured block's Gaussian scatter goes through the momentum back-scatter's tile buckets (and is refused without this step's capacities); otherwise (a general
    // mesh) the LDS table flushes as global atomics
    int coefficients(Coupling& C, hipStream_t stream, CellWindow cw, const double* U, double* Sp, double* Su, double dt, bool bucketed);
    // pass B, after the T solve: q = hA (sum w T - Tp), and with own_tp Tp advanced in place
    int fluxes(Coupling& C, hipStream_t stream, CellWindow cw, const double* T);
    void sync(size_t bi, int64_t n);     // drops a Tp array held for another particle count (counted in tp_resets)
    int get_state(Coupling& C, int device, hipStream_t stream, int batch, double* tp, int64_t* resets);
    int set_temperatures(Coupling& C, int device, hipStream_t stream, int batch, const double* tp, bool on_device);
    int get_heat(int device, hipStream_t stream, int batch, double* q);
    int total_heat(int device, hipStream_t stream, double* sum);      // sum of q over all batches, summed on the device
    int refuse_off(const char* fn) const;                             // the "this solver has no heat transfer" error of entry point <who>_<fn>
};

}  // namespace fy
