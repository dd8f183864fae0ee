// fy::SolidStats: the solid-phase statistics (fy_solver_set_solid_statistics) as the host sees them -- the eight per-cell sums, the fields formed from them, the pass
// that fills both once per step, and the names they are read by.  One object serves fy_solver and fy_ldu_solver (as fy::HeatExchange does): the solver hands it its
// coupling object, its stream, its cell window and, with heat transfer on, the heat exchange whose particle temperatures s7 weighs.  Off: nothing allocated, nothing
// launched.  The kernels are particle_moments.hip's.
#pragma once
#include <string>

#include "coupling.hpp"
#include "heat_exchange.hpp"

namespace fy {

struct SolidStats {
    bool on = false;
    bool with_T = false;                 // the solver has heat transfer: "TParticle" exists
    const char* who = "fy_solver";       // the entry points' prefix in error texts ("fy_ldu_solver")
    size_t n = 0;                        // cells
    DevBuf<double> sums;                 // 8 n: SolidMoments' two halves (a0 | a3 | b0 | b3)
    DevBuf<double> fields;               // 7 n (8 n with heat transfer): nParticle | solidFraction | uSolid | granularTemperature | dSauter [| TParticle]
    DevBuf<double> out8;                 // "solidMoments" [n][8], formed on request
    KernelClock clock;                   // "solid_stats" of the solvers' kernel timing: all launches of one pass together
    ~SolidStats() { clock.destroy(); }

    SolidMoments moments() const { return SolidMoments{sums.p, sums.p + n, sums.p + 4 * n, sums.p + 5 * n}; }
    SolidFields views() const { return SolidFields{fields.p, fields.p + n, fields.p + 2 * n, fields.p + 5 * n, fields.p + 6 * n, with_T ? fields.p + 7 * n : nullptr}; }

    // on: allocates and zeroes (the fields are zero before the first coupling call); off: frees everything
    int set(bool enable, size_t n_cells, bool thermal, hipStream_t stream);
    // once per step, after the T equation's pass B: the sums cleared, every batch's particles scattered, the fields formed.  he: the solver's heat exchange (its
    // temperatures of this step) or nullptr.  bucketed: a structured block's Gaussian scatter goes through the momentum back-scatter's tile buckets (and is refused
    // without this step's capacities, as HeatExchange::coefficients refuses); otherwise (a general mesh) the LDS table flushes as global atomics
    int pass(Coupling& C, hipStream_t stream, CellWindow cw, const double* vol, HeatExchange* he, bool bucketed);
    // one of the six fields by name: its cells and components, or nullptr (off, unknown, or TParticle without heat transfer)
    const double* source(const std::string& name, int* comp) const;
    static bool is_name(const std::string& name);      // solidMoments or one of the six
    // the read-out of a name is_name() accepts: FY_ERR_INVALID while off (the name is then unknown) or for TParticle without heat transfer
    int field(const std::string& name, hipStream_t stream, double** ptr, size_t* count);
};

}  // namespace fy
