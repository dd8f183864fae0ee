// fy::FieldAverage: running means and second central moments of cell fields, updated on the device once per solver step (the role of OpenFOAM's
// fieldAverage function object; the arithmetic is fieldAverage's as recalled from OpenFOAM-6 fieldAverageTemplates.C, DESIGN.md sections 5 and 6):
//     base time:       Dt = T + dt,  a = (Dt - dt) / Dt,  b = dt / Dt
//     base iteration:  Dt = N + 1,   a = (Dt - 1) / Dt,   b = 1 / Dt                 (a, b formed on the host in double)
//     per cell:        P = P + m m;  m_new = a m + b x;  P = (a P + b (x x)) - m_new m_new;  m = m_new          (P only with prime2Mean)
// One object serves fy_solver and fy_ldu_solver: it owns the items, their buffers (owned cells only, no ghost planes), N and T, and the launch.  The solver
// hands it the CURRENT device pointer of each source field at every sample (the solvers' buffers trade places).
#pragma once
#include <string>

#include "common.hpp"

namespace fy {

// the kernel's by-value argument table
struct AvgEntry {
    const double* x;      // the source field's owned cells
    double* m;            // mean, comp values per cell
    double* P;            // prime2Mean: 1 (scalar) or 6 (vector, xx xy xz yy yz zz) values per cell; nullptr = mean only
    double a, b;
    int comp;             // 1 | 3
    int mode;             // 0: flat, two values per thread (16-byte accesses); 1: flat, one value per thread (a pointer off the 16-byte grid); 2: per cell, vector with P
    int nblk;             // blocks of the grid's row that work on this item (its share of the launch by traffic); the rest leave at once
    int pad_;
};
struct AvgTable {
    AvgEntry e[FY_AVERAGE_MAX_ITEMS];
};
int launch_field_average(hipStream_t stream, const AvgTable& tab, int n_items, size_t n_cells);

struct FieldAverage {
    struct Item {
        std::string field;
        int comp = 1;
        bool prime2 = false, iteration_base = false;
        DevBuf<double> m, P;
        int64_t N = 0;        // samples taken
        double T = 0.0;       // simulated time averaged so far
    };
    Item items[FY_AVERAGE_MAX_ITEMS];
    int n_items = 0;
    size_t n_cells = 0;
    double start_after = 0.0, stop_after = 0.0;
    double elapsed = 0.0;     // sum of the steps' deltaT since the solver was created (counted whether or not anything is averaged)
    KernelClock clock;        // "field_average" of fy_solver_get_kernel_timing

    bool on() const { return n_items > 0; }
    void off() { for (Item& it : items) { it.m.release(); it.P.release(); it.field.clear(); it.N = 0; it.T = 0.0; } n_items = 0; }
    ~FieldAverage() { clock.destroy(); }

    // resolve(name, &comp) -> the field's device pointer (owned cells), or nullptr where this solver has no such field
    template <class R>
    int configure(const fy_average_desc* d, size_t cells, hipStream_t stream, const char* who, R&& resolve) {
        off();
        if (!d || d->n_items == 0) return FY_OK;
        if (d->n_items < 0 || d->n_items > FY_AVERAGE_MAX_ITEMS)
            return fail(FY_ERR_INVALID, "%s: %d items (at most FY_AVERAGE_MAX_ITEMS = %d)", who, d->n_items, FY_AVERAGE_MAX_ITEMS);
        if (!(d->start_after >= 0) || !(d->stop_after >= 0)) return fail(FY_ERR_INVALID, "%s: start_after and stop_after must not be negative", who);
        static const char* const known[] = {"U", "p", "alpha", "uParticle", "uSource", "nut", "k", "epsilon", "T", "nParticle", "solidFraction", "uSolid", "granularTemperature", "dSauter", "TParticle"};
        for (int q = 0; q < d->n_items; ++q) {
            char nm[sizeof(d->items[q].field) + 1] = {0};
            std::memcpy(nm, d->items[q].field, sizeof(d->items[q].field));
            bool ok = false;
            for (const char* k : known) ok = ok || std::strcmp(k, nm) == 0;
            int comp = 0;
            if (!ok || !resolve(std::string(nm), &comp)) {
                const int rc = fail(FY_ERR_INVALID, "%s: field '%s' %s (U, p, alpha, uParticle, uSource, nut, k, epsilon, T, nParticle, solidFraction, uSolid, granularTemperature, dSauter, TParticle, where the solver has the field)", who, nm,
                                    ok ? "does not exist in this case" : "cannot be averaged");
                off();
                return rc;
            }
            for (int r = 0; r < q; ++r)
                if (items[r].field == nm) { const int rc = fail(FY_ERR_INVALID, "%s: field '%s' is listed twice", who, nm); off(); return rc; }
            Item& it = items[q];
            it.field = nm; it.comp = comp; it.prime2 = d->items[q].prime2_mean != 0; it.iteration_base = d->items[q].iteration_base != 0;
            int rc = it.m.alloc_exact(cells * (size_t)comp);
            if (rc == FY_OK && it.prime2) rc = it.P.alloc_exact(cells * (size_t)(comp == 3 ? 6 : 1));
            if (rc != FY_OK) { off(); return rc; }
            FY_HIP(hipMemsetAsync(it.m.p, 0, it.m.n * sizeof(double), stream));
            if (it.P.p) FY_HIP(hipMemsetAsync(it.P.p, 0, it.P.n * sizeof(double), stream));
            n_items = q + 1;
        }
        n_cells = cells; start_after = d->start_after; stop_after = d->stop_after;
        FY_HIP(hipStreamSynchronize(stream));
        return FY_OK;
    }

    // the step that has just finished used dt: one launch for all items when the step lies inside the window (timeControl::active() [OF-6])
    template <class R>
    int sample(hipStream_t stream, double dt, R&& resolve) {
        if (elapsed < start_after - 0.5 * dt || (stop_after > 0 && elapsed > stop_after + 0.5 * dt)) return FY_OK;
        AvgTable tab{};
        for (int q = 0; q < n_items; ++q) {
            Item& it = items[q];
            int comp = 0;
            AvgEntry& e = tab.e[q];
            e.x = resolve(it.field, &comp);
            if (!e.x || comp != it.comp) return fail(FY_ERR_INVALID, "fieldAverage: field '%s' is gone", it.field.c_str());
            const double Dt = it.iteration_base ? (double)(it.N + 1) : it.T + dt;
            const double w = it.iteration_base ? 1.0 : dt;
            e.a = (Dt - w) / Dt; e.b = w / Dt;
            e.m = it.m.p; e.P = it.P.p; e.comp = comp;
        }
        clock.begin(stream);
        FY_TRY(launch_field_average(stream, tab, n_items, n_cells));
        clock.end(stream);
        for (int q = 0; q < n_items; ++q) { items[q].N += 1; items[q].T += dt; }
        return FY_OK;
    }

    // "<field>Mean" / "<field>Prime2Mean" of the solvers' field accessors: true when `name` is one of this object's buffers
    bool lookup(const std::string& name, double** ptr, size_t* count) {
        for (int q = 0; q < n_items; ++q) {
            Item& it = items[q];
            if (name == it.field + "Mean") { *ptr = it.m.p; *count = it.m.n; return true; }
            if (it.prime2 && name == it.field + "Prime2Mean") { *ptr = it.P.p; *count = it.P.n; return true; }
        }
        return false;
    }
    int get_state(int item, int64_t* samples, double* time_averaged) const {
        if (item < 0 || item >= n_items) return fail(FY_ERR_INVALID, "fieldAverage: item %d of %d", item, n_items);
        if (samples) *samples = items[item].N;
        if (time_averaged) *time_averaged = items[item].T;
        return FY_OK;
    }
    int set_state(int item, int64_t samples, double time_averaged) {
        if (item < 0 || item >= n_items) return fail(FY_ERR_INVALID, "fieldAverage: item %d of %d", item, n_items);
        if (samples < 0 || !(time_averaged >= 0)) return fail(FY_ERR_INVALID, "fieldAverage: samples and time_averaged must not be negative");
        items[item].N = samples; items[item].T = time_averaged;
        return FY_OK;
    }
};

}  // namespace fy
