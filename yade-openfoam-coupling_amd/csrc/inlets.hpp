// Inlets (fy_inlets_desc; DESIGN.md section 3 "Inlets"): fixed-value velocity sides (fy_solver) or patches (fy_ldu_solver) whose value varies over the faces and in
// time, U_f(t) = sum_m a_m(t) S_m,f.  The host half, shared by both solvers: the descriptor's checks, the time functions (inlets.cpp), the shapes expanded to one vector
// per face and uploaded once, and the step's launch of k_inlet_values (inlets.hip) with the step's a_m as kernel arguments.  Off (no inlet): nothing allocated, nothing
// launched.
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "common.hpp"

namespace fy {

static_assert(sizeof(fy_time_function) == 72 && sizeof(fy_inlet_term) == 88 && sizeof(fy_inlet_desc) == 272 && sizeof(fy_inlets_desc) == 24,
              "the Python mirror (TimeFunction, InletTerm, InletDesc, InletsDesc) states the same sizes");

// the update kernel's arguments: inlet q owns the faces [first[q], first[q + 1]) of the list and writes them from out[3 base[q]] on; a[q][m] = a_m(t) of this step
struct InletArgs {
    int n;
    int first[FY_INLETS_MAX + 1];
    int base[FY_INLETS_MAX];
    int nterms[FY_INLETS_MAX];
    double a[FY_INLETS_MAX][3];
};
// out[3 (base[q] + e - first[q]) + c] = sum_m a[q][m] shapes[3 (m ne + e) + c] for every face e < ne of the list (one lane per face)
int launch_inlet_values(hipStream_t s, const InletArgs& A, int ne, const double* shapes, double* out);

// a side or patch as the inlets see it: its faces' outward area vectors [n][3] in "U_boundary"'s order, where its values start in the solver's per-face buffer
struct InletPatch {
    int n_faces = 0, base = 0;
    std::vector<double> Sf;
};

struct Inlets {
    struct One {
        int patch = 0, nterms = 0, first = 0, count = 0, base = 0;
        fy_time_function fn[3];
        std::vector<double> pts[3];           // the tables' points (fn[m].points points here)
        bool flux_free = true;                // no term's shape carries a net normal flux (the 1e-8 rule of the balance check)
    };
    std::vector<One> in;
    double start_time = 0.0;
    int ne = 0;                               // faces of all inlets
    DevBuf<double> shapes;                    // [3][ne][3]
    KernelClock clock;

    bool on() const { return !in.empty(); }
    bool has(int patch) const { for (const One& o : in) if (o.patch == patch) return true; return false; }
    bool flux_free() const { for (const One& o : in) if (!o.flux_free) return false; return true; }
    void clear() { in.clear(); ne = 0; start_time = 0.0; shapes.release(); clock.reset(); }
    // take over what a freshly configured object holds (the solvers configure aside and commit once nothing can fail any more); every launch is timed while timing is on
    void take(Inlets& o) {
        in.swap(o.in); ne = o.ne; start_time = o.start_time;
        shapes.release(); std::swap(shapes.p, o.shapes.p); std::swap(shapes.n, o.shapes.n);
        for (One& x : in) for (int m = 0; m < x.nterms; ++m) if (x.fn[m].kind == FY_TIME_TABLE) x.fn[m].points = x.pts[m].data();
        clock.reset(); clock.per_collect = (size_t)1 << 20;
    }
    // check the descriptor by name and take it over; patch_of(patch, &info): FY_OK and the side's or patch's faces, or the refusal (not fixed-value, no such patch).
    // Nothing of the present state is touched when it fails
    int configure(const fy_inlets_desc* d, hipStream_t stream, const char* who, const std::function<int(int, InletPatch*)>& patch_of);
    // the values of time t into out (the solver's per-face buffer), one launch
    int update(hipStream_t stream, double t, double* out);
};

// a malformed function by name (who: the caller and the term), or FY_OK
int check_time_function(const fy_time_function& f, const std::string& who);

}  // namespace fy
