// Inlets, the host half (inlets.hpp): the time functions [OF-6 Function1: Constant, Table, Sine, Square, as recalled -- unpinned], the descriptor's checks, the shapes.
#include "inlets.hpp"

#include <cmath>
#include <limits>

namespace fy {

namespace {

// linear interpolation in a table whose times increase strictly; t inside [t_0, t_last]
double table_at(const double* p, int n, double t) {
    if (n == 1 || t <= p[0]) return p[1];
    if (t >= p[2 * (size_t)(n - 1)]) return p[2 * (size_t)(n - 1) + 1];
    int lo = 0, hi = n - 1;                       // p[2 lo] <= t < p[2 hi]
    while (hi - lo > 1) { const int mid = (lo + hi) / 2; if (p[2 * (size_t)mid] <= t) lo = mid; else hi = mid; }
    const double t0 = p[2 * (size_t)lo], v0 = p[2 * (size_t)lo + 1], t1 = p[2 * (size_t)hi], v1 = p[2 * (size_t)hi + 1];
    return v0 + (v1 - v0) * ((t - t0) / (t1 - t0));
}

double eval(const fy_time_function& f, double t) {
    switch (f.kind) {
        case FY_TIME_CONSTANT: return f.value;
        case FY_TIME_TABLE: {
            const double* p = f.points;
            const int n = f.n_points;
            double x = t;
            if (f.out_of_bounds == FY_TIME_REPEAT && (t < p[0] || t > p[2 * (size_t)(n - 1)])) {
                const double span = p[2 * (size_t)(n - 1)] - p[0], u = t - p[0];
                x = p[0] + (u - span * std::floor(u / span));
            }
            return table_at(p, n, x);
        }
        case FY_TIME_SINE: return f.amplitude * std::sin((2.0 * M_PI * f.frequency) * (t - f.t0));
        case FY_TIME_SQUARE: {
            const double ms = f.mark_space == 0.0 ? 1.0 : f.mark_space;
            const double y = f.frequency * (t - f.t0), fr = y - std::floor(y);
            return fr < ms / (1.0 + ms) ? f.amplitude : -f.amplitude;
        }
    }
    return std::numeric_limits<double>::quiet_NaN();
}

}  // namespace

int check_time_function(const fy_time_function& f, const std::string& who) {
    const char* w = who.c_str();
    switch (f.kind) {
        case FY_TIME_CONSTANT:
            if (!std::isfinite(f.value)) return fail(FY_ERR_INVALID, "%s: constant: the value is not finite", w);
            return FY_OK;
        case FY_TIME_TABLE:
            if (f.n_points < 1 || !f.points) return fail(FY_ERR_INVALID, "%s: table: no points (n_points %d)", w, f.n_points);
            if (f.out_of_bounds != FY_TIME_CLAMP && f.out_of_bounds != FY_TIME_REPEAT) return fail(FY_ERR_INVALID, "%s: table: outOfBounds %d (FY_TIME_CLAMP, FY_TIME_REPEAT; error and warn are not offered)", w, f.out_of_bounds);
            if (f.out_of_bounds == FY_TIME_REPEAT && f.n_points < 2) return fail(FY_ERR_INVALID, "%s: table: outOfBounds repeat needs two points or more", w);
            for (int q = 0; q < f.n_points; ++q) {
                if (!std::isfinite(f.points[2 * (size_t)q]) || !std::isfinite(f.points[2 * (size_t)q + 1])) return fail(FY_ERR_INVALID, "%s: table: point %d is not finite", w, q);
                if (q > 0 && !(f.points[2 * (size_t)q] > f.points[2 * (size_t)(q - 1)])) return fail(FY_ERR_INVALID, "%s: table: the times do not increase strictly at point %d (%g after %g)", w, q, f.points[2 * (size_t)q], f.points[2 * (size_t)(q - 1)]);
            }
            return FY_OK;
        case FY_TIME_SINE:
        case FY_TIME_SQUARE: {
            const char* k = f.kind == FY_TIME_SINE ? "sine" : "square";
            if (!(f.frequency > 0) || !std::isfinite(f.frequency)) return fail(FY_ERR_INVALID, "%s: %s: frequency %g must be positive", w, k, f.frequency);
            if (!std::isfinite(f.amplitude) || !std::isfinite(f.t0)) return fail(FY_ERR_INVALID, "%s: %s: amplitude and t0 must be finite", w, k);
            if (f.kind == FY_TIME_SQUARE && (!(f.mark_space >= 0) || !std::isfinite(f.mark_space))) return fail(FY_ERR_INVALID, "%s: square: markSpace %g must be positive (0: 1)", w, f.mark_space);
            return FY_OK;
        }
    }
    return fail(FY_ERR_INVALID, "%s: unknown time function kind %d (FY_TIME_CONSTANT, FY_TIME_TABLE, FY_TIME_SINE, FY_TIME_SQUARE)", w, f.kind);
}

int Inlets::configure(const fy_inlets_desc* d, hipStream_t stream, const char* who, const std::function<int(int, InletPatch*)>& patch_of) {
    if (!d || d->n == 0) { clear(); return FY_OK; }
    if (d->n < 0 || d->n > FY_INLETS_MAX) return fail(FY_ERR_INVALID, "%s: %d inlets (0 to FY_INLETS_MAX = %d)", who, d->n, FY_INLETS_MAX);
    if (!d->inlets) return fail(FY_ERR_INVALID, "%s: n = %d but inlets is NULL", who, d->n);
    if (!std::isfinite(d->start_time)) return fail(FY_ERR_INVALID, "%s: start_time is not finite", who);
    std::vector<One> fresh((size_t)d->n);
    std::vector<InletPatch> pp((size_t)d->n);
    int total = 0;
    for (int q = 0; q < d->n; ++q) {
        const fy_inlet_desc& id = d->inlets[q];
        One& o = fresh[(size_t)q];
        const std::string iw = std::string(who) + ": inlet " + std::to_string(q) + " (patch " + std::to_string(id.patch) + ")";
        if (id.n_terms < 1 || id.n_terms > 3) return fail(FY_ERR_INVALID, "%s: n_terms %d (1 to 3)", iw.c_str(), id.n_terms);
        for (int r = 0; r < q; ++r) if (d->inlets[r].patch == id.patch) return fail(FY_ERR_INVALID, "%s: the patch is listed twice", iw.c_str());
        FY_TRY(patch_of(id.patch, &pp[(size_t)q]));
        o.patch = id.patch; o.nterms = id.n_terms; o.first = total; o.count = pp[(size_t)q].n_faces; o.base = pp[(size_t)q].base;
        for (int m = 0; m < id.n_terms; ++m) {
            const fy_inlet_term& t = id.terms[m];
            const std::string tw = iw + ", term " + std::to_string(m);
            FY_TRY(check_time_function(t.f, tw));
            o.fn[m] = t.f;
            if (t.f.kind == FY_TIME_TABLE) { o.pts[m].assign(t.f.points, t.f.points + 2 * (size_t)t.f.n_points); }
            if (t.shape_kind != FY_SHAPE_UNIFORM && t.shape_kind != FY_SHAPE_PER_FACE && t.shape_kind != FY_SHAPE_FLOW_RATE)
                return fail(FY_ERR_INVALID, "%s: unknown shape kind %d (FY_SHAPE_UNIFORM, FY_SHAPE_PER_FACE, FY_SHAPE_FLOW_RATE)", tw.c_str(), t.shape_kind);
            if (t.shape_kind != FY_SHAPE_FLOW_RATE && !t.shape) return fail(FY_ERR_INVALID, "%s: the shape array is NULL", tw.c_str());
            if (t.shape_kind != FY_SHAPE_UNIFORM && o.count == 0) return fail(FY_ERR_INVALID, "%s: a per-face or flow-rate shape on a side without faces", tw.c_str());
        }
        total += o.count;
    }
    // the shapes, one vector per face and term: [3][total][3]
    std::vector<double> S(9 * (size_t)std::max(total, 1), 0.0);
    for (int q = 0; q < d->n; ++q) {
        One& o = fresh[(size_t)q];
        const InletPatch& P = pp[(size_t)q];
        double sum_mag = 0.0;
        std::vector<double> mag((size_t)o.count);
        for (int e = 0; e < o.count; ++e) {
            const double* s = &P.Sf[3 * (size_t)e];
            mag[(size_t)e] = std::sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
            sum_mag += mag[(size_t)e];
        }
        for (int m = 0; m < o.nterms; ++m) {
            const fy_inlet_term& t = d->inlets[q].terms[m];
            double net = 0.0, tot = 0.0;
            for (int e = 0; e < o.count; ++e) {
                double* out = &S[3 * ((size_t)m * total + o.first + e)];
                const double* s = &P.Sf[3 * (size_t)e];
                for (int c = 0; c < 3; ++c) {
                    if (t.shape_kind == FY_SHAPE_UNIFORM) out[c] = t.shape[c];
                    else if (t.shape_kind == FY_SHAPE_PER_FACE) out[c] = t.shape[3 * (size_t)e + c];
                    else out[c] = -(s[c] / mag[(size_t)e]) / sum_mag;
                    if (!std::isfinite(out[c])) return fail(FY_ERR_INVALID, "%s: inlet %d, term %d: the shape is not finite at face %d", who, q, m, e);
                }
                const double un = (out[0] * s[0] + out[1] * s[1]) + out[2] * s[2];
                net += un; tot += std::fabs(un);
            }
            if (std::fabs(net) > 1e-8 * (tot + 1e-300)) o.flux_free = false;
        }
    }
    DevBuf<double> dev;
    FY_TRY(dev.alloc_exact(S.size()));
    FY_HIP(hipMemcpyAsync(dev.p, S.data(), S.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    FY_HIP(hipStreamSynchronize(stream));                  // (set-up only: S dies with this scope)
    shapes.release();
    std::swap(shapes.p, dev.p); std::swap(shapes.n, dev.n);
    in.swap(fresh);
    for (One& o : in) for (int m = 0; m < o.nterms; ++m) if (o.fn[m].kind == FY_TIME_TABLE) o.fn[m].points = o.pts[m].data();
    ne = total;
    start_time = d->start_time;
    clock.reset();
    return FY_OK;
}

int Inlets::update(hipStream_t stream, double t, double* out) {
    if (ne == 0) return FY_OK;
    InletArgs A{};
    A.n = (int)in.size();
    for (int q = 0; q < A.n; ++q) {
        const One& o = in[(size_t)q];
        A.first[q] = o.first; A.base[q] = o.base; A.nterms[q] = o.nterms;
        for (int m = 0; m < o.nterms; ++m) A.a[q][m] = eval(o.fn[m], t);
    }
    for (int q = A.n; q <= FY_INLETS_MAX; ++q) A.first[q] = ne;
    clock.begin(stream);
    FY_TRY(launch_inlet_values(stream, A, ne, shapes.p, out));
    clock.end(stream);
    return FY_OK;
}

}  // namespace fy

extern "C" double fy_time_function_eval(const fy_time_function* f, double t) {
    if (!f || fy::check_time_function(*f, "fy_time_function_eval") != FY_OK) return std::numeric_limits<double>::quiet_NaN();
    return fy::eval(*f, t);
}
