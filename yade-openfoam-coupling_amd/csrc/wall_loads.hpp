// fy::WallLoads: the forces / wallShearStress / yPlus function objects on the device (include/foamyade_hip.h "Wall loads"; the arithmetic is OpenFOAM-6's forces.C,
// wallShearStress.C, yPlus.C and gaussGrad::correctBoundaryConditions as recalled, unpinned: DESIGN.md sections 3 and 5).  Two launches per sample, no atomics, no
// host synchronisation:
//   faces     the solver's own kernel (k_wall_loads in fv_kernels.hip, k_ldu_wall_loads in ldu_kernels.hip): one lane per boundary face, blockIdx.y = the object.  The
//             lane gathers what only the solver knows -- the owner's Gauss gradient of U, s = (U_b - U_P) delta, p_b, nut_b, y, k_P -- into a WlFace and hands it to
//             wl_face_emit below, which states the stress, the per-face outputs and the sums ONCE for both solvers
//   finalize  the monitors' k_monitor_finalize on a MonOut table over this object's partials: the fold in a fixed order, the store into the object's ring
// A component leaves a block as the monitors' five partials (mon_block_reduce_store: S x, -, -, min x, max x); per object kWlComps components:
//   forces           12: Fp xyz, Fv xyz, Mp xyz, Mv xyz
//   wallShearStress  3 per patch of the set
//   yPlus            2 per patch of the set: "1" (the face count, the average's denominator) and y+
// The rings, the histories, drain / layout / get_rows and the clock are a Monitors object's, filled in here.
#pragma once
#include "monitors.hpp"

namespace fy {

constexpr int kWlMaxObjects = FY_WALL_LOADS_MAX_FORCES + 2;
constexpr int kWlMaxPatches = FY_WALL_LOADS_MAX_PATCHES;
constexpr int kWlComps = 3 * kWlMaxPatches;          // (>= 12)
static_assert(sizeof(fy_wall_loads_desc) == 600, "the Python mirror (WallLoadsDesc) states the same size");
static_assert(kWlMaxObjects <= FY_MONITOR_MAX_OBJECTS && kWlComps >= 12, "MonRings holds the rings; a forces object has 12 components");
enum { WL_FORCES = 0, WL_WSS = 1, WL_YPLUS = 2 };
struct WlObj { int kind, np; int patch[kWlMaxPatches]; double rho, p_ref, cofr[3]; };      // patch[]: sides 2 d + s on the block, patch indices on a general mesh
struct WlTable { int n; unsigned due; WlObj o[kWlMaxObjects]; };                            // bit q of due: object q samples this step

#if defined(__HIPCC__)
// one boundary face as its solver sees it
struct WlFace {
    int patch;
    double Sf[3], A, Cf[3];
    double G[9];             // G[3 i + j] = d_i U_j, the Gauss-linear gradient in the owner cell
    double s[3];             // (U_b - U_P) delta
    double pb, nut_b, nu, y, kP, cmu25;
    bool wall_fn;            // a nutkWallFunction patch
};
// steps 3-7 for object o on the lane's face (have: the lane holds boundary face b; the face takes part when its patch is in the object's set), its stores into the
// per-face fields and its components' partials from slot0 on.  Called by every lane of the block
__device__ __forceinline__ void wl_face_emit(const WlObj& o, bool have, const WlFace& f, int b, double* __restrict__ wss, double* __restrict__ yplus, double* __restrict__ partials, int slot0) {
    int member = -1;
    if (have)
        for (int q = 0; q < o.np; ++q) if (o.patch[q] == f.patch) member = q;
    const bool in = member >= 0;
    double n[3] = {0, 0, 0}, R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, nuEff = 0.0;
    if (in) {
        for (int i = 0; i < 3; ++i) n[i] = f.Sf[i] / f.A;
        double Gb[9], nG[3];
        for (int j = 0; j < 3; ++j) nG[j] = (n[0] * f.G[j] + n[1] * f.G[3 + j]) + n[2] * f.G[6 + j];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Gb[3 * i + j] = f.G[3 * i + j] + n[i] * (f.s[j] - nG[j]);          // gaussGrad::correctBoundaryConditions
        const double t0 = Gb[0] + Gb[0], t1 = Gb[4] + Gb[4], t2 = Gb[8] + Gb[8];
        const double tr3 = ((t0 + t1) + t2) / 3.0;
        nuEff = f.nu + f.nut_b;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[3 * i + j] = -nuEff * (i == j ? (Gb[3 * i + j] + Gb[3 * j + i]) - tr3 : Gb[3 * i + j] + Gb[3 * j + i]);
    }
    const int nblk = (int)gridDim.x, blk = (int)blockIdx.x;
    double v[kMonKinds];
    if (o.kind == WL_FORCES) {
        double x[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (in) {
            const double dp = f.pb - o.p_ref;
            for (int j = 0; j < 3; ++j) {
                x[j] = (o.rho * f.Sf[j]) * dp;
                x[3 + j] = o.rho * ((f.Sf[0] * R[j] + f.Sf[1] * R[3 + j]) + f.Sf[2] * R[6 + j]);
            }
            const double r[3] = {f.Cf[0] - o.cofr[0], f.Cf[1] - o.cofr[1], f.Cf[2] - o.cofr[2]};
            for (int h = 0; h < 2; ++h) {
                const double* F = x + 3 * h;
                double* M = x + 6 + 3 * h;
                M[0] = r[1] * F[2] - r[2] * F[1];
                M[1] = r[2] * F[0] - r[0] * F[2];
                M[2] = r[0] * F[1] - r[1] * F[0];
            }
        }
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            mon_terms(in, x[q], 0.0, 0.0, v);
            mon_block_reduce_store(v, partials, slot0 + q * kMonKinds, nblk, blk);
        }
    } else if (o.kind == WL_WSS) {
        double tau[3] = {0, 0, 0};
        if (in)
            for (int j = 0; j < 3; ++j) tau[j] = -((n[0] * R[j] + n[1] * R[3 + j]) + n[2] * R[6 + j]);
        if (have) { wss[3 * (size_t)b] = tau[0]; wss[3 * (size_t)b + 1] = tau[1]; wss[3 * (size_t)b + 2] = tau[2]; }
        for (int q = 0; q < o.np; ++q)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                mon_terms(member == q, tau[j], 0.0, 0.0, v);
                mon_block_reduce_store(v, partials, slot0 + (3 * q + j) * kMonKinds, nblk, blk);
            }
    } else {
        double yp = 0.0;
        if (in) yp = f.wall_fn ? ((f.cmu25 * f.y) * sqrt(f.kP)) / f.nu : (f.y * sqrt(nuEff * sqrt((f.s[0] * f.s[0] + f.s[1] * f.s[1]) + f.s[2] * f.s[2]))) / f.nu;
        if (have) yplus[b] = yp;
        for (int q = 0; q < o.np; ++q) {
            mon_terms(member == q, 1.0, 0.0, 0.0, v);
            mon_block_reduce_store(v, partials, slot0 + (2 * q) * kMonKinds, nblk, blk);
            mon_terms(member == q, yp, 0.0, 0.0, v);
            mon_block_reduce_store(v, partials, slot0 + (2 * q + 1) * kMonKinds, nblk, blk);
        }
    }
}
#endif

struct WallLoads {
    Monitors m;                    // obj[] (name, labels, ring, history, interval), ring_rows, outs, pf / nblk_f, steps, clock
    WlTable tab{};
    DevBuf<double> wss, yplus;     // "wallShearStress_boundary" [nb][3], "yPlus_boundary" [nb] (allocated with their objects)
    size_t nb = 0;
    double start_time = 0.0;

    bool on() const { return m.on(); }
    void off() { m.off(); tab = WlTable{}; wss.release(); yplus.release(); nb = 0; }
    static bool empty(const fy_wall_loads_desc* d) { return !d || (d->n_forces == 0 && !d->wall_shear_stress.on && !d->y_plus.on); }

    // resolve(set, object name, patches[kWlMaxPatches], &np, &labels) -> FY_OK, or the solver's refusal of the patch set; yplus_ok: nu > 0 or a turbulence model
    template <class RP>
    int configure(const fy_wall_loads_desc* d, size_t bfaces, bool yplus_ok, hipStream_t stream, const char* who, RP&& resolve) {
        off();
        if (empty(d)) return FY_OK;
        const int rc = configure_(d, bfaces, yplus_ok, stream, who, resolve);
        if (rc != FY_OK) off();
        return rc;
    }
    template <class RP>
    int configure_(const fy_wall_loads_desc* d, size_t bfaces, bool yplus_ok, hipStream_t stream, const char* who, RP&& resolve) {
        if (d->n_forces < 0 || d->n_forces > FY_WALL_LOADS_MAX_FORCES)
            return fail(FY_ERR_INVALID, "%s: %d forces objects (at most FY_WALL_LOADS_MAX_FORCES = %d)", who, d->n_forces, FY_WALL_LOADS_MAX_FORCES);
        if (d->ring_rows < 0) return fail(FY_ERR_INVALID, "%s: ring_rows %d must not be negative", who, d->ring_rows);
        m.ring_rows = d->ring_rows > 0 ? d->ring_rows : 256;
        nb = bfaces; start_time = d->start_time;
        m.nblk_f = red_blocks((int)std::max<size_t>(bfaces, 1));
        std::vector<MonOut> ho;
        static const char* const xyz[] = {"_x", "_y", "_z"};
        const int n_obj = d->n_forces + (d->wall_shear_stress.on ? 1 : 0) + (d->y_plus.on ? 1 : 0);
        for (int q = 0; q < n_obj; ++q) {
            const bool is_f = q < d->n_forces, is_w = !is_f && d->wall_shear_stress.on && q == d->n_forces;
            const fy_wall_field_object& fo = is_w ? d->wall_shear_stress : d->y_plus;
            Monitors::Obj& o = m.obj[q];
            WlObj& t = tab.o[q];
            char nm[33] = {0};
            if (is_f) std::memcpy(nm, d->forces[q].name, 32);
            o.name = is_f ? std::string(nm) : is_w ? "wallShearStress" : "yPlus";
            const char* on = o.name.c_str();
            const int interval = is_f ? d->forces[q].interval : fo.interval;
            if (interval < 0) return fail(FY_ERR_INVALID, "%s: object '%s': interval %d (>= 1)", who, on, interval);
            o.interval = interval > 0 ? interval : 1;
            t.kind = is_f ? WL_FORCES : is_w ? WL_WSS : WL_YPLUS;
            std::vector<std::string> pn;
            FY_TRY(resolve(is_f ? d->forces[q].set : fo.set, on, t.patch, &t.np, &pn));
            const int slot0 = q * kWlComps * kMonKinds;
            auto out = [&](int comp, int kind, int den_comp, const std::string& label) {
                ho.push_back(MonOut{1, slot0 + comp * kMonKinds + kind, den_comp < 0 ? -1 : slot0 + den_comp * kMonKinds + MK_SUM, kind == MK_MIN ? 1 : kind == MK_MAX ? 2 : 0, q, o.n_values});
                o.labels.push_back(label);
                ++o.n_values;
            };
            if (is_f) {
                const fy_forces_object& in = d->forces[q];
                if (!(in.rho > 0) || !std::isfinite(in.rho)) return fail(FY_ERR_INVALID, "%s: object '%s': rho %g must be positive (rhoInf)", who, on, in.rho);
                t.rho = in.rho; t.p_ref = in.p_ref;
                for (int a = 0; a < 3; ++a) t.cofr[a] = in.cofr[a];
                static const char* const grp[] = {"Fp", "Fv", "Mp", "Mv"};
                for (int c = 0; c < 12; ++c) out(c, MK_SUM, -1, std::string(grp[c / 3]) + xyz[c % 3]);
            } else if (is_w) {
                for (int p = 0; p < t.np; ++p)
                    for (int k = 0; k < 2; ++k)
                        for (int j = 0; j < 3; ++j) out(3 * p + j, k ? MK_MAX : MK_MIN, -1, std::string(k ? "max(" : "min(") + pn[(size_t)p] + ")" + xyz[j]);
                FY_TRY(wss.alloc_exact(3 * std::max<size_t>(bfaces, 1)));
                FY_HIP(hipMemsetAsync(wss.p, 0, wss.n * sizeof(double), stream));
            } else {
                if (!yplus_ok) return fail(FY_ERR_INVALID, "%s: object '%s': yPlus needs nu > 0 or a turbulence model", who, on);
                for (int p = 0; p < t.np; ++p) {
                    out(2 * p + 1, MK_MIN, -1, "min(" + pn[(size_t)p] + ")");
                    out(2 * p + 1, MK_MAX, -1, "max(" + pn[(size_t)p] + ")");
                    out(2 * p + 1, MK_SUM, 2 * p, "average(" + pn[(size_t)p] + ")");
                }
                FY_TRY(yplus.alloc_exact(std::max<size_t>(bfaces, 1)));
                FY_HIP(hipMemsetAsync(yplus.p, 0, yplus.n * sizeof(double), stream));
            }
            FY_TRY(o.ring.alloc_exact((size_t)m.ring_rows * (size_t)(1 + o.n_values)));
            m.n_objects = tab.n = q + 1;
        }
        FY_TRY(m.pf.alloc_exact((size_t)n_obj * kWlComps * kMonKinds * (size_t)m.nblk_f));
        m.n_outs = (int)ho.size();
        FY_TRY(m.outs.alloc_exact(ho.size()));
        FY_HIP(hipMemcpyAsync(m.outs.p, ho.data(), ho.size() * sizeof(MonOut), hipMemcpyHostToDevice, stream));
        FY_HIP(hipStreamSynchronize(stream));
        return FY_OK;
    }

    // the step that has just finished, at `time`: face_launch(table, partials, nblk, wss, yplus) -> the solver's face kernel
    template <class FL>
    int sample(hipStream_t stream, double time, FL&& face_launch) {
        ++m.steps;
        MonRings r{};
        for (int q = 0; q < m.n_objects; ++q) {
            Monitors::Obj& o = m.obj[q];
            if (m.steps % o.interval) continue;
            if (o.sampled - o.drained >= m.ring_rows) FY_TRY(m.drain(stream));
            r.due |= 1u << q;
            r.ring[q] = o.ring.p; r.row[q] = (int)(o.sampled % m.ring_rows); r.width[q] = 1 + o.n_values;
        }
        if (!r.due) return FY_OK;
        m.clock.begin(stream);
        WlTable t = tab;
        t.due = r.due;
        FY_TRY(face_launch(t, m.pf.p, m.nblk_f, wss.p, yplus.p));
        FY_TRY(launch_monitor_finalize(stream, m.outs.p, m.n_outs, nullptr, 0, m.pf.p, m.nblk_f, r, time));
        m.clock.end(stream);
        for (int q = 0; q < m.n_objects; ++q) if (r.due >> q & 1) ++m.obj[q].sampled;
        return FY_OK;
    }

    // "wallShearStress_boundary" / "yPlus_boundary" while their objects are on
    bool lookup(const std::string& s, double** ptr, size_t* count) {
        if (s == "wallShearStress_boundary" && wss.p) { *ptr = wss.p; *count = 3 * nb; return true; }
        if (s == "yPlus_boundary" && yplus.p) { *ptr = yplus.p; *count = nb; return true; }
        return false;
    }
};

}  // namespace fy
