// fy::Monitors: volFieldValue / surfaceFieldValue as reductions on the device (the role of OpenFOAM's fieldValue function objects; the arithmetic is theirs as recalled
// from OpenFOAM-6 volFieldValue.C / surfaceFieldValue.C, unpinned: DESIGN.md sections 3 and 5).  x_i = the field in cell i, or its boundary value on face i (phi: the flux
// OUT of the domain); m_i = the cell volume V_i or the face area A_i = |Sf_i|; w_i = the weight field (cells: alpha, faces: phi outward); n = cells / faces:
//     sum  S x_i         average  (S x_i) / n         min, max  over i                                   (S = the sum over i; a vector: per component)
//     volIntegrate / areaIntegrate      S (x_i m_i)          volAverage / areaAverage  (S (x_i m_i)) / (S m_i)
//     weightedVolAverage  (S ((w_i V_i) x_i)) / (S (w_i V_i))                       weightedAverage (faces)  (S (w_i x_i)) / (S w_i)
// Every bracket is one IEEE operation (-ffp-contract=off).  Three kernels per sample, no atomics, no host synchronisation:
//   cells     one lane per four cells (a block's tile: 1024 cells): every distinct source component is read once and leaves the block as five partials -- S x, S x m,
//             S x w', min x, max x (w' = w V) -- whatever and however many objects name it; a source "1" gives n, S V and S w V the same way
//   faces     one lane per boundary face and surface object (the solver's own kernel: it forms the values through the solver's boundary statement)
//   finalize  one workgroup per value of a row: folds the partials of its numerator and denominator in a fixed order, divides, stores into the object's ring
// A partial is the block's fold through mon_block_reduce_store below (wave shuffles, then LDS); lanes and blocks without an item hold the operation's neutral value
// (0, +inf, -inf), which is what the padding blocks of red_blocks() store.  The ring [rows][1 + values] (time first) lives on the device; the host copies rows out when
// it is full or when asked (drain), never in between.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "fv_linalg_kernels.hpp"

namespace fy {

constexpr int kMonKinds = 5;                     // partials per source component: S x, S x m, S x w', min, max
enum { MK_SUM = 0, MK_MSUM, MK_WSUM, MK_MIN, MK_MAX };
constexpr int kMonCellsPerLane = 4;              // k_monitor_cells: a block's tile is 256 x this many cells
inline int mon_cell_blocks(int n_cells) { return red_blocks((n_cells + kMonCellsPerLane - 1) / kMonCellsPerLane); }      // its grid = partials per slot (a multiple of 8)
constexpr int kMonCellComps = 24;                // "1" + the components of every field a volume object may name: 15 of the fluid's and the coupling's fields, 8 of the solid statistics
constexpr int kMonFaceComps = 7;                 // per surface object: "1", phi, p, U x y z, T
enum { MF_ONE = 0, MF_PHI = 1, MF_P = 2, MF_U = 3, MF_T = 6 };

struct MonCellSrc { const double* p; int stride, off; };        // x_i = p[i stride + off]; p null: 1
struct MonCellTable {
    int n;
    MonCellSrc s[kMonCellComps];
    const double* V; double V0;                  // cell volumes, or (null) the one volume of a uniform block
    const double* w;                             // the weight field's cells, or null: no object is weighted (w' = 0)
};
struct MonFaceObj { int patch; int fields; };    // patch index | mask of sides; bit q of fields: component q of kMonFaceComps is wanted (MF_ONE always)
struct MonFaceTable { int n; MonFaceObj o[FY_MONITOR_MAX_OBJECTS]; };
// one value of a row: (numerator slot, denominator slot or -1) of the cell (src 0) or face (src 1) partials, op 0 sum | 1 min | 2 max, ring position
struct MonOut { int src, num, den, op, object, col; };
struct MonRings { double* ring[FY_MONITOR_MAX_OBJECTS]; int row[FY_MONITOR_MAX_OBJECTS]; int width[FY_MONITOR_MAX_OBJECTS]; unsigned due; };

int launch_monitor_cells(hipStream_t s, const MonCellTable& t, int n_cells, double* partials);
int launch_monitor_finalize(hipStream_t s, const MonOut* outs, int n_outs, const double* pc, int nblk_c, const double* pf, int nblk_f, const MonRings& r, double time);

#if defined(__HIPCC__)
// the block's fold of one source component's five values: partials[(slot0 + kind) nblk + block].  Called by every lane of the block, any number of times in a row
__device__ __forceinline__ void mon_block_reduce_store(double (&v)[kMonKinds], double* partials, int slot0, int nblk, int block) {
    __shared__ double mon_sh[4][kMonKinds];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < kMonKinds; ++q) {
        double x = v[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double y = __shfl_down(x, o, 64);
            x = q == MK_MIN ? fmin(x, y) : q == MK_MAX ? fmax(x, y) : x + y;
        }
        if (lane == 0) mon_sh[wv][q] = x;
    }
    __syncthreads();
    if (threadIdx.x < kMonKinds) {
        const int q = threadIdx.x;
        double x = mon_sh[0][q];
        for (int w = 1; w < 4; ++w) x = q == MK_MIN ? fmin(x, mon_sh[w][q]) : q == MK_MAX ? fmax(x, mon_sh[w][q]) : x + mon_sh[w][q];
        partials[(size_t)(slot0 + q) * nblk + block] = x;
    }
    __syncthreads();
}
// the five values of one item: x, x m, w' x, x, x -- or the neutral ones of a lane without an item
__device__ __forceinline__ void mon_terms(bool in, double x, double m, double w, double (&v)[kMonKinds]) {
    v[MK_SUM] = in ? x : 0.0;
    v[MK_MSUM] = in ? x * m : 0.0;
    v[MK_WSUM] = in ? w * x : 0.0;
    v[MK_MIN] = in ? x : INFINITY;
    v[MK_MAX] = in ? x : -INFINITY;
}
#endif

struct Monitors {
    struct Obj {
        std::string name;
        int kind = 0, patch = 0, op = 0, interval = 1;
        std::vector<std::string> fields;
        std::vector<int> comps;
        std::vector<std::string> labels;
        int n_values = 0;
        DevBuf<double> ring;
        int64_t sampled = 0, drained = 0;          // rows produced / rows copied to hist
        std::vector<double> hist;                  // [rows][1 + n_values]
    };
    Obj obj[FY_MONITOR_MAX_OBJECTS];
    int n_objects = 0, ring_rows = 0;
    std::vector<std::string> cell_fields;          // the distinct fields of the volume objects, in order of first mention; slot base of field q: cell_base[q]
    std::vector<int> cell_base, cell_comp;
    bool weighted_cells = false, any_vol = false, any_surf = false;
    MonFaceTable ftab{};
    DevBuf<double> pc, pf;
    DevBuf<MonOut> outs;
    int n_outs = 0, nblk_c = 0, nblk_f = 0;
    size_t n_cells = 0, n_bfaces = 0;
    double start_time = 0.0, elapsed = 0.0;        // elapsed: the sum of the steps' deltaT since the solver was created (counted whether or not anything is monitored)
    int64_t steps = 0;
    KernelClock clock;                             // "monitors" of fy_solver_get_kernel_timing: the sample's launches together
    ~Monitors() { clock.destroy(); }

    bool on() const { return n_objects > 0; }
    void off() {
        for (Obj& o : obj) { o.ring.release(); o.hist.clear(); o.fields.clear(); o.comps.clear(); o.labels.clear(); o.name.clear(); o.sampled = o.drained = 0; o.n_values = 0; }
        n_objects = 0; cell_fields.clear(); cell_base.clear(); cell_comp.clear(); pc.release(); pf.release(); outs.release(); n_outs = 0; steps = 0;
        weighted_cells = any_vol = any_surf = false; ftab = MonFaceTable{};
    }
    static const char* op_name(int op) {
        static const char* const nm[] = {"", "sum", "average", "volAverage", "volIntegrate", "weightedVolAverage", "min", "max", "areaAverage", "areaIntegrate", "weightedAverage"};
        return op >= FY_MONITOR_SUM && op <= FY_MONITOR_WEIGHTED_AVERAGE ? nm[op] : "?";
    }

    // cell(name, &comp) -> whether this solver has the cell field; faces(patch, &why) -> the number of faces of a surface object's patch / side mask (0: refused, why says so);
    // has_T: the case has a temperature
    template <class RC, class RF>
    int configure(const fy_monitor_desc* d, size_t cells, size_t bfaces, bool has_T, hipStream_t stream, const char* who, RC&& cell, RF&& faces) {
        off();
        if (!d || d->n_objects == 0) return FY_OK;
        const int rc = configure_(d, cells, bfaces, has_T, stream, who, cell, faces);
        if (rc != FY_OK) off();
        return rc;
    }
    template <class RC, class RF>
    int configure_(const fy_monitor_desc* d, size_t cells, size_t bfaces, bool has_T, hipStream_t stream, const char* who, RC&& cell, RF&& faces) {
        if (d->n_objects < 0 || d->n_objects > FY_MONITOR_MAX_OBJECTS)
            return fail(FY_ERR_INVALID, "%s: %d objects (at most FY_MONITOR_MAX_OBJECTS = %d)", who, d->n_objects, FY_MONITOR_MAX_OBJECTS);
        if (d->ring_rows < 0) return fail(FY_ERR_INVALID, "%s: ring_rows %d must not be negative", who, d->ring_rows);
        ring_rows = d->ring_rows > 0 ? d->ring_rows : 256;
        n_cells = cells; n_bfaces = bfaces; start_time = d->start_time;
        nblk_c = mon_cell_blocks((int)cells); nblk_f = red_blocks((int)std::max<size_t>(bfaces, 1));
        static const char* const cell_known[] = {"U", "p", "alpha", "uParticle", "uSource", "nut", "k", "epsilon", "T", "nParticle", "solidFraction", "uSolid", "granularTemperature", "dSauter", "TParticle"};
        std::vector<MonOut> ho;
        auto str = [](const char* a, size_t cap) { char b[64] = {0}; std::memcpy(b, a, std::min<size_t>(cap, 63)); return std::string(b); };
        for (int q = 0; q < d->n_objects; ++q) {
            const fy_monitor_object& in = d->objects[q];
            Obj& o = obj[q];
            o.name = str(in.name, sizeof(in.name));
            const char* on = o.name.c_str();
            if (in.kind != FY_MONITOR_VOL && in.kind != FY_MONITOR_SURFACE) return fail(FY_ERR_INVALID, "%s: object '%s': unknown kind %d (FY_MONITOR_VOL, FY_MONITOR_SURFACE)", who, on, in.kind);
            const bool vol = in.kind == FY_MONITOR_VOL;
            o.kind = in.kind; o.patch = in.patch; o.op = in.operation; o.interval = in.interval > 0 ? in.interval : 1;
            if (in.interval < 0) return fail(FY_ERR_INVALID, "%s: object '%s': interval %d (>= 1)", who, on, in.interval);
            const bool vol_op = o.op == FY_MONITOR_VOL_AVERAGE || o.op == FY_MONITOR_VOL_INTEGRATE || o.op == FY_MONITOR_WEIGHTED_VOL_AVERAGE;
            const bool surf_op = o.op == FY_MONITOR_AREA_AVERAGE || o.op == FY_MONITOR_AREA_INTEGRATE || o.op == FY_MONITOR_WEIGHTED_AVERAGE;
            const bool any_op = o.op == FY_MONITOR_SUM || o.op == FY_MONITOR_AVERAGE || o.op == FY_MONITOR_MIN || o.op == FY_MONITOR_MAX;
            if (!(any_op || (vol && vol_op) || (!vol && surf_op)))
                return fail(FY_ERR_INVALID, "%s: object '%s': unknown operation %d '%s' for a %s object (%s)", who, on, o.op, op_name(o.op), vol ? "volume" : "surface",
                            vol ? "sum, average, volAverage, volIntegrate, weightedVolAverage, min, max" : "sum, average, areaAverage, areaIntegrate, weightedAverage, min, max");
            const bool weighted = o.op == FY_MONITOR_WEIGHTED_VOL_AVERAGE || o.op == FY_MONITOR_WEIGHTED_AVERAGE;
            const std::string wf = str(in.weight_field, sizeof(in.weight_field));
            const char* want_w = vol ? "alpha" : "phi";
            if (weighted && wf.empty()) return fail(FY_ERR_INVALID, "%s: object '%s': operation %s needs a weight field (weightField %s)", who, on, op_name(o.op), want_w);
            if (!wf.empty() && wf != want_w) return fail(FY_ERR_INVALID, "%s: object '%s': weight field '%s' (a %s object takes %s)", who, on, wf.c_str(), vol ? "volume" : "surface", want_w);
            int comp = 0;
            if (weighted && vol && !cell("alpha", &comp)) return fail(FY_ERR_INVALID, "%s: object '%s': weight field 'alpha' does not exist in this case", who, on);
            if (in.n_fields < 1 || in.n_fields > FY_MONITOR_MAX_FIELDS)
                return fail(FY_ERR_INVALID, "%s: object '%s': %d fields (1 to FY_MONITOR_MAX_FIELDS = %d)", who, on, in.n_fields, FY_MONITOR_MAX_FIELDS);
            int face_base = 0;
            if (!vol) {
                std::string why;
                if (faces(in.patch, &why) <= 0) return fail(FY_ERR_INVALID, "%s: object '%s': %s", who, on, why.c_str());
                face_base = ftab.n * kMonFaceComps * kMonKinds;
                ftab.o[ftab.n].patch = in.patch; ftab.o[ftab.n].fields = 1 << MF_ONE;
            }
            for (int f = 0; f < in.n_fields; ++f) {
                const std::string nm = str(in.fields[f], sizeof(in.fields[f]));
                int base = 0, one = 0;          // first slot of the field's first component, of "1"
                comp = 0;
                if (vol) {
                    bool ok = false;
                    for (const char* k : cell_known) ok = ok || nm == k;
                    if (!ok || !cell(nm, &comp))
                        return fail(FY_ERR_INVALID, "%s: object '%s': field '%s' %s (U, p, alpha, uParticle, uSource, nut, k, epsilon, T, nParticle, solidFraction, uSolid, granularTemperature, dSauter, TParticle, where the solver has the field)", who, on, nm.c_str(),
                                    ok ? "does not exist in this case" : "is unknown");
                    size_t at = 0;
                    while (at < cell_fields.size() && cell_fields[at] != nm) ++at;
                    if (at == cell_fields.size()) {
                        int nextc = 1;
                        for (int c : cell_comp) nextc += c;
                        if (nextc + comp > kMonCellComps) return fail(FY_ERR_INVALID, "%s: object '%s': too many distinct field components (%d)", who, on, kMonCellComps - 1);
                        cell_fields.push_back(nm); cell_comp.push_back(comp); cell_base.push_back(nextc * kMonKinds);
                    }
                    base = cell_base[at];
                } else {
                    const int at = nm == "phi" ? MF_PHI : nm == "p" ? MF_P : nm == "U" ? MF_U : nm == "T" ? MF_T : -1;
                    if (at < 0 || (at == MF_T && !has_T))
                        return fail(FY_ERR_INVALID, "%s: object '%s': field '%s' %s (a surface object takes phi, p, U, T)", who, on, nm.c_str(), at < 0 ? "is unknown" : "does not exist in this case");
                    comp = at == MF_U ? 3 : 1;
                    for (int c = 0; c < comp; ++c) ftab.o[ftab.n].fields |= 1 << (at + c);
                    base = face_base + at * kMonKinds; one = face_base;
                }
                for (int r = 0; r < (int)o.fields.size(); ++r)
                    if (o.fields[r] == nm) return fail(FY_ERR_INVALID, "%s: object '%s': field '%s' is listed twice", who, on, nm.c_str());
                o.fields.push_back(nm); o.comps.push_back(comp);
                for (int c = 0; c < comp; ++c) {
                    MonOut e{vol ? 0 : 1, 0, -1, 0, q, o.n_values};
                    const int s0 = base + c * kMonKinds;
                    switch (o.op) {
                        case FY_MONITOR_SUM: e.num = s0 + MK_SUM; break;
                        case FY_MONITOR_AVERAGE: e.num = s0 + MK_SUM; e.den = one + MK_SUM; break;
                        case FY_MONITOR_VOL_INTEGRATE: case FY_MONITOR_AREA_INTEGRATE: e.num = s0 + MK_MSUM; break;
                        case FY_MONITOR_VOL_AVERAGE: case FY_MONITOR_AREA_AVERAGE: e.num = s0 + MK_MSUM; e.den = one + MK_MSUM; break;
                        case FY_MONITOR_WEIGHTED_VOL_AVERAGE: case FY_MONITOR_WEIGHTED_AVERAGE: e.num = s0 + MK_WSUM; e.den = one + MK_WSUM; break;
                        case FY_MONITOR_MIN: e.num = s0 + MK_MIN; e.op = 1; break;
                        default: e.num = s0 + MK_MAX; e.op = 2; break;
                    }
                    ho.push_back(e);
                    static const char* const xyz[] = {"_x", "_y", "_z"};
                    o.labels.push_back(std::string(op_name(o.op)) + "(" + nm + ")" + (comp == 3 ? xyz[c] : ""));
                    ++o.n_values;
                }
            }
            if (vol) { any_vol = true; weighted_cells = weighted_cells || weighted; }
            else { any_surf = true; ++ftab.n; }
            FY_TRY(o.ring.alloc_exact((size_t)ring_rows * (size_t)(1 + o.n_values)));
            n_objects = q + 1;
        }
        int ncc = 1;
        for (int c : cell_comp) ncc += c;
        if (any_vol) FY_TRY(pc.alloc_exact((size_t)ncc * kMonKinds * (size_t)nblk_c));
        if (any_surf) FY_TRY(pf.alloc_exact((size_t)ftab.n * kMonFaceComps * kMonKinds * (size_t)nblk_f));
        n_outs = (int)ho.size();
        FY_TRY(outs.alloc_exact(ho.size()));
        FY_HIP(hipMemcpyAsync(outs.p, ho.data(), ho.size() * sizeof(MonOut), hipMemcpyHostToDevice, stream));
        // (a face partial that no wanted component writes is never read: every MonOut names a component its object asked for, or "1")
        FY_HIP(hipStreamSynchronize(stream));
        return FY_OK;
    }

    // copy the rows the device has produced and the host has not yet seen into the history (waits for the stream)
    int drain(hipStream_t stream) {
        bool any = false;
        for (int q = 0; q < n_objects; ++q) any = any || obj[q].drained < obj[q].sampled;
        if (!any) return FY_OK;
        FY_HIP(hipStreamSynchronize(stream));
        for (int q = 0; q < n_objects; ++q) {
            Obj& o = obj[q];
            const size_t w = (size_t)(1 + o.n_values);
            while (o.drained < o.sampled) {
                const int64_t r0 = o.drained % ring_rows;
                const int64_t nr = std::min<int64_t>(o.sampled - o.drained, ring_rows - r0);
                const size_t at = o.hist.size();
                o.hist.resize(at + (size_t)nr * w);
                FY_HIP(hipMemcpy(o.hist.data() + at, o.ring.p + (size_t)r0 * w, (size_t)nr * w * sizeof(double), hipMemcpyDeviceToHost));
                o.drained += nr;
            }
        }
        return FY_OK;
    }

    // the step that has just finished: cell(name, &comp) -> the field's owned cells as they lie now; face_launch(table, partials, nblk) -> the solver's face kernel
    template <class RC, class FL>
    int sample(hipStream_t stream, const double* V, double V0, RC&& cell, FL&& face_launch) {
        ++steps;
        MonRings r{};
        bool vol_due = false, surf_due = false;
        for (int q = 0; q < n_objects; ++q) {
            Obj& o = obj[q];
            if (steps % o.interval) continue;
            if (o.sampled - o.drained >= ring_rows) FY_TRY(drain(stream));          // the ring is full: the one place where sampling meets the host
            r.due |= 1u << q;
            r.ring[q] = o.ring.p; r.row[q] = (int)(o.sampled % ring_rows); r.width[q] = 1 + o.n_values;
            (o.kind == FY_MONITOR_VOL ? vol_due : surf_due) = true;
        }
        if (!r.due) return FY_OK;
        clock.begin(stream);
        if (vol_due) {
            MonCellTable t{};
            t.n = 1; t.s[0] = MonCellSrc{nullptr, 0, 0};
            for (size_t f = 0; f < cell_fields.size(); ++f) {
                int comp = 0;
                const double* p = cell(cell_fields[f], &comp);
                if (!p || comp != cell_comp[f]) return fail(FY_ERR_INVALID, "monitors: field '%s' is gone", cell_fields[f].c_str());
                for (int c = 0; c < comp; ++c) t.s[t.n++] = MonCellSrc{p, comp, c};
            }
            t.V = V; t.V0 = V0;
            if (weighted_cells) { int comp = 0; t.w = cell("alpha", &comp); if (!t.w) return fail(FY_ERR_INVALID, "monitors: weight field 'alpha' is gone"); }
            FY_TRY(launch_monitor_cells(stream, t, (int)n_cells, pc.p));
        }
        if (surf_due) FY_TRY(face_launch(ftab, pf.p, nblk_f));
        FY_TRY(launch_monitor_finalize(stream, outs.p, n_outs, pc.p, nblk_c, pf.p, nblk_f, r, start_time + elapsed));
        clock.end(stream);
        for (int q = 0; q < n_objects; ++q) if (r.due >> q & 1) ++obj[q].sampled;
        return FY_OK;
    }

    int layout(int object, int32_t* n_values, char* labels, int cap) const {
        if (object < 0 || object >= n_objects) return fail(FY_ERR_INVALID, "monitors: object %d of %d", object, n_objects);
        const Obj& o = obj[object];
        if (n_values) *n_values = o.n_values;
        if (labels) {
            std::string all;
            for (size_t q = 0; q < o.labels.size(); ++q) all += (q ? "\n" : "") + o.labels[q];
            if ((int)all.size() + 1 > cap) return fail(FY_ERR_INVALID, "monitors: the labels of object '%s' need %zu bytes", o.name.c_str(), all.size() + 1);
            std::memcpy(labels, all.c_str(), all.size() + 1);
        }
        return FY_OK;
    }
    int get_rows(hipStream_t stream, int object, int64_t first_row, int64_t max_rows, double* times, double* values, int64_t* n_rows) {
        if (object < 0 || object >= n_objects) return fail(FY_ERR_INVALID, "monitors: object %d of %d", object, n_objects);
        if (!n_rows || first_row < 0 || max_rows < 0) return fail(FY_ERR_INVALID, "monitors: null n_rows, or a negative first_row / max_rows");
        FY_TRY(drain(stream));
        Obj& o = obj[object];
        const size_t w = (size_t)(1 + o.n_values);
        int64_t have = (int64_t)(o.hist.size() / w) - first_row;
        if (have < 0) have = 0;
        if (!times && !values) { *n_rows = have; return FY_OK; }
        have = std::min(have, max_rows);
        for (int64_t r = 0; r < have; ++r) {
            const double* row = o.hist.data() + (size_t)(first_row + r) * w;
            if (times) times[r] = row[0];
            if (values) std::memcpy(values + (size_t)r * o.n_values, row + 1, (size_t)o.n_values * sizeof(double));
        }
        *n_rows = have;
        return FY_OK;
    }
};

}  // namespace fy
