// OpenFOAM case directories for fy_solver: what icoFoamYade / pimpleFoamYade get from OpenFOAM's runTime / mesh / field
// constructors (icoFoamYade.C:38-46, createFields.H of both solvers) and give back with runTime.write() (icoFoamYade.C:142,
// pimpleFoamYade.C:107), for the one mesh class this library computes on: a single axis-aligned blockMesh hex block (uniform cubes, or graded: simpleGrading (ex ey ez)).
//   read   system/blockMeshDict  (vertices, one `hex` block, simpleGrading (ex ey ez), `boundary` patches -> the 6 box sides)
//          system/controlDict    (startTime, endTime, deltaT, writeControl, writeInterval)
//          system/fvSolution     (PISO | PIMPLE controls, solvers.p / pFinal / U tolerances)
//          constant/transportProperties (nu, partDensity, fluidDensity | continuousPhaseName + rho.<phase>), constant/g
//          <startTime>/U | U.<phase>, <startTime>/p  (boundary types fixedValue / noSlip / zeroGradient / fixedFluxPressure;
//                                                    internalField uniform or nonuniform)
//   write  <time>/U | U.<phase>, p, and in Gaussian mode alpha.<phase>: ASCII volFields with the case's own patch entries
// Anything outside that subset is refused with FY_ERR_UNSUPPORTED and a message naming the file and keyword -- never guessed.
#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "common.hpp"
#include "foam_dict.hpp"
#include "ldu.hpp"

// a case's fields (the order of fy_case_desc's and fy_ldu_case's condition arrays); alpha is written only, it has no start-time file
enum { F_U, F_P, F_NUT, F_K, F_EPS, F_ALPHA, F_T };      // (F_T: the temperature of a case with heatTransfer active)

// one field's boundary conditions, indexed by the case's patch list (field_patches): per patch the FY_BC_* code, the value (U: three), and the
// boundaryField entry as read, re-emitted on write; extra: a block case's entries of other names (a decomposed case's processor patches), as read
struct PatchField {
    std::vector<int32_t> bc;
    std::vector<double> val;
    std::vector<std::string> text;
    std::vector<std::pair<std::string, std::string> > extra;
};

struct fy_foam_case {
    std::string dir;
    int solver = FY_SOLVER_ICO;
    fy_case_desc desc{};
    std::string phase, u_name, start_name;
    double start_time = 0, end_time = 0;
    int write_interval_steps = 0;
    std::string patch_of_side[6];               // blockMesh patch name covering XMIN, XMAX, YMIN, YMAX, ZMIN, ZMAX
    std::vector<double> grading[3];             // graded block: cell sizes per axis (fy_case_desc.hx / hy / hz point here)
    std::vector<std::string> patch_order;       // patch names in blockMeshDict order (one side each here)
    std::vector<double> U0, p0, nut0, k0, eps0; // internalField of the start time (nut0, k0, eps0: turbulence cases only)
    std::vector<double> T0;                     // ... of T | T.<phase> (heatTransfer active)
    PatchField bcs[7];                          // per field (U, p, nut, k, epsilon; F_ALPHA unused; T): the start time's boundary conditions
    // controlDict's output settings [OF-6 Time::readDict]: writeFormat ascii | binary, writePrecision (ASCII digits; absent: 17, lossless --
    // OpenFOAM's own default of 6 would not restart a run where it stopped), purgeWrite N (keep the N newest time directories this run wrote)
    bool write_binary = false;
    int write_precision = 17;
    int purge_write = 0;
    mutable std::vector<std::string> written;   // time directories written so far (purgeWrite's ring)
    // A DECOMPOSED case (decomposePar, simple (1 1 N): processorR = the R-th z-slab, its cells in the global order): the field files are read
    // from and written to <case>/processorR, hold the slab's cells only, and carry the processor patches (procBoundaryRtoS) next to the case's own
    std::string fdir;                           // where the time directories are: dir, or dir/processorR
    size_t fcells = 0, foffset = 0;             // cells per field file, global number of the first one
    int proc_rank = -1, proc_count = 0;
    // constant/polyMesh read instead of blockMeshDict: the mesh's cell numbers may differ from the lattice's (several blocks): file_cell[L] = the mesh's
    // cell at lattice index L = i + nx (j + ny k); empty = the same numbering (one block)
    std::vector<int32_t> file_cell;
    // A GENERAL polyhedral mesh (fy_foam_case_open_general: whatever createMesh.H would hand icoFoamYade, icoFoamYade.C:42): constant/polyMesh's arrays
    // as read, every patch of the boundary file in its order, and per patch the conditions fy_ldu_solver takes.  desc then only carries the controls
    bool general = false;
    int g_cells = 0, g_internal = 0;
    std::vector<double> g_points;
    std::vector<int32_t> g_face_off, g_face_pts, g_own, g_nei, g_patch_start, g_patch_size;
    std::vector<std::string> g_patch_name;
    std::vector<int32_t> g_patch_neighbour;      // per patch: its cyclic partner, or -1
    std::vector<std::string> g_patch_class;      // the boundary file's `type` per patch (wall | patch | symmetryPlane | symmetry | cyclic)
    fy_flow_control_desc flow{};                 // constant/couplingProperties meanVelocityForce (general cases only; fy_ldu_case.flow_control)
    // constant/couplingProperties porousZones (block and general cases; fy_foam_case_porous_zones hands them out as a fy_porous_desc): the active zones in file order,
    // the cells as solver cell labels -- those whose centre lies in the closed box (boxToCell)
    struct PorousMeta { std::string name; double d[3] = {0, 0, 0}, f[3] = {0, 0, 0}, lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}; std::vector<int32_t> cells; };
    std::vector<PorousMeta> porous;
    // controlDict functions: the fieldAverage object (desc.average carries its items in this order) and the names of the objects of other types
    struct AvgField { std::string file; int F; std::string solver_name; int ncomp; bool prime2; };      // F: F_U .. F_ALPHA, or -1 (uParticle, uSource: no start-time file)
    std::string avg_name;
    std::vector<AvgField> avg_fields;
    bool avg_restart_on_restart = false;
    std::vector<std::string> ignored_functions;
    // ... and the volFieldValue / surfaceFieldValue objects (desc.monitors carries them in this order): the region's name ("all" | the patch), the fields' file
    // names, and how many rows of the solver's history fy_foam_case_write_monitors has put into the object's .dat file
    struct MonMeta { std::string name, region; bool vol = true; std::vector<std::string> files; std::vector<int> ncomp; mutable int64_t rows_written = 0; };
    std::vector<MonMeta> monitors;
    // ... and the forces / wallShearStress / yPlus objects (desc.wall_loads carries them; the solver numbers them forces first, then wallShearStress, then yPlus):
    // kind 0 forces | 1 wallShearStress | 2 yPlus, the patch names in the order of the object's row, the rows fy_foam_case_write_wall_loads has written
    struct WlMeta { std::string name; int kind = 0; std::vector<std::string> patches; mutable int64_t rows_written = 0; };
    std::vector<WlMeta> wl_forces, wl_wss, wl_yplus;
    std::vector<const WlMeta*> wall_loads() const {
        std::vector<const WlMeta*> v;
        for (const auto* l : {&wl_forces, &wl_wss, &wl_yplus}) for (const WlMeta& m : *l) v.push_back(&m);
        return v;
    }
    std::string class_of_side[6];               // a block's patch type per side (wall | patch | symmetryPlane ...): the default patch set of wallShearStress / yPlus
    // inlets (fy_inlets_desc; DESIGN.md section 3 "Inlets"): the velocity patches whose entry is fixedValue with a nonuniform list, uniformFixedValue or
    // flowRateInletVelocity.  patch: the side of a block, the patch index of a general mesh; a per-face shape lies in "U_boundary"'s order on that side or patch
    struct InletTerm { fy_time_function f{}; std::vector<double> pts; int shape_kind = FY_SHAPE_UNIFORM; std::vector<double> shape; };
    struct Inlet { int patch = 0; std::vector<InletTerm> terms; };
    std::vector<Inlet> inlets;
    mutable std::vector<fy_inlet_desc> inlet_descs;      // what fy_foam_case_desc / fy_foam_case_ldu_desc hand out: pointers into `inlets`
    // a block read from constant/polyMesh: per side, for face r of the side in "U_boundary"'s order, its place in its PATCH's face list (empty: blockMeshDict alone,
    // where blockMesh's face order cannot be verified)
    std::vector<int32_t> side_face_src[6];
    mutable std::vector<double> u_boundary_now;          // fy_foam_case_write_time*: the solver's "U_boundary" while the fields are written (the inlet patches' `value`)
};

namespace {

using fy::fail;
using fy::FoamDict;

std::string join(const std::string& a, const std::string& b) { return a + "/" + b; }

bool file_exists(const std::string& path) { struct stat st; return stat(path.c_str(), &st) == 0 && S_ISREG(st.st_mode); }

int need_file(const std::string& path, FoamDict* d) {
    std::string err;
    if (!fy::foam_parse_file(path, d, &err)) return fail(FY_ERR_INVALID, "%s", err.c_str());
    return FY_OK;
}

// `name { ... } name { ... }` inside a token list -> named dictionaries, in order
int named_dicts(const std::vector<std::string>& tok, const std::string& what, std::vector<std::pair<std::string, FoamDict> >* out) {
    size_t i = 0;
    double cnt;
    if (i < tok.size() && fy::foam_tok_is_number(tok[i], &cnt)) ++i;
    if (i >= tok.size() || tok[i] != "(") return fail(FY_ERR_INVALID, "%s: expected a list", what.c_str());
    ++i;
    while (i < tok.size() && tok[i] != ")") {
        const std::string name = tok[i++];
        if (i >= tok.size() || tok[i] != "{") return fail(FY_ERR_INVALID, "%s: expected '{' after '%s'", what.c_str(), name.c_str());
        int depth = 0;
        std::string text;
        for (; i < tok.size(); ++i) {
            if (tok[i] == "{") { if (depth++ == 0) continue; }
            if (tok[i] == "}") { if (--depth == 0) { ++i; break; } }
            text += tok[i];
            text += ' ';
        }
        if (depth != 0) return fail(FY_ERR_INVALID, "%s: unbalanced braces in '%s'", what.c_str(), name.c_str());
        FoamDict d;
        std::string err;
        if (!fy::foam_parse(text, &d, &err)) return fail(FY_ERR_INVALID, "%s: patch '%s': %s", what.c_str(), name.c_str(), err.c_str());
        out->emplace_back(name, d);
    }
    return FY_OK;
}

bool near(double a, double b, double scale) { return std::fabs(a - b) <= 1e-9 * scale; }

// one direction of one hex block: its cell sizes from the grading [OF-6 blockMesh lineDivide.C, gradingDescriptor(s).C].  A grading is a list of
// sections (fraction of the length, fraction of the cells, expansion ratio = last cell / first cell of the section); `simpleGrading (2 ...)` is the
// one-section list ((1 1 2)).  Fractions are normalised to sum 1; a section holds label(nDivFrac * n + 0.5) cells, the last one what is left;
// inside a section the sizes form a geometric progression with factor ratio^(1 / (cells - 1)); a negative ratio r means 1 / |r|
struct GradSection { double len, cells, ratio; };
int axis_sizes(const std::string& path, int n, double L, std::vector<GradSection> sec, std::vector<double>* h) {
    double sl = 0.0, sc = 0.0;
    for (GradSection& g : sec) {
        if (!(g.len > 0) || !(g.cells > 0) || g.ratio == 0.0) return fail(FY_ERR_INVALID, "%s: grading section (%g %g %g): fractions must be positive, the ratio non-zero", path.c_str(), g.len, g.cells, g.ratio);
        if (g.ratio < 0) g.ratio = 1.0 / -g.ratio;
        sl += g.len; sc += g.cells;
    }
    h->clear();
    int start = 0;
    for (size_t q = 0; q < sec.size(); ++q) {
        int m = (int)(sec[q].cells / sc * n + 0.5);
        if (q + 1 == sec.size() || m > n - start) m = n - start;
        if (m < 1) return fail(FY_ERR_INVALID, "%s: a grading section is left without cells (%d cells over %zu sections)", path.c_str(), n, sec.size());
        const double len = sec[q].len / sl * L;
        const double r = (sec[q].ratio != 1.0 && m > 1) ? std::pow(sec[q].ratio, 1.0 / (m - 1)) : 1.0;
        double sum = 0.0, w = 1.0;
        const size_t at = h->size();
        for (int i = 0; i < m; ++i) { h->push_back(w); sum += w; w *= r; }
        for (size_t i = at; i < h->size(); ++i) (*h)[i] *= len / sum;
        start += m;
    }
    if (start != n) return fail(FY_ERR_INVALID, "%s: the grading sections hold %d of %d cells", path.c_str(), start, n);
    return FY_OK;
}

struct HexBlock { int hv[8]; int nn[3]; double lo[3], hi[3]; std::vector<double> h[3]; };

// system/blockMeshDict: one hex block, or several that tile a box as a tensor product (Bx x By x Bz blocks, every one present, neighbours
// agreeing on the cell sizes along the faces they share -- what blockMesh merges into one rectilinear lattice); simpleGrading with one
// expansion ratio or a multi-grading list per direction.  Curved edges, edgeGrading, mergePatchPairs and sides shared by two patches are refused.
int read_block_mesh(fy_foam_case* c) {
    const std::string path = join(c->dir, "system/blockMeshDict");
    FoamDict d;
    FY_TRY(need_file(path, &d));
    double scale = 1.0;
    if (!d.scalar("convertToMeters", &scale)) d.scalar("scale", &scale);
    const auto* vt = d.tokens("vertices");
    std::vector<double> v;
    if (!vt || !fy::foam_read_list(*vt, 0, 3, &v) || v.size() < 24 || v.size() % 3 != 0)
        return fail(FY_ERR_UNSUPPORTED, "%s: need at least 8 vertices (x y z)", path.c_str());
    for (double& x : v) x *= scale;
    const int nvert = (int)(v.size() / 3);
    for (const char* key : {"edges", "mergePatchPairs"}) {
        const auto* et = d.tokens(key);
        if (et) for (const std::string& t : *et) if (t != "(" && t != ")") return fail(FY_ERR_UNSUPPORTED, "%s: a non-empty '%s' list is not supported (straight edges, conforming blocks)", path.c_str(), key);
    }
    const auto* bt = d.tokens("blocks");
    double lead;
    const size_t t0 = (bt && !bt->empty() && fy::foam_tok_is_number((*bt)[0], &lead)) ? 1 : 0;      // (an optional element count before the list)
    if (!bt || bt->size() < 24 + t0 || (*bt)[t0] != "(" || (*bt)[t0 + 1] != "hex") return fail(FY_ERR_UNSUPPORTED, "%s: blocks must hold 'hex' blocks", path.c_str());
    const std::vector<std::string>& T = *bt;
    std::vector<HexBlock> blocks;
    size_t i = t0 + 1;
    auto num = [&](double* x) { return i < T.size() && fy::foam_tok_is_number(T[i], x) ? (++i, true) : false; };
    auto tok = [&](const char* w) { return i < T.size() && T[i] == w ? (++i, true) : false; };
    double scl = 0.0;
    while (i < T.size() && T[i] != ")") {
        HexBlock B;
        if (!tok("hex") || !tok("(")) return fail(FY_ERR_UNSUPPORTED, "%s: blocks must hold 'hex' blocks", path.c_str());
        for (int q = 0; q < 8; ++q) { double x; if (!num(&x)) return fail(FY_ERR_INVALID, "%s: malformed hex vertex list", path.c_str()); B.hv[q] = (int)x; }
        if (!tok(")")) return fail(FY_ERR_INVALID, "%s: malformed hex vertex list", path.c_str());
        if (i < T.size() && T[i] != "(") ++i;                                   // (an optional cellZone name)
        if (!tok("(")) return fail(FY_ERR_INVALID, "%s: malformed hex cell counts", path.c_str());
        for (int q = 0; q < 3; ++q) { double x; if (!num(&x)) return fail(FY_ERR_INVALID, "%s: malformed hex cell counts", path.c_str()); B.nn[q] = (int)x; }
        if (!tok(")")) return fail(FY_ERR_INVALID, "%s: malformed hex cell counts", path.c_str());
        if (!tok("simpleGrading")) return fail(FY_ERR_UNSUPPORTED, "%s: only simpleGrading is supported (no edgeGrading)", path.c_str());
        if (!tok("(")) return fail(FY_ERR_INVALID, "%s: malformed simpleGrading", path.c_str());
        std::vector<GradSection> grad[3];
        for (int a = 0; a < 3; ++a) {
            double r;
            if (num(&r)) { grad[a].push_back(GradSection{1.0, 1.0, r}); continue; }
            if (!tok("(")) return fail(FY_ERR_INVALID, "%s: simpleGrading takes an expansion ratio or a list ((fraction cells ratio) ...) per direction", path.c_str());
            while (tok("(")) {
                GradSection g;
                if (!num(&g.len) || !num(&g.cells) || !num(&g.ratio) || !tok(")")) return fail(FY_ERR_INVALID, "%s: malformed multi-grading section (fraction cells ratio)", path.c_str());
                grad[a].push_back(g);
            }
            if (!tok(")") || grad[a].empty()) return fail(FY_ERR_INVALID, "%s: malformed multi-grading list", path.c_str());
        }
        if (!tok(")")) return fail(FY_ERR_INVALID, "%s: simpleGrading takes three entries", path.c_str());
        for (int q = 0; q < 8; ++q) if (B.hv[q] < 0 || B.hv[q] >= nvert) return fail(FY_ERR_INVALID, "%s: hex vertex label out of range", path.c_str());
        auto P = [&](int q, int a) { return v[3 * (size_t)B.hv[q] + a]; };
        // blockMesh's hex: 0-1 = local x, 0-3 = local y, 0-4 = local z; require them to be +x, +y, +z of an axis-aligned box
        const double L[3] = {P(1, 0) - P(0, 0), P(3, 1) - P(0, 1), P(4, 2) - P(0, 2)};
        const double bs = std::fabs(L[0]) + std::fabs(L[1]) + std::fabs(L[2]);
        scl = std::max(scl, bs);
        const int bits[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
        for (int q = 0; q < 8; ++q)
            for (int a = 0; a < 3; ++a)
                if (!near(P(q, a), P(0, a) + bits[q][a] * L[a], bs)) return fail(FY_ERR_UNSUPPORTED, "%s: every block must be an axis-aligned box with the standard hex vertex order", path.c_str());
        if (!(L[0] > 0 && L[1] > 0 && L[2] > 0) || B.nn[0] < 1 || B.nn[1] < 1 || B.nn[2] < 1) return fail(FY_ERR_INVALID, "%s: degenerate block", path.c_str());
        for (int a = 0; a < 3; ++a) {
            B.lo[a] = P(0, a); B.hi[a] = P(0, a) + L[a];
            FY_TRY(axis_sizes(path, B.nn[a], L[a], grad[a], &B.h[a]));
        }
        blocks.push_back(B);
    }
    if (blocks.empty()) return fail(FY_ERR_UNSUPPORTED, "%s: blocks must hold 'hex' blocks", path.c_str());
    // ---- the blocks as a tensor product: break points per axis, one block per slot, equal sizes along shared intervals
    std::vector<double> brk[3];
    for (int a = 0; a < 3; ++a) {
        for (const HexBlock& B : blocks) { brk[a].push_back(B.lo[a]); brk[a].push_back(B.hi[a]); }
        std::sort(brk[a].begin(), brk[a].end());
        std::vector<double> u;
        for (double x : brk[a]) if (u.empty() || !near(x, u.back(), scl)) u.push_back(x);
        brk[a].swap(u);
    }
    const size_t nslot[3] = {brk[0].size() - 1, brk[1].size() - 1, brk[2].size() - 1};
    if (nslot[0] * nslot[1] * nslot[2] != blocks.size())
        return fail(FY_ERR_UNSUPPORTED, "%s: the %zu blocks do not tile a box as a %zu x %zu x %zu tensor product (L-shaped or partly refined arrangements are not supported)", path.c_str(),
                    blocks.size(), nslot[0], nslot[1], nslot[2]);
    std::vector<int> taken(blocks.size(), 0);
    std::vector<const std::vector<double>*> hs[3];
    for (int a = 0; a < 3; ++a) hs[a].assign(nslot[a], nullptr);
    for (const HexBlock& B : blocks) {
        size_t at[3];
        for (int a = 0; a < 3; ++a) {
            size_t q = 0;
            while (q < nslot[a] && !near(brk[a][q], B.lo[a], scl)) ++q;
            if (q == nslot[a] || !near(brk[a][q + 1], B.hi[a], scl)) return fail(FY_ERR_UNSUPPORTED, "%s: a block spans more than one interval of the block lattice (not a tensor-product arrangement)", path.c_str());
            at[a] = q;
            if (!hs[a][q]) hs[a][q] = &B.h[a];
            else {
                const std::vector<double>& o = *hs[a][q];
                bool same = o.size() == B.h[a].size();
                for (size_t m = 0; same && m < o.size(); ++m) same = near(o[m], B.h[a][m], o[m]);
                if (!same) return fail(FY_ERR_UNSUPPORTED, "%s: neighbouring blocks disagree on the cell sizes along a shared direction (non-conforming blocks)", path.c_str());
            }
        }
        int& t = taken[at[0] + nslot[0] * (at[1] + nslot[1] * at[2])];
        if (t++) return fail(FY_ERR_INVALID, "%s: two blocks occupy the same place", path.c_str());
    }
    double L[3], lo[3];
    int nn[3];
    std::vector<double> h[3];
    for (int a = 0; a < 3; ++a) {
        for (size_t q = 0; q < nslot[a]; ++q) h[a].insert(h[a].end(), hs[a][q]->begin(), hs[a][q]->end());
        nn[a] = (int)h[a].size(); lo[a] = brk[a].front(); L[a] = brk[a].back() - brk[a].front();
    }
    const double dx = L[0] / nn[0];
    bool cubes = true;
    for (int a = 0; a < 3; ++a) for (double x : h[a]) cubes = cubes && near(x, dx, dx);
    c->desc.nx = nn[0]; c->desc.ny = nn[1]; c->desc.nz = nn[2]; c->desc.dx = dx;
    c->desc.hx = c->desc.hy = c->desc.hz = nullptr;
    if (!cubes) {       // a graded block (or uniform cells that are not cubes): per-axis cell sizes
        for (int a = 0; a < 3; ++a) c->grading[a] = h[a];
        c->desc.hx = c->grading[0].data(); c->desc.hy = c->grading[1].data(); c->desc.hz = c->grading[2].data();
    }
    for (int a = 0; a < 3; ++a) c->desc.origin[a] = lo[a];

    const auto* bd = d.tokens("boundary");
    if (!bd) return fail(FY_ERR_UNSUPPORTED, "%s: no 'boundary' list (the old 'patches' syntax is not supported)", path.c_str());
    std::vector<std::pair<std::string, FoamDict> > patches;
    FY_TRY(named_dicts(*bd, path + ": boundary", &patches));
    double covered[6] = {0, 0, 0, 0, 0, 0};
    for (auto& pd : patches) {
        const auto* ft = pd.second.tokens("faces");
        std::vector<double> f;
        if (!ft) return fail(FY_ERR_INVALID, "%s: patch '%s' has no faces", path.c_str(), pd.first.c_str());
        // ( (a b c d) (a b c d) ... ): read as 4-component tuples
        if (!fy::foam_read_list(*ft, 0, 4, &f) || f.empty()) return fail(FY_ERR_INVALID, "%s: patch '%s': malformed faces list", path.c_str(), pd.first.c_str());
        std::string ty;
        if (pd.second.word("type", &ty) && (ty == "empty" || ty == "cyclic" || ty == "wedge"))
            return fail(FY_ERR_UNSUPPORTED, "%s: patch '%s' of type '%s' is not supported (wall / patch / symmetryPlane sides of a 3-D box)", path.c_str(), pd.first.c_str(), ty.c_str());
        for (size_t q = 0; q + 3 < f.size(); q += 4) {
            int side = -1;
            double flo[3] = {1e300, 1e300, 1e300}, fhi[3] = {-1e300, -1e300, -1e300};
            for (int m = 0; m < 4; ++m) {
                const int vi = (int)f[q + m];
                if (vi < 0 || vi >= nvert) return fail(FY_ERR_INVALID, "%s: patch '%s': vertex label out of range", path.c_str(), pd.first.c_str());
                for (int a = 0; a < 3; ++a) { flo[a] = std::min(flo[a], v[3 * (size_t)vi + a]); fhi[a] = std::max(fhi[a], v[3 * (size_t)vi + a]); }
            }
            for (int a = 0; a < 3 && side < 0; ++a)
                for (int s = 0; s < 2 && side < 0; ++s)
                    if (near(flo[a], lo[a] + s * L[a], scl) && near(fhi[a], lo[a] + s * L[a], scl)) side = 2 * a + s;
            if (side < 0) return fail(FY_ERR_UNSUPPORTED, "%s: patch '%s' has a face that is not a side of the block", path.c_str(), pd.first.c_str());
            if (!c->patch_of_side[side].empty() && c->patch_of_side[side] != pd.first)
                return fail(FY_ERR_UNSUPPORTED, "%s: side %d of the box is shared by the patches '%s' and '%s' (one boundary condition per side)", path.c_str(), side, c->patch_of_side[side].c_str(), pd.first.c_str());
            c->patch_of_side[side] = pd.first;
            c->class_of_side[side] = ty.empty() ? "patch" : ty;
            const int a = side / 2, t1 = (a + 1) % 3, t2 = (a + 2) % 3;
            covered[side] += (fhi[t1] - flo[t1]) * (fhi[t2] - flo[t2]);
        }
        c->patch_order.push_back(pd.first);
    }
    for (int s = 0; s < 6; ++s) {
        if (c->patch_of_side[s].empty()) return fail(FY_ERR_INVALID, "%s: block side %d belongs to no patch", path.c_str(), s);
        const int a = s / 2;
        const double area = L[(a + 1) % 3] * L[(a + 2) % 3];
        if (!near(covered[s], area, area)) return fail(FY_ERR_INVALID, "%s: block side %d is covered %s by its patch's faces (%g of %g)", path.c_str(), s, covered[s] > area ? "more than once" : "only in part", covered[s], area);
    }
    return FY_OK;
}

// constant/polyMesh (points, faces, owner, neighbour, boundary: what the reference's solvers read -- createMesh.H -- and blockMesh wrote): accepted
// when it is a rectilinear lattice of hexahedra filling an axis-aligned box, i.e. what blockMesh makes of the block arrangements read_block_mesh
// takes.  The lattice comes from the distinct point coordinates; a cell's place in it from the smallest corner of its faces' points; its number in the
// mesh need not be the lattice's (blocks are numbered one after the other): file_cell keeps the map, and the field files are read and written through it.
int read_poly_mesh(fy_foam_case* c) {
    const std::string base = join(c->dir, "constant/polyMesh");
    std::vector<std::string> tk;
    std::string err;
    auto code_of = [&]() { return err.find("not supported") != std::string::npos ? FY_ERR_UNSUPPORTED : FY_ERR_INVALID; };      // (an unsupported file format falls back to blockMeshDict)
    auto list_of = [&](const char* name) -> int { return fy::foam_list_file_tokens(join(base, name), &tk, &err) ? FY_OK : fail(code_of(), "%s", err.c_str()); };
    // ---- points: N (x y z) ...
    std::vector<double> pts;
    if (!fy::foam_numeric_list_file(join(base, "points"), &pts, &err)) return fail(code_of(), "%s", err.c_str());
    if (pts.size() < 25 || (pts.size() - 1) % 3 != 0 || (double)((pts.size() - 1) / 3) != pts[0]) return fail(FY_ERR_INVALID, "%s/points: malformed point list", base.c_str());
    pts.erase(pts.begin());
    const size_t npts = pts.size() / 3;
    std::vector<double> ax[3];
    double span = 0.0;
    for (int a = 0; a < 3; ++a) {
        std::vector<double> v(npts);
        for (size_t q = 0; q < npts; ++q) v[q] = pts[3 * q + a];
        std::sort(v.begin(), v.end());
        span = std::max(span, v.back() - v.front());
        ax[a].swap(v);
    }
    for (int a = 0; a < 3; ++a) {
        std::vector<double> u;
        for (double x : ax[a]) if (u.empty() || !(std::fabs(x - u.back()) <= 1e-9 * span)) u.push_back(x);
        ax[a].swap(u);
        if (ax[a].size() < 2) return fail(FY_ERR_INVALID, "%s/points: the mesh is flat along axis %d", base.c_str(), a);
    }
    const size_t np1[3] = {ax[0].size(), ax[1].size(), ax[2].size()};
    if (np1[0] * np1[1] * np1[2] != npts)
        return fail(FY_ERR_UNSUPPORTED, "%s/points: %zu points on %zu x %zu x %zu distinct coordinates -- not a rectilinear lattice (only axis-aligned boxes of hexahedra are supported)", base.c_str(),
                    npts, np1[0], np1[1], np1[2]);
    const int nn[3] = {(int)np1[0] - 1, (int)np1[1] - 1, (int)np1[2] - 1};
    const size_t ncell = (size_t)nn[0] * nn[1] * nn[2];
    auto index_of = [&](int a, double x) { return (int)(std::lower_bound(ax[a].begin(), ax[a].end(), x - 1e-9 * span) - ax[a].begin()); };
    std::vector<int32_t> pidx(3 * npts);
    for (size_t q = 0; q < npts; ++q) for (int a = 0; a < 3; ++a) pidx[3 * q + a] = index_of(a, pts[3 * q + a]);
    { std::vector<double>().swap(pts); }
    // ---- faces: N 4(a b c d) ...
    std::vector<int32_t> fl;
    if (!fy::foam_label_list_file(join(base, "faces"), &fl, &err)) return fail(FY_ERR_INVALID, "%s", err.c_str());
    if (fl.empty() || (fl.size() - 1) % 5 != 0 || (size_t)fl[0] != (fl.size() - 1) / 5) return fail(FY_ERR_UNSUPPORTED, "%s/faces: only quadrilateral faces (hexahedral cells) are supported", base.c_str());
    const size_t nfaces = (fl.size() - 1) / 5;
    std::vector<int32_t> fpt(4 * nfaces);
    for (size_t f = 0; f < nfaces; ++f) {
        if (fl[1 + 5 * f] != 4) return fail(FY_ERR_UNSUPPORTED, "%s/faces: only quadrilateral faces (hexahedral cells) are supported", base.c_str());
        for (int m = 0; m < 4; ++m) {
            const int32_t l = fl[2 + 5 * f + m];
            if (l < 0 || (size_t)l >= npts) return fail(FY_ERR_INVALID, "%s/faces: point label out of range", base.c_str());
            fpt[4 * f + m] = l;
        }
    }
    { std::vector<int32_t>().swap(fl); }
    std::vector<int32_t> own, nei;
    if (!fy::foam_label_list_file(join(base, "owner"), &own, &err)) return fail(FY_ERR_INVALID, "%s", err.c_str());
    if (own.empty() || (size_t)own[0] != own.size() - 1 || own.size() - 1 != nfaces) return fail(FY_ERR_INVALID, "%s/owner: %zu entries for %zu faces", base.c_str(), own.size() - 1, nfaces);
    own.erase(own.begin());
    if (!fy::foam_label_list_file(join(base, "neighbour"), &nei, &err)) return fail(FY_ERR_INVALID, "%s", err.c_str());
    if (nei.empty() || (size_t)nei[0] != nei.size() - 1 || nei.size() - 1 > nfaces) return fail(FY_ERR_INVALID, "%s/neighbour: malformed", base.c_str());
    nei.erase(nei.begin());
    // ---- every cell's smallest corner -> its place in the lattice
    std::vector<int32_t> cmin(3 * ncell, INT32_MAX);
    auto touch = [&](int32_t cell, size_t f) -> bool {
        if (cell < 0 || (size_t)cell >= ncell) return false;
        for (int m = 0; m < 4; ++m) for (int a = 0; a < 3; ++a) {
            int32_t& v = cmin[3 * (size_t)cell + a];
            v = std::min(v, pidx[3 * (size_t)fpt[4 * f + m] + a]);
        }
        return true;
    };
    for (size_t f = 0; f < nfaces; ++f) {
        if (!touch(own[f], f) || (f < nei.size() && !touch(nei[f], f)))
            return fail(FY_ERR_UNSUPPORTED, "%s: cell labels beyond %zu = the lattice's cell count (not a box filled with hexahedra)", base.c_str(), ncell);
    }
    c->file_cell.assign(ncell, -1);
    bool identity = true;
    for (size_t q = 0; q < ncell; ++q) {
        const int i = cmin[3 * q], j = cmin[3 * q + 1], k = cmin[3 * q + 2];
        if (i < 0 || i >= nn[0] || j < 0 || j >= nn[1] || k < 0 || k >= nn[2]) return fail(FY_ERR_UNSUPPORTED, "%s: cell %zu does not sit in the lattice", base.c_str(), q);
        const size_t L = (size_t)i + (size_t)nn[0] * ((size_t)j + (size_t)nn[1] * (size_t)k);
        if (c->file_cell[L] != -1) return fail(FY_ERR_UNSUPPORTED, "%s: two cells share the lattice place (%d %d %d)", base.c_str(), i, j, k);
        c->file_cell[L] = (int32_t)q;
        identity = identity && L == q;
    }
    if (identity) c->file_cell.clear();
    // ---- boundary: N ( name { type ...; nFaces n; startFace s; } ... ): every patch's faces lie on sides of the box, every side belongs to one patch
    FY_TRY(list_of("boundary"));
    std::vector<std::pair<std::string, FoamDict> > patches;
    FY_TRY(named_dicts(tk, base + "/boundary", &patches));
    std::vector<size_t> side_faces(6, 0);
    for (int sd = 0; sd < 6; ++sd) c->side_face_src[sd].assign((size_t)nn[(sd / 2 + 1) % 3] * (size_t)nn[(sd / 2 + 2) % 3], -1);
    for (auto& pd : patches) {
        int nf = 0, sf = 0;
        std::string ty;
        pd.second.word("type", &ty);
        if (!pd.second.integer("nFaces", &nf) || !pd.second.integer("startFace", &sf) || nf < 0 || sf < 0 || (size_t)sf + (size_t)nf > nfaces)
            return fail(FY_ERR_INVALID, "%s/boundary: patch '%s' needs nFaces and startFace inside the face list", base.c_str(), pd.first.c_str());
        if (nf == 0) continue;                               // (a patch without faces -- blockMesh's empty `defaultFaces` -- constrains nothing, whatever its type)
        if (ty == "empty" || ty == "cyclic" || ty == "wedge" || ty == "processor")
            return fail(FY_ERR_UNSUPPORTED, "%s/boundary: patch '%s' of type '%s' is not supported (wall / patch / symmetryPlane sides of a 3-D box)", base.c_str(), pd.first.c_str(), ty.c_str());
        for (int q = 0; q < nf; ++q) {
            const size_t f = (size_t)sf + (size_t)q;
            int side = -1;
            for (int a = 0; a < 3 && side < 0; ++a)
                for (int sd = 0; sd < 2 && side < 0; ++sd) {
                    bool all = true;
                    for (int m = 0; m < 4; ++m) all = all && pidx[3 * (size_t)fpt[4 * f + m] + a] == (sd ? nn[a] : 0);
                    if (all) side = 2 * a + sd;
                }
            if (side < 0) return fail(FY_ERR_UNSUPPORTED, "%s/boundary: patch '%s' has a face that is not on a side of the box", base.c_str(), pd.first.c_str());
            if (!c->patch_of_side[side].empty() && c->patch_of_side[side] != pd.first)
                return fail(FY_ERR_UNSUPPORTED, "%s/boundary: side %d of the box is shared by the patches '%s' and '%s' (one boundary condition per side)", base.c_str(), side, c->patch_of_side[side].c_str(), pd.first.c_str());
            c->patch_of_side[side] = pd.first;
            c->class_of_side[side] = ty;
            ++side_faces[(size_t)side];
            {   // the face's place on its side in "U_boundary"'s order (the lower remaining axis fastest), from its smallest corner
                int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX};
                for (int m = 0; m < 4; ++m) for (int a = 0; a < 3; ++a) lo[a] = std::min(lo[a], pidx[3 * (size_t)fpt[4 * f + m] + a]);
                const int d = side / 2;
                const size_t r = d == 0 ? (size_t)lo[1] + (size_t)nn[1] * lo[2] : d == 1 ? (size_t)lo[0] + (size_t)nn[0] * lo[2] : (size_t)lo[0] + (size_t)nn[0] * lo[1];
                if (r < c->side_face_src[side].size()) c->side_face_src[side][r] = q;
            }
        }
        if (nf > 0) c->patch_order.push_back(pd.first);
    }
    for (int sd = 0; sd < 6; ++sd) {
        const int a = sd / 2;
        const size_t want = (size_t)nn[(a + 1) % 3] * (size_t)nn[(a + 2) % 3];
        if (side_faces[(size_t)sd] != want) return fail(FY_ERR_INVALID, "%s/boundary: side %d of the box has %zu of its %zu faces in patches", base.c_str(), sd, side_faces[(size_t)sd], want);
    }
    // ---- the block: cell sizes per axis, cubes or graded
    std::vector<double> h[3];
    for (int a = 0; a < 3; ++a) for (int q = 0; q < nn[a]; ++q) h[a].push_back(ax[a][(size_t)q + 1] - ax[a][(size_t)q]);
    const double dx = (ax[0].back() - ax[0].front()) / nn[0];
    bool cubes = true;
    for (int a = 0; a < 3; ++a) for (double x : h[a]) cubes = cubes && near(x, dx, dx);
    c->desc.nx = nn[0]; c->desc.ny = nn[1]; c->desc.nz = nn[2]; c->desc.dx = dx;
    c->desc.hx = c->desc.hy = c->desc.hz = nullptr;
    if (!cubes) {
        for (int a = 0; a < 3; ++a) c->grading[a] = h[a];
        c->desc.hx = c->grading[0].data(); c->desc.hy = c->grading[1].data(); c->desc.hz = c->grading[2].data();
    }
    for (int a = 0; a < 3; ++a) c->desc.origin[a] = ax[a].front();
    return FY_OK;
}

std::string entry_text(const FoamDict& d, const std::string& indent = "        ") {
    std::string t;
    for (const std::string& k : d.order) {
        const auto* tk = d.tokens(k);
        if (!tk) {                                             // a sub-dictionary (an inlet's function: `uniformValue { type sine; ... }`, `uniformValueCoeffs { ... }`)
            if (const FoamDict* sub = d.subdict(k)) t += indent + k + "\n" + indent + "{\n" + entry_text(*sub, indent + "    ") + indent + "}\n";
            continue;
        }
        bool blob = false;
        for (const std::string& s : *tk) blob = blob || (!s.empty() && s[0] == '\x01');
        if (blob) continue;                                // (a binary list: not text; the types that need a value here take `uniform`)
        t += indent + k;
        for (const std::string& s : *tk) t += " " + s;
        t += ";\n";
    }
    return t;
}

int read_internal(const FoamDict& f, const std::string& path, int ncomp, size_t ncell, std::vector<double>* out, const std::vector<int32_t>* file_cell = nullptr) {
    const auto* t = f.tokens("internalField");
    if (!t || t->empty()) return fail(FY_ERR_INVALID, "%s: no internalField", path.c_str());
    out->assign(ncell * (size_t)ncomp, 0.0);
    if ((*t)[0] == "uniform") {
        double v[3] = {0, 0, 0};
        if (ncomp == 1) { if (t->size() < 2 || !fy::foam_tok_is_number((*t)[1], &v[0])) return fail(FY_ERR_INVALID, "%s: malformed uniform internalField", path.c_str()); }
        else if (!f.vector3("internalField", v)) return fail(FY_ERR_INVALID, "%s: malformed uniform internalField", path.c_str());
        for (size_t c = 0; c < ncell; ++c) for (int q = 0; q < ncomp; ++q) (*out)[c * ncomp + q] = v[q];
        return FY_OK;
    }
    if ((*t)[0] == "nonuniform" && t->size() > 2) {
        std::vector<double> v;
        if (!fy::foam_read_list(*t, 2, ncomp, &v) || v.size() != ncell * (size_t)ncomp)
            return fail(FY_ERR_INVALID, "%s: nonuniform internalField does not hold %zu values", path.c_str(), ncell);
        if (file_cell && !file_cell->empty()) {           // the mesh's cell numbers -> lattice order
            for (size_t L = 0; L < ncell; ++L) for (int q = 0; q < ncomp; ++q) (*out)[L * ncomp + q] = v[(size_t)(*file_cell)[L] * ncomp + q];
        } else {
            out->swap(v);
        }
        return FY_OK;
    }
    return fail(FY_ERR_UNSUPPORTED, "%s: internalField must be 'uniform' or 'nonuniform List<...>'", path.c_str());
}

// boundaryField entries that belong to none of the six sides (a decomposed case's processor patches): kept as text, written back as they are
// A processor patch is written back with a `value` entry in any case: processorFvPatchField's dictionary constructor reads one [OF-6
// processorFvPatchField.C], so reconstructPar would refuse a file without it -- where the file's value was a binary list (not kept as text) or
// absent, `uniform 0` stands in (the patch's values are re-evaluated from the neighbour's cells on the first use)
void keep_extra_patches(const fy_foam_case* c, const FoamDict& bf, int ncomp, std::vector<std::pair<std::string, std::string> >* out) {
    out->clear();
    for (const std::string& name : bf.order) {
        bool side = false;
        for (int s = 0; s < 6; ++s) side = side || c->patch_of_side[s] == name;
        const FoamDict* pd = bf.subdict(name);
        if (side || !pd) continue;
        std::string text = entry_text(*pd);
        if (text.find("        value ") == std::string::npos) text += ncomp == 3 ? "        value uniform (0 0 0);\n" : "        value uniform 0;\n";
        out->emplace_back(name, text);
    }
}
// `value nonuniform List<...> 0()`: what decomposePar writes for a patch that has no face on this processor (every z side of the block on the ranks
// that do not touch it): the patch's value is then nobody's business here
bool empty_patch_value(const std::vector<std::string>* vt, int ncomp) {
    if (!vt || vt->size() < 3 || (*vt)[0] != "nonuniform") return false;
    std::vector<double> v;
    return fy::foam_read_list(*vt, 2, ncomp, &v) && v.empty();
}

// `value uniform <x>` / `value uniform (x y z)` -> v
bool uniform_scalar(const FoamDict& pd, double* v) {
    const auto* vt = pd.tokens("value");
    return vt && vt->size() >= 2 && (*vt)[0] == "uniform" && fy::foam_tok_is_number((*vt)[1], v);
}
bool uniform_vector(const FoamDict& pd, double* v) {
    const auto* vt = pd.tokens("value");
    return vt && !vt->empty() && (*vt)[0] == "uniform" && pd.vector3("value", v);
}

// ---- inlets: OpenFOAM-6's Function1 entries [Constant, Table, Sine, Square, as recalled -- unpinned] -> the terms of an inlet (include/foamyade_hip.h "Inlets")
using InletTerm = fy_foam_case::InletTerm;
bool tok_num(const std::vector<std::string>& t, size_t i, double* v) { return i < t.size() && fy::foam_tok_is_number(t[i], v); }
// `(x y z)` at token i
bool tok_vec(const std::vector<std::string>& t, size_t i, double* v) {
    return i + 4 < t.size() && t[i] == "(" && tok_num(t, i + 1, v) && tok_num(t, i + 2, v + 1) && tok_num(t, i + 3, v + 2) && t[i + 4] == ")";
}
// the rows `(t v)` / `(t (x y z))` of a table from token i on ("(" or a count and "(")
bool read_table_rows(const std::vector<std::string>& t, size_t i, int ncomp, std::vector<double>* times, std::vector<double>* vals) {
    double x;
    if (tok_num(t, i, &x)) ++i;
    if (i >= t.size() || t[i] != "(") return false;
    for (++i; i < t.size() && t[i] != ")";) {
        if (t[i] != "(" || !tok_num(t, i + 1, &x)) return false;
        times->push_back(x);
        i += 2;
        double v[3];
        if (ncomp == 1) { if (!tok_num(t, i, v)) return false; vals->push_back(v[0]); i += 1; }
        else { if (!tok_vec(t, i, v)) return false; vals->insert(vals->end(), v, v + 3); i += 5; }
        if (i >= t.size() || t[i] != ")") return false;
        ++i;
    }
    return !times->empty() && i < t.size();
}
// entry `key` of patch dictionary pd as a Function1 of scalars (ncomp 1: a flow rate, every term takes the flow-rate shape) or of vectors (ncomp 3) -> terms.
// Written `key <number | (x y z)>;`, `key constant <value>;`, `key table ((t v) ...);`, `key sine | square;` with `<key>Coeffs { ... }`, or `key { type ...; ... }`
int read_function1(const FoamDict& pd, const std::string& key, int ncomp, const std::string& w, std::vector<InletTerm>* out) {
    const FoamDict* sub = pd.subdict(key);
    const std::vector<std::string>* tk = sub ? nullptr : pd.tokens(key);
    if (!sub && (!tk || tk->empty())) return fail(FY_ERR_UNSUPPORTED, "%s: no '%s' entry", w.c_str(), key.c_str());
    std::string type;
    const FoamDict* co = nullptr;
    size_t at = 0;
    if (sub) {
        if (!sub->word("type", &type)) return fail(FY_ERR_UNSUPPORTED, "%s: '%s' is a dictionary without a type", w.c_str(), key.c_str());
        co = sub->subdict(type + "Coeffs") ? sub->subdict(type + "Coeffs") : sub;
    } else {
        double v;
        if ((*tk)[0] == "(" || fy::foam_tok_is_number((*tk)[0], &v)) type = "constant";
        else { type = (*tk)[0]; at = 1; co = pd.subdict(key + "Coeffs"); }
    }
    const char* accepted = "accepted: constant, table (outOfBounds clamp | repeat), sine, square";
    auto shaped = [&](InletTerm& T, const double* vec) {          // a scalar function's terms carry the flow-rate shape, a vector function's a vector
        if (ncomp == 1) T.shape_kind = FY_SHAPE_FLOW_RATE;
        else { T.shape_kind = FY_SHAPE_UNIFORM; T.shape.assign(vec, vec + 3); }
    };
    if (type == "constant" || type == "uniform") {
        const std::vector<std::string>* vt = sub ? co->tokens("value") : tk;
        InletTerm T;
        T.f.kind = FY_TIME_CONSTANT; T.f.value = 1.0;
        double v[3] = {0, 0, 0};
        if (!vt || (ncomp == 1 ? !tok_num(*vt, sub ? 0 : at, &T.f.value) : !tok_vec(*vt, sub ? 0 : at, v)))
            return fail(FY_ERR_UNSUPPORTED, "%s: %s constant needs %s", w.c_str(), key.c_str(), ncomp == 1 ? "a number" : "a vector (x y z)");
        shaped(T, v);
        out->push_back(T);
        return FY_OK;
    }
    if (type == "table") {
        const std::vector<std::string>* vt = sub ? co->tokens("values") : tk;
        std::vector<double> times, vals;
        if (!vt || !read_table_rows(*vt, sub ? 0 : at, ncomp, &times, &vals))
            return fail(FY_ERR_UNSUPPORTED, "%s: %s table needs rows %s", w.c_str(), key.c_str(), ncomp == 1 ? "((t v) ...)" : "((t (x y z)) ...)");
        int oob = FY_TIME_CLAMP;
        std::string word;
        if (co && co->word("outOfBounds", &word)) {
            if (word == "repeat") oob = FY_TIME_REPEAT;
            else if (word != "clamp") return fail(FY_ERR_UNSUPPORTED, "%s: %s table: outOfBounds '%s' is not supported (clamp, repeat)", w.c_str(), key.c_str(), word.c_str());
        }
        if (co && co->word("interpolationScheme", &word) && word != "linear") return fail(FY_ERR_UNSUPPORTED, "%s: %s table: interpolationScheme '%s' is not supported (linear)", w.c_str(), key.c_str(), word.c_str());
        if (co && co->has("file")) return fail(FY_ERR_UNSUPPORTED, "%s: %s table: a table read from a file (tableFile) is not supported", w.c_str(), key.c_str());
        for (int a = 0; a < ncomp; ++a) {
            InletTerm T;
            T.f.kind = FY_TIME_TABLE; T.f.out_of_bounds = oob; T.f.n_points = (int32_t)times.size();
            for (size_t q = 0; q < times.size(); ++q) { T.pts.push_back(times[q]); T.pts.push_back(vals[q * (size_t)ncomp + a]); }
            const double e[3] = {a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0};
            shaped(T, e);
            out->push_back(T);
        }
        return FY_OK;
    }
    if (type == "sine" || type == "square") {
        if (!co) return fail(FY_ERR_UNSUPPORTED, "%s: %s %s needs its coefficients (%sCoeffs { amplitude; frequency; scale; level; }, or a dictionary with `type %s`)", w.c_str(), key.c_str(), type.c_str(), key.c_str(), type.c_str());
        InletTerm W, L;
        W.f.kind = type == "sine" ? FY_TIME_SINE : FY_TIME_SQUARE;
        W.f.amplitude = 1.0; W.f.mark_space = 1.0;
        const auto* at_ = co->tokens("amplitude");
        if (at_) for (const std::string& x : *at_) if (x == "(" || x == "table" || x == "sine" || x == "square") return fail(FY_ERR_UNSUPPORTED, "%s: %s %s: amplitude must be a number (`amplitude 2;` or `amplitude constant 2;`)", w.c_str(), key.c_str(), type.c_str());
        co->scalar("amplitude", &W.f.amplitude);
        if (!co->scalar("frequency", &W.f.frequency)) return fail(FY_ERR_UNSUPPORTED, "%s: %s %s needs a frequency", w.c_str(), key.c_str(), type.c_str());
        co->scalar("start", &W.f.t0); co->scalar("t0", &W.f.t0);
        co->scalar("markSpace", &W.f.mark_space);
        L.f.kind = FY_TIME_CONSTANT; L.f.value = 1.0;
        double sc[3] = {0, 0, 0}, lv[3] = {0, 0, 0};
        if (ncomp == 1) {
            if (!co->scalar("scale", &sc[0]) || !co->scalar("level", &lv[0])) return fail(FY_ERR_UNSUPPORTED, "%s: %s %s needs scale and level (numbers)", w.c_str(), key.c_str(), type.c_str());
            W.f.amplitude *= sc[0]; L.f.value = lv[0];
        } else if (!co->vector3("scale", sc) || !co->vector3("level", lv)) return fail(FY_ERR_UNSUPPORTED, "%s: %s %s needs scale and level (vectors)", w.c_str(), key.c_str(), type.c_str());
        shaped(W, sc); shaped(L, lv);
        out->push_back(W); out->push_back(L);
        return FY_OK;
    }
    return fail(FY_ERR_UNSUPPORTED, "%s: %s of type '%s' is not supported (%s; not tableFile, polynomial, coded)", w.c_str(), key.c_str(), type.c_str(), accepted);
}
// the sides of a block that patch `name` covers
int sides_of_patch(const fy_foam_case* c, const std::string& name) { int n = 0; for (int s = 0; s < 6; ++s) n += c->patch_of_side[s] == name; return n; }
size_t side_size(const fy_foam_case* c, int side) {
    const int nn[3] = {c->desc.nx, c->desc.ny, c->desc.nz};
    return (size_t)nn[(side / 2 + 1) % 3] * (size_t)nn[(side / 2 + 2) % 3];
}
// a velocity patch whose entry makes it an inlet: ty = fixedValue with a non-empty `value nonuniform List<vector>`, uniformFixedValue, flowRateInletVelocity
int inlet_condition(fy_foam_case* c, const std::string& path, size_t pa, const std::string& name, const FoamDict& pd, const std::string& ty) {
    const std::string w = path + ": patch '" + name + "'";
    if (!c->general && c->proc_count > 0) return fail(FY_ERR_UNSUPPORTED, "%s: %s in a decomposed case is not supported (inlets run on one domain)", w.c_str(), ty.c_str());
    if (c->general) for (int32_t nb : c->g_patch_neighbour) if (nb >= 0) return fail(FY_ERR_UNSUPPORTED, "%s: %s in a case with cyclic patches is not supported", w.c_str(), ty.c_str());
    fy_foam_case::Inlet in;
    in.patch = (int)pa;
    if (ty == "fixedValue") {
        std::vector<double> v;
        if (!fy::foam_read_list(*pd.tokens("value"), 2, 3, &v)) return fail(FY_ERR_INVALID, "%s: malformed 'value nonuniform List<vector>'", w.c_str());
        InletTerm T;
        T.f.kind = FY_TIME_CONSTANT; T.f.value = 1.0; T.shape_kind = FY_SHAPE_PER_FACE;
        if (c->general) {
            if (v.size() != 3 * (size_t)c->g_patch_size[pa]) return fail(FY_ERR_INVALID, "%s: the nonuniform value holds %zu vectors, the patch has %d faces", w.c_str(), v.size() / 3, (int)c->g_patch_size[pa]);
            T.shape = v;
        } else {
            const std::vector<int32_t>& src = c->side_face_src[pa];
            if (src.empty())
                return fail(FY_ERR_UNSUPPORTED, "%s: a nonuniform fixedValue needs constant/polyMesh: with system/blockMeshDict alone the order of blockMesh's boundary faces cannot be "
                                                "verified here (run blockMesh, or give 'value uniform (x y z)')", w.c_str());
            size_t total = 0;
            for (int s = 0; s < 6; ++s) if (c->patch_of_side[s] == name) total += side_size(c, s);
            if (v.size() != 3 * total) return fail(FY_ERR_INVALID, "%s: the nonuniform value holds %zu vectors, the patch has %zu faces", w.c_str(), v.size() / 3, total);
            T.shape.resize(3 * src.size());
            for (size_t r = 0; r < src.size(); ++r) {
                if (src[r] < 0 || (size_t)src[r] >= total) return fail(FY_ERR_INVALID, "%s: a face of side %zu has no place in the patch's face list", w.c_str(), pa);
                for (int q = 0; q < 3; ++q) T.shape[3 * r + q] = v[3 * (size_t)src[r] + q];
            }
        }
        in.terms.push_back(T);
    } else if (ty == "uniformFixedValue") {
        FY_TRY(read_function1(pd, "uniformValue", 3, w, &in.terms));
    } else {
        bool ex = false;
        if (pd.has("massFlowRate") || pd.has("rho") || pd.has("rhoInlet")) return fail(FY_ERR_UNSUPPORTED, "%s: flowRateInletVelocity with massFlowRate / rho is not supported (volumetricFlowRate)", w.c_str());
        if (pd.boolean("extrapolateProfile", &ex) && ex) return fail(FY_ERR_UNSUPPORTED, "%s: flowRateInletVelocity with extrapolateProfile is not supported", w.c_str());
        if (!c->general && sides_of_patch(c, name) > 1) return fail(FY_ERR_UNSUPPORTED, "%s: flowRateInletVelocity on a patch that covers several sides of the block is not supported", w.c_str());
        FY_TRY(read_function1(pd, "volumetricFlowRate", 1, w, &in.terms));
    }
    c->inlets.push_back(in);
    return FY_OK;
}
// the case's inlets as the solvers take them (pointers into the case object)
void inlets_desc(const fy_foam_case* c, fy_inlets_desc* out) {
    c->inlet_descs.assign(c->inlets.size(), fy_inlet_desc{});
    for (size_t q = 0; q < c->inlets.size(); ++q) {
        const fy_foam_case::Inlet& in = c->inlets[q];
        fy_inlet_desc& d = c->inlet_descs[q];
        d.patch = in.patch; d.n_terms = (int32_t)in.terms.size();
        for (size_t m = 0; m < in.terms.size() && m < 3; ++m) {
            d.terms[m].f = in.terms[m].f;
            if (in.terms[m].f.kind == FY_TIME_TABLE) d.terms[m].f.points = in.terms[m].pts.data();
            d.terms[m].shape_kind = in.terms[m].shape_kind;
            d.terms[m].shape = in.terms[m].shape.empty() ? nullptr : in.terms[m].shape.data();
        }
    }
    *out = fy_inlets_desc{};
    out->start_time = c->start_time; out->n = (int32_t)c->inlets.size(); out->inlets = c->inlets.empty() ? nullptr : c->inlet_descs.data();
}

// whether the case has field F: U and p always, nut with a turbulence model, k with kEqn / kEpsilon, epsilon with kEpsilon, alpha with pimpleFoamYade
bool has_field(const fy_foam_case* c, int F) {
    const int tm = c->desc.turbulence_model;
    switch (F) {
        case F_NUT: return tm != FY_TURBULENCE_LAMINAR;
        case F_K: return tm == FY_TURBULENCE_KEQN || tm == FY_TURBULENCE_KEPSILON;
        case F_EPS: return tm == FY_TURBULENCE_KEPSILON;
        case F_ALPHA: return c->solver == FY_SOLVER_PIMPLE;
        case F_T: return c->desc.thermal.on != 0;
        default: return true;
    }
}

std::string field_name(const fy_foam_case* c, int F) {
    static const char* const group[] = {"", "", "nut.", "k.", "epsilon.", "alpha."};
    if (F == F_T) return c->phase.empty() ? std::string("T") : "T." + c->phase;       // (named with the velocity's group, like the turbulence fields)
    return F == F_U ? c->u_name : F == F_P ? std::string("p") : group[F] + c->phase;
}

// the patch list a field's conditions are indexed by: the six sides of a block (XMIN .. ZMAX; one patch may cover several), every patch of a general mesh
std::vector<std::string> field_patches(const fy_foam_case* c) {
    return c->general ? c->g_patch_name : std::vector<std::string>(c->patch_of_side, c->patch_of_side + 6);
}

// one patch's entry of field F (type ty): its FY_BC_* code and value, or the refusal.  The two kinds of case take different sets of types:
//   both      U: fixedValue (uniform, or one vector per face: an inlet), uniformFixedValue and flowRateInletVelocity (volumetricFlowRate) with a Function1 of the kinds
//             read_function1 takes (inlets: DESIGN.md section 3), noSlip, zeroGradient, symmetryPlane / symmetry / slip.  p: zeroGradient, symmetryPlane / symmetry, fixedValue (uniform).
//             nut: zeroGradient, symmetryPlane / symmetry, fixedValue (uniform), calculated and nutkWallFunction with kEqn / kEpsilon.
//             k: zeroGradient, symmetryPlane / symmetry, kqRWallFunction, fixedValue (uniform).  epsilon: those of k but kqRWallFunction, epsilonWallFunction
//   a block   also takes `value nonuniform List<...> 0()` for a fixedValue U or p (decomposePar's value of a patch without a face on the processor), and
//             fixedFluxPressure with either solver; a wall function's kappa / E are taken as read, the last side's winning
//   a general mesh  also takes cyclic entries (folded into internal faces: their code is not used), fixedFluxPressure with pimpleFoamYade only, and nut
//             calculated without a k equation as a fixed value; it checks an entry's type against a constraint patch's (U, p) and a wall function's patch
//             class (nut, epsilon), defaults kappa / E per patch and refuses patches that differ, and needs nutkWallFunction under an epsilonWallFunction
int patch_condition(fy_foam_case* c, int F, const std::string& path, size_t pa, const std::string& name, const FoamDict& pd, const std::string& ty, int32_t* bc, double* val) {
    const bool g = c->general;
    const char* pn = name.c_str();
    const std::string cls = g ? c->g_patch_class[pa] : std::string();
    const bool k_model = has_field(c, F_K);
    const bool zero_grad = ty == "zeroGradient" || ty == "symmetryPlane" || ty == "symmetry" || (g && ty == "cyclic");      // (a scalar on a symmetry plane: the cell value)
    // open boundaries, general meshes only (DESIGN.md section 3 "Open boundaries"): U inletOutlet | pressureInletOutletVelocity, k and
    // epsilon inletOutlet [OF-6 inletOutletFvPatchField, pressureInletOutletVelocityFvPatchVectorField, as recalled].  `phi`, if given, must be the case's flux;
    // `value` is optional and not used.  A block keeps refusing the words with its own lists (below)
    if (g && ((ty == "inletOutlet" && (F == F_U || F == F_K || F == F_EPS)) || (ty == "pressureInletOutletVelocity" && F == F_U))) {
        if (cls == "wall" || cls == "symmetryPlane" || cls == "symmetry" || cls == "cyclic")
            return fail(FY_ERR_UNSUPPORTED, "%s: patch '%s': %s on a %s patch is not supported (an open boundary sits on a patch of type patch in constant/polyMesh/boundary)", path.c_str(), pn,
                        ty.c_str(), cls.c_str());
        std::string flux;
        if (pd.word("phi", &flux) && flux != "phi" && !(c->solver == FY_SOLVER_PIMPLE && !c->phase.empty() && flux == "phi." + c->phase))
            return fail(FY_ERR_UNSUPPORTED, "%s: patch '%s': %s with phi %s is not supported (the case's flux: phi%s)", path.c_str(), pn, ty.c_str(), flux.c_str(),
                        c->solver == FY_SOLVER_PIMPLE && !c->phase.empty() ? (", phi." + c->phase).c_str() : "");
        if (ty == "pressureInletOutletVelocity") {
            if (pd.has("tangentialVelocity")) return fail(FY_ERR_UNSUPPORTED, "%s: patch '%s': pressureInletOutletVelocity with tangentialVelocity is not supported", path.c_str(), pn);
            *bc = FY_BC_U_PRESSURE_INLET_OUTLET;
            return FY_OK;
        }
        const auto* iv = pd.tokens("inletValue");
        const bool ok = iv && !iv->empty() && (*iv)[0] == "uniform" && (F == F_U ? tok_vec(*iv, 1, val) : tok_num(*iv, 1, val));
        if (!ok) return fail(FY_ERR_UNSUPPORTED, "%s: patch '%s': inletOutlet needs 'inletValue uniform %s'", path.c_str(), pn, F == F_U ? "(x y z)" : F == F_K ? "<k>" : "<epsilon>");
        *bc = F == F_U ? FY_BC_U_INLET_OUTLET : FY_BC_NUT_INLET_OUTLET;
        return FY_OK;
    }
    // [OF-6 fvPatchField::New]: a field's entry on a constraint patch must carry the patch's own type
    if (g && (F == F_U || F == F_P) && (cls == "symmetryPlane" || cls == "symmetry" || cls == "cyclic") && c->g_patch_size[pa] > 0 && ty != cls)
        return fail(FY_ERR_INVALID, "%s: patch '%s' is a %s patch (constant/polyMesh/boundary): its entry must be of that type, not '%s'", path.c_str(), pn, cls.c_str(), ty.c_str());
    // [OF-6 nutWallFunctionFvPatchScalarField::checkType]: a wall function sits on a wall patch
    if (g && (F == F_NUT || F == F_EPS) && ty.find("WallFunction") != std::string::npos && cls != "wall")
        return fail(FY_ERR_UNSUPPORTED, "%s: patch '%s': %s is a wall function, but the patch is of type '%s' (constant/polyMesh/boundary), not wall", path.c_str(), pn, ty.c_str(), cls.c_str());
    if (F == F_T) {
        if (ty == "fixedValue") {
            *bc = FY_BC_T_FIXED_VALUE;
            if (!uniform_scalar(pd, val)) return fail(FY_ERR_UNSUPPORTED, "%s: patch '%s': fixedValue needs 'value uniform <T>'", path.c_str(), pn);
            return FY_OK;
        }
        if (ty == "zeroGradient" || ty == "symmetryPlane" || ty == "symmetry") { *bc = FY_BC_T_ZERO_GRADIENT; return FY_OK; }
        return fail(FY_ERR_UNSUPPORTED, "%s: patch '%s': temperature boundary type '%s' is not supported (zeroGradient, fixedValue)", path.c_str(), pn, ty.c_str());
    }
    switch (F) {
        case F_U:
            if (ty == "uniformFixedValue" || ty == "flowRateInletVelocity") { *bc = FY_BC_U_FIXED_VALUE; return inlet_condition(c, path, pa, name, pd, ty); }
            if (ty == "fixedValue") {
                *bc = FY_BC_U_FIXED_VALUE;
                const auto* vt = pd.tokens("value");
                if (vt && vt->size() > 2 && (*vt)[0] == "nonuniform" && !empty_patch_value(vt, 3)) return inlet_condition(c, path, pa, name, pd, ty);      // one vector per face
                if ((g || !empty_patch_value(pd.tokens("value"), 3)) && !uniform_vector(pd, val))
                    return fail(FY_ERR_UNSUPPORTED, "%s: patch '%s': fixedValue needs 'value uniform (x y z)' or 'value nonuniform List<vector> N(...)'", path.c_str(), pn);
                return FY_OK;
            }
            if (ty == "noSlip") { *bc = FY_BC_U_FIXED_VALUE; return FY_OK; }
            if (ty == "zeroGradient" || (g && ty == "cyclic")) { *bc = FY_BC_U_ZERO_GRADIENT; return FY_OK; }
            if (ty == "symmetryPlane" || ty == "symmetry" || ty == "slip") { *bc = FY_BC_U_SLIP; return FY_OK; }      // (one and the same on a planar patch or face)
            break;
        case F_P:
            if (ty == "fixedValue") {
                *bc = FY_BC_P_FIXED_VALUE;
                if ((g || !empty_patch_value(pd.tokens("value"), 1)) && !uniform_scalar(pd, val))
                    return fail(FY_ERR_UNSUPPORTED, "%s: patch '%s': fixedValue needs 'value uniform <p>'", path.c_str(), pn);
                return FY_OK;
            }
            if (ty == "fixedFluxPressure" && (!g || c->solver == FY_SOLVER_PIMPLE)) { *bc = FY_BC_P_FIXED_FLUX; return FY_OK; }
            if (zero_grad) { *bc = FY_BC_P_ZERO_GRADIENT; return FY_OK; }
            break;
        case F_NUT:
            if (ty == "nutkWallFunction" && (k_model || g)) {
                if (!k_model) return fail(FY_ERR_UNSUPPORTED, "%s: patch '%s': nutkWallFunction needs a model with a k equation (kEqn, kEpsilon)", path.c_str(), pn);
                // [OF-6 nutkWallFunctionFvPatchScalarField]: Cmu / kappa / E per patch (defaults 0.09, 0.41, 9.8); one set serves the case here
                *bc = FY_BC_WALL_FUNCTION;
                uniform_scalar(pd, val);
                double cmu = c->desc.ras_cmu, kap = g ? 0.41 : c->desc.wf_kappa, E = g ? 9.8 : c->desc.wf_E;
                pd.scalar("kappa", &kap); pd.scalar("E", &E);
                if (pd.scalar("Cmu", &cmu) && cmu != c->desc.ras_cmu) return fail(FY_ERR_UNSUPPORTED, "%s: patch '%s': a wall-function Cmu other than the model's is not supported", path.c_str(), pn);
                for (size_t q = pa; g && q-- > 0;)                  // the last wall-function patch before this one
                    if (c->bcs[F_NUT].bc[q] == FY_BC_WALL_FUNCTION) {
                        if (kap != c->desc.wf_kappa || E != c->desc.wf_E)
                            return fail(FY_ERR_UNSUPPORTED, "%s: patches '%s' and '%s' give nutkWallFunction different kappa / E: one set serves the case", path.c_str(), c->g_patch_name[q].c_str(), pn);
                        break;
                    }
                c->desc.wf_kappa = kap; c->desc.wf_E = E;
                return FY_OK;
            }
            if (ty == "calculated" && k_model) { *bc = FY_BC_NUT_CALCULATED; uniform_scalar(pd, val); return FY_OK; }      // the file's value until the first correctNut(), the model's expression afterwards
            if (ty == "fixedValue" || (g && ty == "calculated")) {           // (calculated keeps its value: what fixedValue does here)
                *bc = FY_BC_NUT_FIXED_VALUE;
                if (!uniform_scalar(pd, val)) return fail(FY_ERR_UNSUPPORTED, "%s: patch '%s': %s needs 'value uniform <nut>'", path.c_str(), pn, ty.c_str());
                return FY_OK;
            }
            if (zero_grad) { *bc = FY_BC_NUT_ZERO_GRADIENT; return FY_OK; }
            break;
        case F_K:
        case F_EPS:
            if (ty == "fixedValue") {
                *bc = FY_BC_NUT_FIXED_VALUE;
                if (!uniform_scalar(pd, val)) return fail(FY_ERR_UNSUPPORTED, "%s: patch '%s': fixedValue needs 'value uniform <%s>'", path.c_str(), pn, F == F_K ? "k" : "epsilon");
                return FY_OK;
            }
            if (zero_grad || (F == F_K && ty == "kqRWallFunction")) { *bc = FY_BC_NUT_ZERO_GRADIENT; return FY_OK; }
            if (F == F_EPS && ty == "epsilonWallFunction") {
                // [OF-6 epsilonWallFunctionFvPatchScalarField::calculate: nutWallFunctionFvPatchScalarField::nutw(turbModel, patchi)]: kappa and E are the patch's nut wall function's
                if (g && c->bcs[F_NUT].bc[pa] != FY_BC_WALL_FUNCTION)
                    return fail(FY_ERR_UNSUPPORTED, "%s: patch '%s': epsilonWallFunction takes its constants from the patch's nut wall function, and nut.%s is not nutkWallFunction there", path.c_str(), pn, c->phase.c_str());
                *bc = FY_BC_WALL_FUNCTION;
                return FY_OK;
            }
            break;
    }
    static const char* const what[] = {"velocity", "pressure", "nut", "k", "epsilon"};
    // (the velocity lists name the types of a plain patch; an inlet's -- uniformFixedValue, flowRateInletVelocity -- are in INTEGRATION.md section 6)
    static const char* const block_types[] = {"fixedValue, noSlip, zeroGradient, symmetryPlane, symmetry, slip", "zeroGradient, fixedValue, fixedFluxPressure",
                                              "zeroGradient, fixedValue; calculated / nutkWallFunction with kEqn / kEpsilon", "zeroGradient, kqRWallFunction, fixedValue",
                                              "zeroGradient, fixedValue, epsilonWallFunction"};
    static const char* const general_types[] = {"fixedValue, noSlip, zeroGradient, symmetryPlane, symmetry, slip",
                                                "zeroGradient, symmetryPlane, symmetry, fixedValue; fixedFluxPressure with pimpleFoamYade",
                                                "zeroGradient, symmetryPlane, symmetry, cyclic, fixedValue, calculated; nutkWallFunction with kEqn / kEpsilon",
                                                "zeroGradient, kqRWallFunction, symmetryPlane, symmetry, cyclic, fixedValue",
                                                "zeroGradient, symmetryPlane, symmetry, cyclic, fixedValue, epsilonWallFunction"};
    return fail(FY_ERR_UNSUPPORTED, "%s: patch '%s': %s boundary type '%s' is not supported%s (%s)", path.c_str(), pn, what[F], ty.c_str(), g ? " on a general mesh" : "",
                (g ? general_types : block_types)[F]);
}

// <startTime>/<field F> of either kind of case [OF-6: U, p MUST_READ; nut_ of eddyViscosity, k_ of kEqn / kEpsilon, epsilon_ of kEpsilon MUST_READ, named
// with the velocity's group]: internalField uniform or nonuniform (-> *internal, a block's in lattice order; its first value -> *initial), and a typed
// boundaryField entry for every patch of the case's list -> c->bcs[F]
int read_field(fy_foam_case* c, int F, std::vector<double>* internal, double* initial = nullptr) {
    const int ncomp = F == F_U ? 3 : 1;
    const std::string path = join(c->fdir, c->start_name + "/" + field_name(c, F));
    FoamDict f;
    FY_TRY(need_file(path, &f));
    FY_TRY(read_internal(f, path, ncomp, c->fcells, internal, c->general ? nullptr : &c->file_cell));
    if (initial) *initial = internal->empty() ? 0.0 : (*internal)[0];
    const FoamDict* bf = f.subdict("boundaryField");
    if (!bf) return fail(FY_ERR_INVALID, "%s: no boundaryField", path.c_str());
    PatchField& r = c->bcs[F];
    if (!c->general) keep_extra_patches(c, *bf, ncomp, &r.extra);
    const std::vector<std::string> names = field_patches(c);
    r.bc.assign(names.size(), 0); r.val.assign(names.size() * ncomp, 0.0); r.text.assign(names.size(), std::string());
    for (size_t pa = 0; pa < names.size(); ++pa) {
        const FoamDict* pd = bf->subdict(names[pa]);
        std::string ty;
        if (!pd || !pd->word("type", &ty)) return fail(FY_ERR_INVALID, "%s: boundaryField has no (typed) entry for patch '%s'", path.c_str(), names[pa].c_str());
        r.text[pa] = entry_text(*pd);
        FY_TRY(patch_condition(c, F, path, pa, names[pa], *pd, ty, &r.bc[pa], &r.val[(size_t)ncomp * pa]));
        if ((F == F_K || F == F_EPS) && r.bc[pa] == FY_BC_NUT_INLET_OUTLET && !pd->has("value")) {      // a written time directory carries a value: the inlet value
            char buf[96];
            std::snprintf(buf, sizeof(buf), "        value uniform %.17g;\n", r.val[pa]);
            r.text[pa] += buf;
        }
    }
    return FY_OK;
}

// a block's field files, the six sides' conditions then copied into fy_case_desc
int read_fields(fy_foam_case* c) {
    FY_TRY(read_field(c, F_U, &c->U0));
    FY_TRY(read_field(c, F_P, &c->p0));
    if (has_field(c, F_NUT)) FY_TRY(read_field(c, F_NUT, &c->nut0, &c->desc.nut_initial));
    if (has_field(c, F_K)) FY_TRY(read_field(c, F_K, &c->k0, &c->desc.k_initial));
    if (has_field(c, F_EPS)) FY_TRY(read_field(c, F_EPS, &c->eps0, &c->desc.eps_initial));
    if (has_field(c, F_T)) {
        const std::string path = join(c->fdir, c->start_name + "/" + field_name(c, F_T));
        if (!file_exists(path))
            return fail(FY_ERR_UNSUPPORTED, "%s: no such file, but constant/couplingProperties has heatTransfer active: the temperature field of the start time is needed "
                                            "(volScalarField, internalField uniform | nonuniform, patches zeroGradient | fixedValue)", path.c_str());
        FY_TRY(read_field(c, F_T, &c->T0, &c->desc.thermal.T_initial));
        std::copy(c->bcs[F_T].bc.begin(), c->bcs[F_T].bc.end(), c->desc.thermal.T_bc);
        std::copy(c->bcs[F_T].val.begin(), c->bcs[F_T].val.end(), c->desc.thermal.T_value);
    }
    fy_case_desc& d = c->desc;
    const struct { int F; int32_t* bc; double* val; } to[] = {{F_U, d.u_bc, &d.u_value[0][0]}, {F_P, d.p_bc, d.p_value}, {F_NUT, d.nut_bc, d.nut_value},
                                                             {F_K, d.k_bc, d.k_value}, {F_EPS, d.eps_bc, d.eps_value}};
    for (const auto& t : to) {
        if (!has_field(c, t.F)) continue;
        std::copy(c->bcs[t.F].bc.begin(), c->bcs[t.F].bc.end(), t.bc);
        std::copy(c->bcs[t.F].val.begin(), c->bcs[t.F].val.end(), t.val);
    }
    return FY_OK;
}

// a general mesh's field files: fy_foam_case_ldu_desc hands out the records (epsilon before k: an epsilonWallFunction looks at nut's patch)
int read_general_fields(fy_foam_case* c) {
    FY_TRY(read_field(c, F_U, &c->U0));
    FY_TRY(read_field(c, F_P, &c->p0));
    if (has_field(c, F_NUT)) FY_TRY(read_field(c, F_NUT, &c->nut0, &c->desc.nut_initial));
    if (has_field(c, F_EPS)) FY_TRY(read_field(c, F_EPS, &c->eps0, &c->desc.eps_initial));
    if (has_field(c, F_K)) FY_TRY(read_field(c, F_K, &c->k0, &c->desc.k_initial));
    return FY_OK;
}

// constant/polyMesh of ANY mesh, kept in OpenFOAM's own addressing for fy_ldu_solver [OF-6 polyMesh: points, faces (n(p0 .. pn-1) each), owner,
// neighbour (internal faces first), boundary].  The cell count is not stored in the files: it is the largest owner + 1 [OF-6 polyMesh::initMesh]
int read_general_mesh(fy_foam_case* c) {
    const std::string base = join(c->dir, "constant/polyMesh");
    std::string err;
    std::vector<double> pts;
    if (!fy::foam_numeric_list_file(join(base, "points"), &pts, &err)) return fail(err.find("not supported") != std::string::npos ? FY_ERR_UNSUPPORTED : FY_ERR_INVALID, "%s", err.c_str());
    if (pts.size() < 13 || (pts.size() - 1) % 3 != 0 || (double)((pts.size() - 1) / 3) != pts[0]) return fail(FY_ERR_INVALID, "%s/points: malformed point list", base.c_str());
    c->g_points.assign(pts.begin() + 1, pts.end());
    { std::vector<double>().swap(pts); }
    const size_t npts = c->g_points.size() / 3;
    std::vector<int32_t> fl;
    if (!fy::foam_label_list_file(join(base, "faces"), &fl, &err)) return fail(FY_ERR_INVALID, "%s", err.c_str());
    if (fl.size() < 2 || fl[0] < 4) return fail(FY_ERR_INVALID, "%s/faces: malformed face list", base.c_str());
    const size_t nfaces = (size_t)fl[0];
    c->g_face_off.assign(1, 0);
    c->g_face_off.reserve(nfaces + 1);
    c->g_face_pts.reserve(fl.size());
    size_t q = 1;
    for (size_t f = 0; f < nfaces; ++f) {
        if (q >= fl.size() || fl[q] < 3 || q + (size_t)fl[q] >= fl.size()) return fail(FY_ERR_INVALID, "%s/faces: face %zu is cut short or has fewer than three points", base.c_str(), f);
        const int n = fl[q++];
        for (int m = 0; m < n; ++m, ++q) {
            if (fl[q] < 0 || (size_t)fl[q] >= npts) return fail(FY_ERR_INVALID, "%s/faces: face %zu names point %d of %zu", base.c_str(), f, fl[q], npts);
            c->g_face_pts.push_back(fl[q]);
        }
        c->g_face_off.push_back((int32_t)c->g_face_pts.size());
    }
    if (q != fl.size()) return fail(FY_ERR_INVALID, "%s/faces: %zu labels follow the last of the %zu faces", base.c_str(), fl.size() - q, nfaces);
    { std::vector<int32_t>().swap(fl); }
    if (!fy::foam_label_list_file(join(base, "owner"), &c->g_own, &err)) return fail(FY_ERR_INVALID, "%s", err.c_str());
    if (c->g_own.empty() || (size_t)c->g_own[0] != c->g_own.size() - 1 || c->g_own.size() - 1 != nfaces) return fail(FY_ERR_INVALID, "%s/owner: %zu entries for %zu faces", base.c_str(), c->g_own.size() - 1, nfaces);
    c->g_own.erase(c->g_own.begin());
    if (!fy::foam_label_list_file(join(base, "neighbour"), &c->g_nei, &err)) return fail(FY_ERR_INVALID, "%s", err.c_str());
    if (c->g_nei.empty() || (size_t)c->g_nei[0] != c->g_nei.size() - 1 || c->g_nei.size() - 1 > nfaces) return fail(FY_ERR_INVALID, "%s/neighbour: malformed", base.c_str());
    c->g_nei.erase(c->g_nei.begin());
    c->g_internal = (int)c->g_nei.size();
    int32_t top = -1;
    // nCells = the highest cell label in owner OR neighbour, + 1 [OF-6 polyMesh::initMesh]: the highest-numbered cells own no internal face (owner <
    // neighbour) and, when they lie in the interior, no boundary face either -- they appear in `neighbour` only (tests/test_case_vs_oracle.py found it)
    for (int32_t v : c->g_own) top = std::max(top, v);
    for (int32_t v : c->g_nei) top = std::max(top, v);
    c->g_cells = top + 1;
    std::vector<std::string> tk;
    if (!fy::foam_list_file_tokens(join(base, "boundary"), &tk, &err)) return fail(FY_ERR_INVALID, "%s", err.c_str());
    std::vector<std::pair<std::string, FoamDict> > patches;
    FY_TRY(named_dicts(tk, base + "/boundary", &patches));
    std::vector<std::string> cyc_nbr;
    for (auto& pd : patches) {
        int nf = 0, sf = 0;
        std::string ty;
        pd.second.word("type", &ty);
        if (!pd.second.integer("nFaces", &nf) || !pd.second.integer("startFace", &sf) || nf < 0 || sf < c->g_internal || (size_t)sf + (size_t)nf > nfaces)
            return fail(FY_ERR_INVALID, "%s/boundary: patch '%s' needs nFaces and startFace among the boundary faces", base.c_str(), pd.first.c_str());
        // the patch classes fy_ldu_solver has conditions for: another constraint patch (empty, wedge, processor) would be silently treated as a wall
        if (nf > 0 && ty != "wall" && ty != "patch" && ty != "symmetryPlane" && ty != "symmetry" && ty != "cyclic")
            return fail(FY_ERR_UNSUPPORTED, "%s/boundary: patch '%s' of type '%s' is not supported on a general mesh (wall, patch, symmetryPlane, symmetry, cyclic)", base.c_str(), pd.first.c_str(), ty.c_str());
        std::string nbr, tf;
        if (ty == "cyclic") {
            if (!pd.second.word("neighbourPatch", &nbr)) return fail(FY_ERR_INVALID, "%s/boundary: cyclic patch '%s' needs neighbourPatch", base.c_str(), pd.first.c_str());
            if (pd.second.word("transform", &tf) && tf != "translational" && tf != "unknown" && tf != "noOrdering" && tf != "none")
                return fail(FY_ERR_UNSUPPORTED, "%s/boundary: cyclic patch '%s': transform '%s' is not supported (translational cyclics)", base.c_str(), pd.first.c_str(), tf.c_str());
        }
        cyc_nbr.push_back(nbr);
        c->g_patch_name.push_back(pd.first);
        c->g_patch_class.push_back(ty);
        c->g_patch_start.push_back(sf);
        c->g_patch_size.push_back(nf);
    }
    if (c->g_patch_name.empty()) return fail(FY_ERR_INVALID, "%s/boundary: no patches", base.c_str());
    c->g_patch_neighbour.assign(c->g_patch_name.size(), -1);
    for (size_t a = 0; a < cyc_nbr.size(); ++a) {
        if (cyc_nbr[a].empty()) continue;
        for (size_t b = 0; b < c->g_patch_name.size(); ++b) if (c->g_patch_name[b] == cyc_nbr[a] && b != a && c->g_patch_class[b] == "cyclic") c->g_patch_neighbour[a] = (int32_t)b;
        if (c->g_patch_neighbour[a] < 0) return fail(FY_ERR_INVALID, "%s/boundary: cyclic patch '%s': neighbourPatch '%s' is not another cyclic patch", base.c_str(), c->g_patch_name[a].c_str(), cyc_nbr[a].c_str());
    }
    c->patch_order = c->g_patch_name;
    return FY_OK;
}

// what fy_ldu_solver discretises with (include/foamyade_hip.h): Gauss linear convection, Gauss linear corrected laplacian, corrected snGrad.  read_controls
// has refused everything the lattice solver cannot do; on a general mesh "orthogonal" / "uncorrected" are different schemes, and so are the upwinded ones
int check_general_schemes(const fy_foam_case* c) {
    const std::string path = join(c->dir, "system/fvSchemes");
    FoamDict d;
    FY_TRY(need_file(path, &d));
    for (const char* dn : {"laplacianSchemes", "snGradSchemes"}) {
        const FoamDict* sd = d.subdict(dn);
        for (const std::string& k : sd->order) {
            const auto* tk = sd->tokens(k);
            if (!tk) continue;
            bool corrected = false;
            for (const std::string& t : *tk) corrected = corrected || t == "corrected";
            if (!corrected) return fail(FY_ERR_UNSUPPORTED, "%s: %s.%s: on a general mesh the scheme must be 'corrected' (the full non-orthogonal correction, icoFoamYade.C:114-131)", path.c_str(), dn, k.c_str());
        }
    }
    return FY_OK;
}


// porousZones { <name> { type DarcyForchheimer; box (x0 y0 z0) (x1 y1 z1); d (dx dy dz); f (fx fy fz); active on; } ... } of constant/couplingProperties: the role of
// the explicitPorositySource fvOption with a diagonal tensor in the global axes -- constant/fvOptions itself is not read, as the reference's solvers do not read it.
// A cell belongs to a zone if its centre lies in the closed box [OF-6 boxToCell]; the centres are the solver's own (a block's from its origin and cell sizes, a
// general mesh's from LduHostMesh::build).  Nothing of it is written to a time directory: a restart reads the same file
int read_porous_zones(fy_foam_case* c, const FoamDict& d, const std::string& path) {
    c->porous.clear();
    if (!d.has("porousZones")) return FY_OK;
    const char* accepted = "type, box, d, f, active";
    const FoamDict* pz = d.subdict("porousZones");
    if (!pz) return fail(FY_ERR_INVALID, "%s: porousZones must be a dictionary { <name> { %s } ... }", path.c_str(), accepted);
    std::vector<double> ctr;                                       // [3 n] cell centres by solver cell label, formed for the first active zone
    auto centres = [&]() -> int {
        if (!ctr.empty()) return FY_OK;
        if (c->general) {
            fy_poly_mesh pm;
            FY_TRY(fy_foam_case_poly_mesh(c, &pm));
            fy::LduHostMesh hm;
            FY_TRY(hm.build(&pm));
            ctr = hm.C;
            return FY_OK;
        }
        const fy_case_desc& cd = c->desc;
        std::vector<double> x[3];
        const int n[3] = {cd.nx, cd.ny, cd.nz};
        for (int a = 0; a < 3; ++a) {
            x[a].resize((size_t)n[a]);
            double node = cd.origin[a];
            for (int q = 0; q < n[a]; ++q) {
                if (c->grading[a].empty()) x[a][(size_t)q] = cd.origin[a] + ((double)q + 0.5) * cd.dx;
                else { x[a][(size_t)q] = node + 0.5 * c->grading[a][(size_t)q]; node += c->grading[a][(size_t)q]; }
            }
        }
        ctr.resize(3 * (size_t)n[0] * n[1] * n[2]);
        size_t l = 0;
        for (int k = 0; k < n[2]; ++k) for (int j = 0; j < n[1]; ++j) for (int i = 0; i < n[0]; ++i, ++l) { ctr[3 * l] = x[0][(size_t)i]; ctr[3 * l + 1] = x[1][(size_t)j]; ctr[3 * l + 2] = x[2][(size_t)k]; }
        return FY_OK;
    };
    std::vector<int> owner;                                        // per cell: 1 + the zone that took it
    for (const std::string& name : pz->order) {
        const FoamDict* z = pz->subdict(name);
        if (!z) return fail(FY_ERR_INVALID, "%s: porousZones.%s must be a dictionary { %s }", path.c_str(), name.c_str(), accepted);
        for (const std::string& k : z->order)
            if (k != "type" && k != "box" && k != "d" && k != "f" && k != "active")
                return fail(FY_ERR_UNSUPPORTED, "%s: porousZones.%s.%s is not an entry this reader knows (%s; a zone is a box in the global axes)", path.c_str(), name.c_str(), k.c_str(), accepted);
        std::string w;
        if (!z->word("type", &w) || w != "DarcyForchheimer")
            return fail(FY_ERR_UNSUPPORTED, "%s: porousZones.%s.type %s; accepts DarcyForchheimer", path.c_str(), name.c_str(), w.empty() ? "(missing)" : w.c_str());
        bool active = true;
        if (z->has("active") && !z->boolean("active", &active)) { z->word("active", &w); return fail(FY_ERR_UNSUPPORTED, "%s: porousZones.%s.active %s; accepts on | off", path.c_str(), name.c_str(), w.c_str()); }
        fy_foam_case::PorousMeta m;
        m.name = name;
        const std::vector<std::string>* t = z->tokens("box");
        bool ok = t && t->size() == 10 && (*t)[0] == "(" && (*t)[4] == ")" && (*t)[5] == "(" && (*t)[9] == ")";
        for (int a = 0; ok && a < 3; ++a) {
            char *e0 = nullptr, *e1 = nullptr;
            m.lo[a] = std::strtod((*t)[(size_t)(1 + a)].c_str(), &e0); m.hi[a] = std::strtod((*t)[(size_t)(6 + a)].c_str(), &e1);
            ok = *e0 == 0 && *e1 == 0 && std::isfinite(m.lo[a]) && std::isfinite(m.hi[a]);
        }
        if (!ok) return fail(FY_ERR_UNSUPPORTED, "%s: porousZones.%s.box is missing or not two points; accepts (x0 y0 z0) (x1 y1 z1)", path.c_str(), name.c_str());
        for (const char* key : {"d", "f"}) {
            double* v = key[0] == 'd' ? m.d : m.f;
            if (!z->vector3(key, v)) return fail(FY_ERR_UNSUPPORTED, "%s: porousZones.%s.%s is missing or not a vector; accepts (x y z), per global axis, in %s", path.c_str(), name.c_str(), key, key[0] == 'd' ? "1/m^2" : "1/m");
            for (int a = 0; a < 3; ++a)
                if (!std::isfinite(v[a]) || v[a] < 0) return fail(FY_ERR_UNSUPPORTED, "%s: porousZones.%s.%s has a negative or non-finite component %g; accepts values >= 0", path.c_str(), name.c_str(), key, v[a]);
        }
        if (!active) continue;
        if (c->proc_count > 0)
            return fail(FY_ERR_UNSUPPORTED, "%s: porousZones.%s: porous zones are not available on z-slabs (a decomposed case, -parallel); accepts active off", path.c_str(), name.c_str());
        if (c->porous.size() == FY_POROUS_MAX_ZONES) return fail(FY_ERR_UNSUPPORTED, "%s: porousZones holds more than %d active zones (FY_POROUS_MAX_ZONES)", path.c_str(), FY_POROUS_MAX_ZONES);
        if (name.size() > 31) return fail(FY_ERR_UNSUPPORTED, "%s: porousZones.%s: a zone's name has at most 31 characters", path.c_str(), name.c_str());
        FY_TRY(centres());
        const size_t n = ctr.size() / 3;
        owner.resize(n, 0);
        for (size_t l = 0; l < n; ++l) {
            bool in = true;
            for (int a = 0; a < 3; ++a) in = in && ctr[3 * l + (size_t)a] >= m.lo[a] && ctr[3 * l + (size_t)a] <= m.hi[a];
            if (!in) continue;
            if (owner[l]) return fail(FY_ERR_UNSUPPORTED, "%s: porousZones.%s and porousZones.%s overlap (cell %zu lies in both boxes); accepts boxes that share no cell centre", path.c_str(),
                                      c->porous[(size_t)owner[l] - 1].name.c_str(), name.c_str(), l);
            owner[l] = (int)c->porous.size() + 1;
            m.cells.push_back((int32_t)l);
        }
        if (m.cells.empty()) return fail(FY_ERR_UNSUPPORTED, "%s: porousZones.%s.box (%g %g %g) (%g %g %g) selects no cell (a cell belongs to the zone if its centre lies in the closed box)", path.c_str(), name.c_str(),
                                         m.lo[0], m.lo[1], m.lo[2], m.hi[0], m.hi[1], m.hi[2]);
        c->porous.push_back(std::move(m));
    }
    return FY_OK;
}

// constant/couplingProperties (optional; not a file of the reference, whose closures are fixed in FoamYade.C): the drag closure and the opt-in force
// models of the case's coupling object -- fy_set_drag_law / fy_set_force_models, applied when a solver is made from the case.  One reader for block and
// general cases; a missing file or entry leaves the reference's behaviour, a word the case's solver cannot take is refused here
int read_coupling_properties(fy_foam_case* c) {
    c->desc.drag_law = FY_DRAG_REFERENCE; c->desc.force_models = 0;
    c->desc.thermal = fy_thermal_desc{};
    c->desc.solid_stats = 0;
    c->flow = fy_flow_control_desc{};
    const std::string path = join(c->dir, "constant/couplingProperties");
    if (!file_exists(path)) return FY_OK;
    FoamDict d;
    FY_TRY(need_file(path, &d));
    const bool gaussian = c->solver == FY_SOLVER_PIMPLE;          // pimpleFoamYade.C:52; icoFoamYade couples point forces (icoFoamYade.C:53)
    const char* solver = gaussian ? "pimpleFoamYade" : "icoFoamYade";
    std::string w;
    if (d.word("dragModel", &w)) {
        static const struct { const char* word; int law; bool gaussian, point; } laws[] = {
            {"reference", FY_DRAG_REFERENCE, true, true}, {"DiFelice", FY_DRAG_DI_FELICE, true, false}, {"KochHill", FY_DRAG_KOCH_HILL, true, false},
            {"Beetstra", FY_DRAG_BEETSTRA, true, false}, {"SchillerNaumann", FY_DRAG_SCHILLER_NAUMANN, false, true}};
        bool ok = false;
        for (const auto& l : laws) if (w == l.word && (gaussian ? l.gaussian : l.point)) { c->desc.drag_law = l.law; ok = true; }
        if (!ok) return fail(FY_ERR_UNSUPPORTED, "%s: dragModel %s; %s accepts %s", path.c_str(), w.c_str(), solver,
                             gaussian ? "reference | DiFelice | KochHill | Beetstra" : "reference | SchillerNaumann");
    }
    if (d.word("liftModel", &w)) {
        if (w == "SaffmanMei" && gaussian) c->desc.force_models |= FY_FORCE_SAFFMAN_MEI_LIFT;
        else if (w != "none") return fail(FY_ERR_UNSUPPORTED, "%s: liftModel %s; %s accepts %s", path.c_str(), w.c_str(), solver, gaussian ? "none | SaffmanMei" : "none");
    }
    const struct { const char* key; unsigned flag; } switches[] = {{"addedMass", FY_FORCE_ADDED_MASS}, {"gaussianTorque", FY_FORCE_GAUSSIAN_TORQUE}};
    for (const auto& sw : switches) {
        if (!d.has(sw.key)) continue;
        bool on = false;
        d.word(sw.key, &w);
        if (!d.boolean(sw.key, &on) || (on && !gaussian))
            return fail(FY_ERR_UNSUPPORTED, "%s: %s %s; %s accepts %s", path.c_str(), sw.key, w.c_str(), solver, gaussian ? "on | off" : "off");
        if (on) c->desc.force_models |= sw.flag;
    }
    // solidStatistics on | off: the solid-phase statistics (fy_solver_set_solid_statistics), for both solvers, block and general cases; one domain only
    if (d.has("solidStatistics")) {
        bool on = false;
        d.word("solidStatistics", &w);
        if (!d.boolean("solidStatistics", &on)) return fail(FY_ERR_UNSUPPORTED, "%s: solidStatistics %s; %s accepts on | off", path.c_str(), w.c_str(), solver);
        if (on && c->proc_count > 0)
            return fail(FY_ERR_UNSUPPORTED, "%s: solidStatistics on: solid statistics are not available on z-slabs (a decomposed case, -parallel); accepts off", path.c_str());
        c->desc.solid_stats = on ? 1 : 0;
    }
    // heatTransfer { active; nusseltModel; Cp; kappa; Prt; particleTemperature; particleCp; beta; TRef; }: the fluid temperature equation, the particles' heat
    // exchange and, with the last three, particle temperatures that evolve and Boussinesq buoyancy (fy_thermal_desc); 0/T, div(phi,T) | div(alphaPhic,T) and solvers.T complete it (read_controls, read_fields)
    if (d.has("heatTransfer")) {
        const FoamDict* h = d.subdict("heatTransfer");
        if (!h) return fail(FY_ERR_INVALID, "%s: heatTransfer must be a dictionary { active; nusseltModel; Cp; kappa; Prt; particleTemperature; particleCp; beta; TRef; }", path.c_str());
        for (const std::string& k : h->order)
            if (k != "active" && k != "nusseltModel" && k != "Cp" && k != "kappa" && k != "Prt" && k != "particleTemperature" && k != "particleCp" && k != "beta" && k != "TRef")
                return fail(FY_ERR_UNSUPPORTED, "%s: heatTransfer.%s is not an entry this reader knows (active, nusseltModel, Cp, kappa, Prt, particleTemperature, particleCp, beta, TRef)",
                            path.c_str(), k.c_str());
        bool active = true;
        if (h->has("active") && !h->boolean("active", &active)) { h->word("active", &w); return fail(FY_ERR_UNSUPPORTED, "%s: heatTransfer.active %s; accepts on | off", path.c_str(), w.c_str()); }
        if (active) {
            fy_thermal_desc& t = c->desc.thermal;
            if (c->general) return fail(FY_ERR_UNSUPPORTED, "%s: heatTransfer.active on: heat transfer runs on the structured block only, and this case holds a general mesh; accepts off", path.c_str());
            if (c->proc_count > 0) return fail(FY_ERR_UNSUPPORTED, "%s: heatTransfer.active on: heat transfer is not available on z-slabs (a decomposed case, -parallel); accepts off", path.c_str());
            t.on = 1;
            t.nusselt_law = FY_NUSSELT_RANZ_MARSHALL;
            if (h->word("nusseltModel", &w)) {
                if (w == "Gunn" && gaussian) t.nusselt_law = FY_NUSSELT_GUNN;
                else if (w != "RanzMarshall") return fail(FY_ERR_UNSUPPORTED, "%s: heatTransfer.nusseltModel %s; %s accepts %s", path.c_str(), w.c_str(), solver, gaussian ? "RanzMarshall | Gunn" : "RanzMarshall");
            }
            if (!h->scalar("Cp", &t.cp) || !(t.cp > 0)) return fail(FY_ERR_UNSUPPORTED, "%s: heatTransfer.Cp is missing or not positive; accepts a specific heat in J/kg/K", path.c_str());
            if (!h->scalar("kappa", &t.kappa) || !(t.kappa > 0)) return fail(FY_ERR_UNSUPPORTED, "%s: heatTransfer.kappa is missing or not positive; accepts a conductivity in W/m/K", path.c_str());
            t.prt = 1.0;
            if (h->has("Prt") && (!h->scalar("Prt", &t.prt) || !(t.prt > 0))) return fail(FY_ERR_UNSUPPORTED, "%s: heatTransfer.Prt must be a positive number", path.c_str());
            if (h->has("particleTemperature") && !h->scalar("particleTemperature", &t.particle_temperature))
                return fail(FY_ERR_UNSUPPORTED, "%s: heatTransfer.particleTemperature must be a number (the uniform temperature of the particles, K)", path.c_str());
            if (h->has("particleCp") && (!h->scalar("particleCp", &t.particle_cp) || !(t.particle_cp >= 0)))
                return fail(FY_ERR_UNSUPPORTED, "%s: heatTransfer.particleCp must be a number that is not negative (the particles' specific heat in J/kg/K; 0: their temperatures stay as given)", path.c_str());
            if (h->has("beta") && (!h->scalar("beta", &t.beta) || !std::isfinite(t.beta)))
                return fail(FY_ERR_UNSUPPORTED, "%s: heatTransfer.beta must be a number (the thermal expansion coefficient in 1/K; 0: no buoyancy)", path.c_str());
            if (h->has("TRef") && (!h->scalar("TRef", &t.T_ref) || !std::isfinite(t.T_ref)))
                return fail(FY_ERR_UNSUPPORTED, "%s: heatTransfer.TRef must be a number (the temperature at which the buoyancy vanishes, K)", path.c_str());
            if (t.beta != 0.0 && !h->has("TRef"))
                return fail(FY_ERR_UNSUPPORTED, "%s: heatTransfer.beta %g needs heatTransfer.TRef, the temperature at which the buoyancy vanishes", path.c_str(), t.beta);
            t.T_convection_scheme = FY_CONVECTION_LINEAR;
        }
    }
    // meanVelocityForce { Ubar; relaxation; superficial; selectionMode all; fields (U); active; }: flow-rate control of a general-mesh case (fy_flow_control_desc), the
    // role of the fvOption of that name -- constant/fvOptions itself is not read, as the reference's solvers do not read it.  gradient0 is the start time's
    // uniform/meanVelocityForceProperties `gradient`, when that file is there [OF-6 meanVelocityForce::meanVelocityForce, as recalled]
    if (d.has("meanVelocityForce")) {
        const char* accepted = "Ubar, relaxation, superficial, selectionMode, fields, active";
        const FoamDict* m = d.subdict("meanVelocityForce");
        if (!m) return fail(FY_ERR_INVALID, "%s: meanVelocityForce must be a dictionary { %s }", path.c_str(), accepted);
        for (const std::string& k : m->order)
            if (k != "Ubar" && k != "relaxation" && k != "superficial" && k != "selectionMode" && k != "fields" && k != "active")
                return fail(FY_ERR_UNSUPPORTED, "%s: meanVelocityForce.%s is not an entry this reader knows (%s)", path.c_str(), k.c_str(), accepted);
        bool active = true;
        if (m->has("active") && !m->boolean("active", &active)) { m->word("active", &w); return fail(FY_ERR_UNSUPPORTED, "%s: meanVelocityForce.active %s; accepts on | off", path.c_str(), w.c_str()); }
        if (active) {
            fy_flow_control_desc& f = c->flow;
            if (!c->general) return fail(FY_ERR_UNSUPPORTED, "%s: meanVelocityForce.active on: flow-rate control needs a general mesh: the block has no periodic sides; accepts off", path.c_str());
            if (m->word("selectionMode", &w) && w != "all") return fail(FY_ERR_UNSUPPORTED, "%s: meanVelocityForce.selectionMode %s; accepts all", path.c_str(), w.c_str());
            if (const std::vector<std::string>* t = m->tokens("fields")) {
                if (t->size() != 3 || (*t)[0] != "(" || (*t)[2] != ")" || (*t)[1] != c->u_name) {
                    std::string got;
                    for (const std::string& x : *t) got += (got.empty() ? "" : " ") + x;
                    return fail(FY_ERR_UNSUPPORTED, "%s: meanVelocityForce.fields %s; accepts (%s)", path.c_str(), got.c_str(), c->u_name.c_str());
                }
            }
            if (!m->vector3("Ubar", f.ubar)) return fail(FY_ERR_UNSUPPORTED, "%s: meanVelocityForce.Ubar is missing or not a vector; accepts (Ux Uy Uz), the bulk velocity to hold", path.c_str());
            const double m2 = f.ubar[0] * f.ubar[0] + f.ubar[1] * f.ubar[1] + f.ubar[2] * f.ubar[2];
            if (!std::isfinite(m2) || !(m2 > 0)) return fail(FY_ERR_UNSUPPORTED, "%s: meanVelocityForce.Ubar must be finite and not zero", path.c_str());
            f.relaxation = 1.0;
            if (m->has("relaxation") && (!m->scalar("relaxation", &f.relaxation) || !(f.relaxation >= 0 && f.relaxation <= 1)))
                return fail(FY_ERR_UNSUPPORTED, "%s: meanVelocityForce.relaxation must be a number in [0, 1]", path.c_str());
            bool sup = false;
            if (m->has("superficial")) {
                m->word("superficial", &w);
                if (!m->boolean("superficial", &sup) || (sup && !gaussian))
                    return fail(FY_ERR_UNSUPPORTED, "%s: meanVelocityForce.superficial %s; %s accepts %s", path.c_str(), w.c_str(), solver, gaussian ? "on | off" : "off");
            }
            f.superficial = sup ? 1 : 0;
            f.gradient0 = 0.0;
            const std::string rpath = join(join(c->fdir, c->start_name), "uniform/meanVelocityForceProperties");
            if (file_exists(rpath)) {
                FoamDict r;
                FY_TRY(need_file(rpath, &r));
                if (!r.scalar("gradient", &f.gradient0) || !std::isfinite(f.gradient0)) return fail(FY_ERR_INVALID, "%s: needs `gradient <number>;`", rpath.c_str());
            }
            f.on = 1;
        }
    }
    FY_TRY(read_porous_zones(c, d, path));
    return FY_OK;
}

const char* monitor_op_word(int op) {
    static const char* const nm[] = {"", "sum", "average", "volAverage", "volIntegrate", "weightedVolAverage", "min", "max", "areaAverage", "areaIntegrate", "weightedAverage"};
    return op >= FY_MONITOR_SUM && op <= FY_MONITOR_WEIGHTED_AVERAGE ? nm[op] : "?";
}

// the solid statistics' fields (constant/couplingProperties solidStatistics on) as fieldAverage and volFieldValue name them: whether the case has `stem`, and the
// words they add to an accepted-fields list
bool has_solid_stat(const fy_foam_case* c, const std::string& stem) { return c->desc.solid_stats != 0 && (stem != "TParticle" || c->desc.thermal.on); }
std::string solid_stats_words(const fy_foam_case* c) {
    if (!c->desc.solid_stats) return std::string();
    return std::string(", nParticle, solidFraction, uSolid, granularTemperature, dSauter") + (c->desc.thermal.on ? ", TParticle" : "");
}

// One volFieldValue / surfaceFieldValue object of controlDict `functions` [OF-6 fieldValue, volFieldValue, surfaceFieldValue as recalled] -> desc.monitors and c->monitors.
// Accepted: fields (file names), operation, weightField, regionType all | patch with name, writeFields false, writeControl / executeControl timeStep with
// writeInterval / executeInterval N, enabled, libs, log.  Everything else the function objects offer is refused by name
int read_monitor(fy_foam_case* c, const std::string& name, const std::string& ty, const FoamDict* o, const std::string& where) {
    const char* w = where.c_str();
    const bool vol = ty == "volFieldValue";
    static const char* const keys[] = {"type", "libs", "log", "enabled", "fields", "operation", "weightField", "regionType", "name", "writeFields", "writeControl",
                                       "executeControl", "writeInterval", "executeInterval"};
    for (const std::string& k : o->order) {
        bool known = false;
        for (const char* a : keys) known = known || k == a;
        if (!known) return fail(FY_ERR_UNSUPPORTED, "%s: %s is not supported; accepted: type, libs, log, enabled, fields, operation, weightField, regionType, name, writeFields false, "
                                                    "writeControl | executeControl timeStep, writeInterval | executeInterval", w, k.c_str());
    }
    if (c->proc_count > 1)
        return fail(FY_ERR_UNSUPPORTED, "%s: type %s is not available in a decomposed (-parallel) run; accepted: an undecomposed case on one domain, or 'enabled false'", w, ty.c_str());
    fy_monitor_desc& md = c->desc.monitors;
    if (md.n_objects >= FY_MONITOR_MAX_OBJECTS)
        return fail(FY_ERR_UNSUPPORTED, "%s: more than %d volFieldValue / surfaceFieldValue objects; accepted: at most %d", w, FY_MONITOR_MAX_OBJECTS, FY_MONITOR_MAX_OBJECTS);
    if (name.size() >= sizeof(md.objects[0].name)) return fail(FY_ERR_UNSUPPORTED, "%s: the object's name is longer than %zu characters; accepted: a shorter name", w, sizeof(md.objects[0].name) - 1);
    fy_monitor_object ob{};
    fy_foam_case::MonMeta meta;
    meta.name = name; meta.vol = vol;
    std::snprintf(ob.name, sizeof(ob.name), "%s", name.c_str());
    ob.kind = vol ? FY_MONITOR_VOL : FY_MONITOR_SURFACE;
    std::string word;
    if (!o->word("regionType", &word) || word != (vol ? "all" : "patch"))
        return fail(FY_ERR_UNSUPPORTED, "%s: regionType %s is not supported; accepted: %s", w, word.empty() ? "(absent)" : word.c_str(), vol ? "all" : "patch (with name <patch>)");
    meta.region = "all";
    if (!vol) {
        std::string pn;
        if (!o->word("name", &pn)) return fail(FY_ERR_INVALID, "%s: regionType patch needs 'name <patch>;'", w);
        const std::vector<std::string> patches = field_patches(c);
        std::string all;
        int found = -1, mask = 0;
        for (size_t q = 0; q < patches.size(); ++q) {
            if (patches[q] == pn) { found = (int)q; mask |= 1 << q; }
            if (all.find(patches[q]) == std::string::npos) all += (all.empty() ? "" : ", ") + patches[q];
        }
        if (found < 0) return fail(FY_ERR_UNSUPPORTED, "%s: name %s: the mesh has no such patch; accepted: %s", w, pn.c_str(), all.c_str());
        if (c->general && c->g_patch_neighbour.size() > (size_t)found && c->g_patch_neighbour[(size_t)found] >= 0)
            return fail(FY_ERR_UNSUPPORTED, "%s: name %s is a cyclic patch, whose faces are internal faces of the solver's mesh; accepted: a patch of boundary faces", w, pn.c_str());
        ob.patch = c->general ? found : mask;                    // (block: one patch may cover several sides -- `walls`)
        meta.region = pn;
    }
    static const struct { const char* word; int op; int kinds; } ops[] = {
        {"sum", FY_MONITOR_SUM, 3}, {"average", FY_MONITOR_AVERAGE, 3}, {"min", FY_MONITOR_MIN, 3}, {"max", FY_MONITOR_MAX, 3},
        {"volAverage", FY_MONITOR_VOL_AVERAGE, 1}, {"volIntegrate", FY_MONITOR_VOL_INTEGRATE, 1}, {"weightedVolAverage", FY_MONITOR_WEIGHTED_VOL_AVERAGE, 1},
        {"areaAverage", FY_MONITOR_AREA_AVERAGE, 2}, {"areaIntegrate", FY_MONITOR_AREA_INTEGRATE, 2}, {"weightedAverage", FY_MONITOR_WEIGHTED_AVERAGE, 2}};
    word.clear();
    o->word("operation", &word);
    for (const auto& e : ops) if (word == e.word && (e.kinds & (vol ? 1 : 2))) ob.operation = e.op;
    if (!ob.operation)
        return fail(FY_ERR_UNSUPPORTED, "%s: operation %s is not supported; accepted: %s", w, word.empty() ? "(absent)" : word.c_str(),
                    vol ? "sum, average, volAverage, volIntegrate, weightedVolAverage, min, max" : "sum, average, areaAverage, areaIntegrate, weightedAverage, min, max");
    const bool weighted = ob.operation == FY_MONITOR_WEIGHTED_VOL_AVERAGE || ob.operation == FY_MONITOR_WEIGHTED_AVERAGE;
    const std::string want_w = vol ? field_name(c, F_ALPHA) : std::string("phi");
    word.clear();
    if (o->word("weightField", &word)) {
        if (word != want_w || (vol && !has_field(c, F_ALPHA)))
            return fail(FY_ERR_UNSUPPORTED, "%s: weightField %s is not supported; accepted: %s", w, word.c_str(), vol ? (has_field(c, F_ALPHA) ? want_w.c_str() : "none (icoFoamYade has no void fraction)") : "phi");
        std::snprintf(ob.weight_field, sizeof(ob.weight_field), "%s", vol ? "alpha" : "phi");
    } else if (weighted)
        return fail(FY_ERR_UNSUPPORTED, "%s: operation %s needs a weightField; accepted: weightField %s", w, monitor_op_word(ob.operation), want_w.c_str());
    bool wf = false;
    word.clear();
    o->word("writeFields", &word);
    if (o->has("writeFields") && (!o->boolean("writeFields", &wf) || wf)) return fail(FY_ERR_UNSUPPORTED, "%s: writeFields %s is not supported; accepted: false", w, word.c_str());
    for (const char* key : {"writeControl", "executeControl"})
        if (o->word(key, &word) && word != "timeStep") return fail(FY_ERR_UNSUPPORTED, "%s: %s %s is not supported; accepted: timeStep (with writeInterval N)", w, key, word.c_str());
    double iv = 1, iv2 = 0;
    const bool h1 = o->scalar("writeInterval", &iv), h2 = o->scalar("executeInterval", &iv2);
    if (!h1 && h2) iv = iv2;
    if ((h1 && h2 && iv != iv2) || !(iv >= 1) || iv != std::floor(iv) || iv > 1e9)
        return fail(FY_ERR_UNSUPPORTED, "%s: writeInterval %g / executeInterval %g is not supported; accepted: one whole number of steps >= 1 for both", w, iv, h2 ? iv2 : iv);
    ob.interval = (int32_t)iv;
    const auto* ft = o->tokens("fields");
    if (!ft) return fail(FY_ERR_INVALID, "%s: no 'fields ( <name> ... )' list", w);
    const std::string ph = c->phase.empty() ? std::string("<phase>") : c->phase;
    const std::string accepted = vol ? c->u_name + ", p, alpha." + ph + ", nut." + ph + ", k." + ph + ", epsilon." + ph + ", uParticle, uSource" + (c->desc.thermal.on ? ", " + field_name(c, F_T) : std::string()) + solid_stats_words(c)
                                     : "phi, p, " + c->u_name + (c->desc.thermal.on ? ", " + field_name(c, F_T) : std::string());
    static const struct { const char* stem; int F; int ncomp; bool surface; } known[] = {
        {"U", F_U, 3, true}, {"p", F_P, 1, true}, {"alpha", F_ALPHA, 1, false}, {"nut", F_NUT, 1, false}, {"k", F_K, 1, false}, {"epsilon", F_EPS, 1, false},
        {"uParticle", -1, 3, false}, {"uSource", -1, 3, false}, {"T", F_T, 1, true}, {"phi", -2, 1, true},
        {"nParticle", -3, 1, false}, {"solidFraction", -3, 1, false}, {"uSolid", -3, 3, false}, {"granularTemperature", -3, 1, false}, {"dSauter", -3, 1, false}, {"TParticle", -3, 1, false}};
    for (const std::string& file : *ft) {
        double cnt;
        if (file == "(" || file == ")" || fy::foam_tok_is_number(file, &cnt)) continue;
        const std::string stem = file.substr(0, file.find('.'));
        const auto* kf = &known[0];
        bool is_known = false;
        for (const auto& k : known)
            if (stem == k.stem && (vol ? k.F != -2 : k.surface) && (k.F != F_T || c->desc.thermal.on) && (k.F != -3 || has_solid_stat(c, stem))) { kf = &k; is_known = true; }
        if (!is_known) return fail(FY_ERR_UNSUPPORTED, "%s: unknown field '%s'; accepted: %s", w, file.c_str(), accepted.c_str());
        const bool has = kf->F >= 0 ? (has_field(c, kf->F) && file == field_name(c, kf->F)) : (file == kf->stem && (stem != "uParticle" || c->solver == FY_SOLVER_PIMPLE));
        if (!has) return fail(FY_ERR_UNSUPPORTED, "%s: this case has no field '%s'; accepted: %s", w, file.c_str(), accepted.c_str());
        for (const std::string& f : meta.files) if (f == file) return fail(FY_ERR_INVALID, "%s: field '%s' is listed twice", w, file.c_str());
        if (ob.n_fields >= FY_MONITOR_MAX_FIELDS) return fail(FY_ERR_UNSUPPORTED, "%s: more than %d fields; accepted: at most %d", w, FY_MONITOR_MAX_FIELDS, FY_MONITOR_MAX_FIELDS);
        std::snprintf(ob.fields[ob.n_fields++], sizeof(ob.fields[0]), "%s", kf->stem);
        meta.files.push_back(file); meta.ncomp.push_back(kf->ncomp);
    }
    if (ob.n_fields == 0) return fail(FY_ERR_INVALID, "%s: the 'fields' list is empty", w);
    md.objects[md.n_objects++] = ob;
    md.start_time = c->start_time;
    c->monitors.push_back(meta);
    return FY_OK;
}

// One forces / wallShearStress / yPlus object of controlDict `functions` [OF-6 forces, wallShearStress, yPlus as recalled] -> desc.wall_loads and c->wl_*.
// forces: patches (...), rho rhoInf with rhoInf <v>, pRef (default 0), CofR; p, U, log, libs, enabled, writeControl | executeControl timeStep with writeInterval |
// executeInterval are accepted and unused beyond the interval.  wallShearStress / yPlus: an optional patches (...), default every patch of type wall.  Everything else
// is refused by name
int read_wall_load(fy_foam_case* c, const std::string& name, const std::string& ty, const FoamDict* o, const std::string& where) {
    const char* w = where.c_str();
    const int kind = ty == "forces" ? 0 : ty == "wallShearStress" ? 1 : 2;
    static const char* const common[] = {"type", "libs", "log", "enabled", "patches", "writeControl", "executeControl", "writeInterval", "executeInterval"};
    static const char* const only_forces[] = {"rho", "rhoInf", "pRef", "CofR", "p", "U"};
    const char* accepted = kind == 0 ? "type, libs, log, enabled, patches, rho rhoInf, rhoInf, pRef, CofR, p, U, writeControl | executeControl timeStep, writeInterval | executeInterval"
                                     : "type, libs, log, enabled, patches, writeControl | executeControl timeStep, writeInterval | executeInterval";
    for (const std::string& k : o->order) {
        bool known = false;
        for (const char* a : common) known = known || k == a;
        if (kind == 0) for (const char* a : only_forces) known = known || k == a;
        if (!known) return fail(FY_ERR_UNSUPPORTED, "%s: %s is not supported; accepted: %s", w, k.c_str(), accepted);
    }
    if (c->proc_count > 1)
        return fail(FY_ERR_UNSUPPORTED, "%s: type %s is not available in a decomposed (-parallel) run; accepted: an undecomposed case on one domain, or 'enabled false'", w, ty.c_str());
    fy_wall_loads_desc& wd = c->desc.wall_loads;
    if (kind == 0 && wd.n_forces >= FY_WALL_LOADS_MAX_FORCES)
        return fail(FY_ERR_UNSUPPORTED, "%s: more than %d forces objects; accepted: at most %d", w, FY_WALL_LOADS_MAX_FORCES, FY_WALL_LOADS_MAX_FORCES);
    if (kind != 0 && (kind == 1 ? wd.wall_shear_stress.on : wd.y_plus.on))
        return fail(FY_ERR_UNSUPPORTED, "%s: a second object of type %s (the first is '%s'); accepted: one enabled object of this type, with all patches in its list", w, ty.c_str(),
                    (kind == 1 ? c->wl_wss : c->wl_yplus)[0].name.c_str());
    if (name.size() >= sizeof(wd.forces[0].name)) return fail(FY_ERR_UNSUPPORTED, "%s: the object's name is longer than %zu characters; accepted: a shorter name", w, sizeof(wd.forces[0].name) - 1);
    std::string word;
    for (const char* key : {"writeControl", "executeControl"})
        if (o->word(key, &word) && word != "timeStep") return fail(FY_ERR_UNSUPPORTED, "%s: %s %s is not supported; accepted: timeStep (with writeInterval N)", w, key, word.c_str());
    double iv = 1, iv2 = 0;
    const bool h1 = o->scalar("writeInterval", &iv), h2 = o->scalar("executeInterval", &iv2);
    if (!h1 && h2) iv = iv2;
    if ((h1 && h2 && iv != iv2) || !(iv >= 1) || iv != std::floor(iv) || iv > 1e9)
        return fail(FY_ERR_UNSUPPORTED, "%s: writeInterval %g / executeInterval %g is not supported; accepted: one whole number of steps >= 1 for both", w, iv, h2 ? iv2 : iv);
    // the patch set: the names listed, or (wallShearStress, yPlus) every patch of type wall
    const std::vector<std::string> patches = field_patches(c);
    std::string all;
    for (const std::string& pn : patches) if (all.find(pn) == std::string::npos) all += (all.empty() ? "" : ", ") + pn;
    std::vector<std::string> want;
    if (const auto* pt = o->tokens("patches")) {
        for (const std::string& t : *pt) if (t != "(" && t != ")") want.push_back(t);
        if (want.empty()) return fail(FY_ERR_INVALID, "%s: the 'patches' list is empty; accepted: %s", w, all.c_str());
    } else if (kind == 0) {
        return fail(FY_ERR_INVALID, "%s: no 'patches ( <name> ... )' list; accepted: %s", w, all.c_str());
    } else {
        for (size_t q = 0; q < patches.size(); ++q) {
            const std::string cls = c->general ? c->g_patch_class[q] : c->class_of_side[q];
            if (cls == "wall" && std::find(want.begin(), want.end(), patches[q]) == want.end()) want.push_back(patches[q]);
        }
        if (want.empty()) return fail(FY_ERR_UNSUPPORTED, "%s: the mesh has no patch of type wall; accepted: patches ( <name> ... ) among %s", w, all.c_str());
    }
    fy_wall_patch_set set{};
    fy_foam_case::WlMeta meta;
    meta.name = name; meta.kind = kind;
    for (const std::string& pn : want) {
        if (std::find(meta.patches.begin(), meta.patches.end(), pn) != meta.patches.end()) return fail(FY_ERR_INVALID, "%s: patches: '%s' is listed twice", w, pn.c_str());
        int found = -1;
        for (size_t q = 0; q < patches.size(); ++q) if (patches[q] == pn) { if (found < 0) found = (int)q; set.sides |= 1 << q; }
        if (found < 0) return fail(FY_ERR_UNSUPPORTED, "%s: patches: the mesh has no patch '%s'; accepted: %s", w, pn.c_str(), all.c_str());
        if (c->general) {
            if (c->g_patch_neighbour.size() > (size_t)found && c->g_patch_neighbour[(size_t)found] >= 0)
                return fail(FY_ERR_UNSUPPORTED, "%s: patches: '%s' is a cyclic patch, whose faces are internal faces of the solver's mesh; accepted: patches of boundary faces", w, pn.c_str());
            if (set.n_patches >= FY_WALL_LOADS_MAX_PATCHES) return fail(FY_ERR_UNSUPPORTED, "%s: more than %d patches; accepted: at most %d", w, FY_WALL_LOADS_MAX_PATCHES, FY_WALL_LOADS_MAX_PATCHES);
            set.patches[set.n_patches++] = found;
        }
        meta.patches.push_back(pn);
    }
    if (c->general) set.sides = 0;
    else {                                       // a block's rows run over the SIDES of the set, in the order x- x+ y- y+ z- z+: one row entry per side, named by its patch
        meta.patches.clear();
        static const char* const side_word[] = {"x-", "x+", "y-", "y+", "z-", "z+"};
        for (int q = 0; q < 6; ++q)
            if ((set.sides >> q) & 1) meta.patches.push_back(std::count(patches.begin(), patches.end(), patches[(size_t)q]) > 1 ? patches[(size_t)q] + ":" + side_word[q] : patches[(size_t)q]);
    }
    wd.start_time = c->start_time;
    if (kind == 0) {
        word.clear();
        if (!o->word("rho", &word) || word != "rhoInf")
            return fail(FY_ERR_UNSUPPORTED, "%s: rho %s is not supported; accepted: rho rhoInf (with rhoInf <value>: the solvers are incompressible)", w, word.empty() ? "(absent)" : word.c_str());
        fy_forces_object fo{};
        std::snprintf(fo.name, sizeof(fo.name), "%s", name.c_str());
        fo.set = set; fo.interval = (int32_t)iv;
        if (!o->scalar("rhoInf", &fo.rho) || !(fo.rho > 0)) return fail(FY_ERR_INVALID, "%s: rho rhoInf needs 'rhoInf <value>;' with a positive value", w);
        if (o->has("pRef") && !o->scalar("pRef", &fo.p_ref)) return fail(FY_ERR_INVALID, "%s: pRef needs a number", w);
        if (!o->vector3("CofR", fo.cofr)) return fail(FY_ERR_INVALID, "%s: no 'CofR (x y z);'", w);
        wd.forces[wd.n_forces++] = fo;
        c->wl_forces.push_back(meta);
    } else {
        fy_wall_field_object& fo = kind == 1 ? wd.wall_shear_stress : wd.y_plus;
        fo.on = 1; fo.set = set; fo.interval = (int32_t)iv;
        (kind == 1 ? c->wl_wss : c->wl_yplus).push_back(meta);
    }
    return FY_OK;
}

// controlDict `functions` [OF-6 functionObjectList; fieldAverage / fieldAverageItem as recalled]: one fieldAverage object -> desc.average (solver field names)
// and c->avg_fields (file names); objects of other types are accepted and not run, their names kept.  Everything fieldAverage offers beyond the plain running
// mean / prime2Mean is refused by name.  Called last in read_controls: which fields the case has depends on the solver and the turbulence model.
int read_functions(fy_foam_case* c, const FoamDict& d, const std::string& path) {
    c->desc.average = fy_average_desc{};
    c->avg_name.clear(); c->avg_fields.clear(); c->ignored_functions.clear(); c->avg_restart_on_restart = false;
    c->desc.monitors = fy_monitor_desc{}; c->monitors.clear();
    c->desc.wall_loads = fy_wall_loads_desc{}; c->wl_forces.clear(); c->wl_wss.clear(); c->wl_yplus.clear();
    const FoamDict* fn = d.subdict("functions");
    if (!fn) return FY_OK;
    for (const std::string& name : fn->order) {
        const FoamDict* o = fn->subdict(name);
        if (!o) continue;
        std::string ty;
        o->word("type", &ty);
        const bool monitor = ty == "volFieldValue" || ty == "surfaceFieldValue";
        const bool wall_load = ty == "forces" || ty == "wallShearStress" || ty == "yPlus";
        if (ty != "fieldAverage" && !monitor && !wall_load) { c->ignored_functions.push_back(name + " (type " + (ty.empty() ? "?" : ty) + ")"); continue; }
        bool enabled = true;
        if (o->boolean("enabled", &enabled) && !enabled) continue;
        const std::string where = path + ": functions." + name;
        if (monitor) { FY_TRY(read_monitor(c, name, ty, o, where)); continue; }
        if (wall_load) { FY_TRY(read_wall_load(c, name, ty, o, where)); continue; }
        const char* w = where.c_str();
        if (!c->avg_name.empty())
            return fail(FY_ERR_UNSUPPORTED, "%s: a second object of type fieldAverage (the first is '%s'); accepted: one enabled fieldAverage object, with all fields in its list", w, c->avg_name.c_str());
        if (c->proc_count > 1)
            return fail(FY_ERR_UNSUPPORTED, "%s: type fieldAverage is not available in a decomposed (-parallel) run; accepted: an undecomposed case on one domain, or 'enabled false'", w);
        c->avg_name = name;
        if (o->has("window")) return fail(FY_ERR_UNSUPPORTED, "%s: window is not supported; accepted: no window (the average runs from timeStart on)", w);
        for (const char* key : {"restartOnOutput", "periodicRestart"}) {
            bool on = false;
            std::string word;
            o->word(key, &word);
            if (o->has(key) && (!o->boolean(key, &on) || on)) return fail(FY_ERR_UNSUPPORTED, "%s: %s %s is not supported; accepted: off", w, key, word.c_str());
        }
        std::string word;
        if (o->word("writeControl", &word) && word != "writeTime" && word != "outputTime")
            return fail(FY_ERR_UNSUPPORTED, "%s: writeControl %s is not supported; accepted: writeTime, outputTime (the averages are written with the time directory)", w, word.c_str());
        if (o->word("executeControl", &word) && word != "timeStep")
            return fail(FY_ERR_UNSUPPORTED, "%s: executeControl %s is not supported; accepted: timeStep with executeInterval 1 (a sample every step)", w, word.c_str());
        double iv = 1;
        if (o->scalar("executeInterval", &iv) && iv != 1) return fail(FY_ERR_UNSUPPORTED, "%s: executeInterval %g is not supported; accepted: 1 (a sample every step)", w, iv);
        if (o->has("restartOnRestart") && !o->boolean("restartOnRestart", &c->avg_restart_on_restart)) return fail(FY_ERR_INVALID, "%s: restartOnRestart must be on or off", w);
        double t0 = c->start_time, t1 = 0;
        if (o->scalar("timeStart", &t0)) c->desc.average.start_after = std::max(0.0, t0 - c->start_time);
        if (o->scalar("timeEnd", &t1)) c->desc.average.stop_after = t1 > c->start_time ? t1 - c->start_time : 1e-300;      // (an end at or before the start: never a sample)
        const auto* ft = o->tokens("fields");
        if (!ft) return fail(FY_ERR_INVALID, "%s: no 'fields ( <name> { mean ..; prime2Mean ..; base ..; } ... )' list", w);
        std::vector<std::pair<std::string, FoamDict> > fields;
        FY_TRY(named_dicts(*ft, where + ".fields", &fields));
        const std::string ph = c->phase.empty() ? std::string("<phase>") : c->phase;
        const std::string accepted = c->u_name + ", p, alpha." + ph + ", nut." + ph + ", k." + ph + ", epsilon." + ph + ", uParticle, uSource" + (c->desc.thermal.on ? ", " + field_name(c, F_T) : std::string()) +
                                     solid_stats_words(c);
        for (const auto& fd : fields) {
            const std::string& file = fd.first;
            const std::string fw = where + ".fields." + file;
            if (fd.second.has("window") || fd.second.has("windowName"))
                return fail(FY_ERR_UNSUPPORTED, "%s: window is not supported; accepted: no window (the average runs from timeStart on)", fw.c_str());
            bool mean = false, prime2 = false;
            if (!fd.second.boolean("mean", &mean) || !fd.second.boolean("prime2Mean", &prime2)) return fail(FY_ERR_INVALID, "%s: needs 'mean on|off;' and 'prime2Mean on|off;'", fw.c_str());
            std::string base;
            if (!fd.second.word("base", &base) || (base != "time" && base != "iteration"))
                return fail(FY_ERR_UNSUPPORTED, "%s: base %s is not supported; accepted: time, iteration", fw.c_str(), base.empty() ? "(absent)" : base.c_str());
            // the file name -> the case's field
            static const struct { const char* stem; int F; const char* solver_name; int ncomp; } known[] = {
                {"U", F_U, "U", 3}, {"p", F_P, "p", 1}, {"alpha", F_ALPHA, "alpha", 1}, {"nut", F_NUT, "nut", 1}, {"k", F_K, "k", 1}, {"epsilon", F_EPS, "epsilon", 1},
                {"uParticle", -1, "uParticle", 3}, {"uSource", -1, "uSource", 3}, {"T", F_T, "T", 1},
                {"nParticle", -3, "nParticle", 1}, {"solidFraction", -3, "solidFraction", 1}, {"uSolid", -3, "uSolid", 3}, {"granularTemperature", -3, "granularTemperature", 1},
                {"dSauter", -3, "dSauter", 1}, {"TParticle", -3, "TParticle", 1}};
            const std::string stem = file.substr(0, file.find('.'));
            const auto* kf = &known[0];
            bool is_known = false;
            for (const auto& k : known) if (stem == k.stem && (k.F != F_T || c->desc.thermal.on) && (k.F != -3 || has_solid_stat(c, stem))) { kf = &k; is_known = true; }      // (T is a field of a case with heat transfer only)
            if (!is_known) return fail(FY_ERR_UNSUPPORTED, "%s: unknown field '%s'; accepted: %s", fw.c_str(), file.c_str(), accepted.c_str());
            const bool has = kf->F >= 0 ? (has_field(c, kf->F) && file == field_name(c, kf->F))
                                        : (file == kf->stem && (stem != "uParticle" || c->solver == FY_SOLVER_PIMPLE));
            if (!has) return fail(FY_ERR_UNSUPPORTED, "%s: this case has no field '%s' (%s, %s); accepted: %s", fw.c_str(), file.c_str(),
                                  c->solver == FY_SOLVER_PIMPLE ? "pimpleFoamYade" : "icoFoamYade", c->desc.turbulence_model == FY_TURBULENCE_LAMINAR ? "laminar" : "with a turbulence model", accepted.c_str());
            if (!mean && prime2) return fail(FY_ERR_UNSUPPORTED, "%s: prime2Mean on needs mean on (OpenFOAM refuses it too); accepted: mean on with prime2Mean on|off, or both off", fw.c_str());
            if (!mean) continue;                       // mean off; prime2Mean off: nothing to keep
            for (const auto& a : c->avg_fields) if (a.file == file) return fail(FY_ERR_INVALID, "%s: the field is listed twice", fw.c_str());
            fy_average_desc& av = c->desc.average;
            if (av.n_items >= FY_AVERAGE_MAX_ITEMS) return fail(FY_ERR_UNSUPPORTED, "%s: more than %d averaged fields; accepted: at most %d", fw.c_str(), FY_AVERAGE_MAX_ITEMS, FY_AVERAGE_MAX_ITEMS);
            fy_average_item& it = av.items[av.n_items++];
            std::snprintf(it.field, sizeof(it.field), "%s", kf->solver_name);
            it.prime2_mean = prime2 ? 1 : 0; it.iteration_base = base == "iteration" ? 1 : 0;
            c->avg_fields.push_back({file, kf->F, kf->solver_name, kf->ncomp, prime2});
        }
        if (c->desc.average.n_items == 0) { c->desc.average = fy_average_desc{}; }      // (every field switched off: nothing is averaged)
    }
    return FY_OK;
}

int read_controls(fy_foam_case* c) {
    FoamDict control_dict;
    {
        const std::string path = join(c->dir, "system/controlDict");
        FoamDict d;
        FY_TRY(need_file(path, &d));
        if (!d.scalar("deltaT", &c->desc.dt) || !(c->desc.dt > 0)) return fail(FY_ERR_INVALID, "%s: deltaT missing or not positive", path.c_str());
        if (!d.scalar("endTime", &c->end_time)) return fail(FY_ERR_INVALID, "%s: endTime missing", path.c_str());
        c->start_time = 0.0; c->start_name = "0";
        std::string from;
        if (d.word("startFrom", &from) && from != "startTime" && from != "latestTime" && from != "firstTime")
            return fail(FY_ERR_UNSUPPORTED, "%s: startFrom %s is not supported (startTime, firstTime, latestTime)", path.c_str(), from.c_str());
        if (from == "latestTime" || from == "firstTime") {
            // the time directories of the case: the entries of the case directory whose names read as numbers [OF-6 Time::findTimes]
            DIR* dd = opendir(c->fdir.c_str());
            if (!dd) return fail(FY_ERR_INVALID, "%s: cannot list %s", path.c_str(), c->fdir.c_str());
            bool any = false;
            while (struct dirent* de = readdir(dd)) {
                double t;
                struct stat st;
                if (!fy::foam_tok_is_number(de->d_name, &t) || stat(join(c->fdir, de->d_name).c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) continue;
                if (!any || (from == "latestTime" ? t > c->start_time : t < c->start_time)) { c->start_time = t; c->start_name = de->d_name; }
                any = true;
            }
            closedir(dd);
            if (!any) return fail(FY_ERR_INVALID, "%s: startFrom %s: the case holds no time directory", path.c_str(), from.c_str());
        } else if (d.word("startTime", &c->start_name)) d.scalar("startTime", &c->start_time);
        std::string wc = "timeStep";
        d.word("writeControl", &wc);
        double wi = 0;
        d.scalar("writeInterval", &wi);
        if (wc == "timeStep") c->write_interval_steps = (int)wi;
        else if (wc == "runTime" || wc == "adjustableRunTime") c->write_interval_steps = (int)std::llround(wi / c->desc.dt);
        else return fail(FY_ERR_UNSUPPORTED, "%s: writeControl %s is not supported (timeStep, runTime, adjustableRunTime)", path.c_str(), wc.c_str());
        std::string wf = "ascii";
        if (d.word("writeFormat", &wf) && wf != "ascii" && wf != "binary") return fail(FY_ERR_INVALID, "%s: writeFormat %s (ascii or binary)", path.c_str(), wf.c_str());
        c->write_binary = wf == "binary";
        std::string comp;
        if (d.word("writeCompression", &comp) && comp != "off" && comp != "no" && comp != "false" && comp != "none" && comp != "uncompressed")
            return fail(FY_ERR_UNSUPPORTED, "%s: writeCompression %s is not supported (off)", path.c_str(), comp.c_str());
        double wp = 0, pw = 0;
        if (d.scalar("writePrecision", &wp)) { if (!(wp >= 1 && wp <= 17)) return fail(FY_ERR_INVALID, "%s: writePrecision %g", path.c_str(), wp); c->write_precision = (int)wp; }
        if (d.scalar("purgeWrite", &pw)) { if (pw < 0) return fail(FY_ERR_INVALID, "%s: purgeWrite %g", path.c_str(), pw); c->purge_write = (int)pw; }
        // readTimeControls.H [OF-6]: adjustTimeStep (default no), maxCo (default 1), maxDeltaT (default great).  Only pimpleFoamYade
        // includes setDeltaT.H (pimpleFoamYade.C:62-64); icoFoamYade's loop (icoFoamYade.C:65-70) never reads the switch, so there it is
        // ignored exactly as the reference ignores it
        bool adj = false;
        if (d.boolean("adjustTimeStep", &adj) && adj && c->solver == FY_SOLVER_PIMPLE) {
            if (wc != "timeStep") return fail(FY_ERR_UNSUPPORTED, "%s: adjustTimeStep with writeControl %s (output times that cut the time step) is not supported; use writeControl timeStep", path.c_str(), wc.c_str());
            c->desc.adjust_time_step = 1;
            c->desc.max_co = 1.0; c->desc.max_delta_t = 1e300;
            d.scalar("maxCo", &c->desc.max_co);
            d.scalar("maxDeltaT", &c->desc.max_delta_t);
        }
        control_dict = d;
    }
    {
        const std::string path = join(c->dir, "constant/transportProperties");
        FoamDict d;
        FY_TRY(need_file(path, &d));
        if (!d.scalar("nu", &c->desc.nu)) return fail(FY_ERR_INVALID, "%s: nu missing (createFields.H: transportProperties.lookup(\"nu\"))", path.c_str());
        if (!d.scalar("partDensity", &c->desc.rho_particle)) return fail(FY_ERR_INVALID, "%s: partDensity missing (createFields.H)", path.c_str());
        c->phase.clear();
        c->u_name = "U";
        if (c->solver == FY_SOLVER_PIMPLE) {
            // pimpleFoamYade/createFields.H:3-15,91-99: continuousPhaseName and rho.<phase>
            if (!d.word("continuousPhaseName", &c->phase)) return fail(FY_ERR_INVALID, "%s: continuousPhaseName missing (pimpleFoamYade/createFields.H:3-15)", path.c_str());
            c->u_name = "U." + c->phase;
            if (!d.scalar("rho." + c->phase, &c->desc.rho_fluid)) return fail(FY_ERR_INVALID, "%s: rho.%s missing (pimpleFoamYade/createFields.H:91-99)", path.c_str(), c->phase.c_str());
        } else {
            if (!d.scalar("fluidDensity", &c->desc.rho_fluid)) return fail(FY_ERR_INVALID, "%s: fluidDensity missing (icoFoamYade/createFields.H:41-46)", path.c_str());
        }
    }
    {
        const std::string path = join(c->dir, "constant/g");
        FoamDict d;
        FY_TRY(need_file(path, &d));          // readGravitationalAcceleration.H (createFields.H:1 of both solvers)
        if (!d.vector3("value", c->desc.g)) return fail(FY_ERR_INVALID, "%s: 'value (gx gy gz)' missing", path.c_str());
    }
    FY_TRY(read_coupling_properties(c));
    if (c->solver == FY_SOLVER_PIMPLE) {
        // continuousPhaseTurbulence (pimpleFoamYade/createFields.H): PhaseIncompressibleTurbulenceModel::New reads
        // constant/turbulenceProperties.<phase> [OF-6: IOobject::groupName(turbulenceModel::propertiesName, U.group())]; the plain name is
        // accepted too, and a case without the file runs the laminar model (the reference would stop).  DPMTurbulenceModels.C:67-77
        // instantiates laminar Stokes, RAS kEpsilon, LES Smagorinsky and LES kEqn; Stokes and Smagorinsky are implemented.
        std::string path = join(c->dir, "constant/turbulenceProperties." + c->phase);
        FoamDict d;
        bool have = file_exists(path);
        if (!have) { path = join(c->dir, "constant/turbulenceProperties"); have = file_exists(path); }
        if (have) {
            FY_TRY(need_file(path, &d));
            std::string sim;
            if (!d.word("simulationType", &sim)) return fail(FY_ERR_INVALID, "%s: simulationType missing", path.c_str());
            if (sim == "laminar") {
                std::string lm;
                const FoamDict* ld = d.subdict("laminar");
                if (ld && ld->word("laminarModel", &lm) && lm != "Stokes") return fail(FY_ERR_UNSUPPORTED, "%s: laminarModel %s (DPMTurbulenceModels.C:67-68 instantiates Stokes only)", path.c_str(), lm.c_str());
            } else if (sim == "LES") {
                const FoamDict* ld = d.subdict("LES");
                std::string model, delta;
                if (!ld || !ld->word("LESModel", &model)) return fail(FY_ERR_INVALID, "%s: LES { LESModel ...; } missing", path.c_str());
                if (model != "Smagorinsky" && model != "kEqn") return fail(FY_ERR_UNSUPPORTED, "%s: LESModel %s is not implemented (DPMTurbulenceModels.C:73-77 instantiates Smagorinsky and kEqn; both are)", path.c_str(), model.c_str());
                bool on = true;
                if (ld->boolean("turbulence", &on) && !on) return fail(FY_ERR_UNSUPPORTED, "%s: 'turbulence off' (frozen nut) is not supported: use simulationType laminar", path.c_str());
                if (!ld->word("delta", &delta) || delta != "cubeRootVol") return fail(FY_ERR_UNSUPPORTED, "%s: LES delta must be cubeRootVol (got '%s')", path.c_str(), delta.c_str());
                c->desc.turbulence_model = model == "kEqn" ? FY_TURBULENCE_KEQN : FY_TURBULENCE_SMAGORINSKY;
                if (const FoamDict* sc = ld->subdict(model + "Coeffs")) { sc->scalar("Ck", &c->desc.les_ck); sc->scalar("Ce", &c->desc.les_ce); }
                if (const FoamDict* dc = ld->subdict("cubeRootVolCoeffs")) dc->scalar("deltaCoeff", &c->desc.les_delta_coeff);
            } else if (sim == "RAS") {
                const FoamDict* rd = d.subdict("RAS");
                std::string model;
                if (!rd || !rd->word("RASModel", &model)) return fail(FY_ERR_INVALID, "%s: RAS { RASModel ...; } missing", path.c_str());
                if (model != "kEpsilon") return fail(FY_ERR_UNSUPPORTED, "%s: RASModel %s is not implemented (DPMTurbulenceModels.C:70-71 instantiates kEpsilon only)", path.c_str(), model.c_str());
                bool on = true;
                if (rd->boolean("turbulence", &on) && !on) return fail(FY_ERR_UNSUPPORTED, "%s: 'turbulence off' (frozen nut) is not supported: use simulationType laminar", path.c_str());
                c->desc.turbulence_model = FY_TURBULENCE_KEPSILON;
                if (const FoamDict* kc = rd->subdict("kEpsilonCoeffs")) {
                    kc->scalar("Cmu", &c->desc.ras_cmu); kc->scalar("C1", &c->desc.ras_c1); kc->scalar("C2", &c->desc.ras_c2); kc->scalar("C3", &c->desc.ras_c3);
                    kc->scalar("sigmak", &c->desc.ras_sigmak); kc->scalar("sigmaEps", &c->desc.ras_sigmaeps);
                }
            } else {
                return fail(FY_ERR_UNSUPPORTED, "%s: simulationType %s is not one of laminar, RAS, LES", path.c_str(), sim.c_str());
            }
        }
    }
    {
        // the discretisation is fixed in this library (Euler ddt, Gauss linear grad / div / laplacian, linear
        // interpolation, orthogonal snGrad): a case that asks for anything else would be silently mis-solved, so it is refused
        const std::string path = join(c->dir, "system/fvSchemes");
        FoamDict d;
        FY_TRY(need_file(path, &d));
        struct Want { const char* dict; const char* must; const char* alt; const char* forbid; };
        const Want wants[] = {{"ddtSchemes", "Euler", nullptr, nullptr},
                              {"gradSchemes", "linear", nullptr, "Limited"},
                              {"divSchemes", "linear", "upwind", "UpwindV"},         // parsed by name below: Gauss linear | upwind | linearUpwind grad(U) | the limited schemes; not the V variants
                              {"laplacianSchemes", "linear", nullptr, nullptr},
                              {"interpolationSchemes", "linear", nullptr, "pwind"},
                              {"snGradSchemes", "corrected", "orthogonal", nullptr}};   // corrected == uncorrected == orthogonal on this mesh
        int n_div = 0;
        bool t_div_named = false, t_div_default = false;      // div(phi,T) | div(alphaPhic,T) given by name; a usable `default`
        for (const Want& w : wants) {
            const FoamDict* sd = d.subdict(w.dict);
            if (!sd) return fail(FY_ERR_INVALID, "%s: %s missing", path.c_str(), w.dict);
            for (const std::string& k : sd->order) {
                const auto* tk = sd->tokens(k);
                if (!tk) continue;
                std::string joined;
                for (const std::string& t : *tk) joined += t + " ";
                const bool is_div = std::string(w.dict) == "divSchemes";
                // divSchemes: [bounded] Gauss <scheme> [args]; the scheme by name
                int sch = -1;
                double lim_k = 1.0;
                if (is_div && joined.find("none") != 0) {
                    size_t q = 0;
                    if (q < tk->size() && (*tk)[q] == "bounded") ++q;
                    if (q + 1 < tk->size() && (*tk)[q] == "Gauss") {
                        const std::string& nm = (*tk)[q + 1];
                        static const struct { const char* name; int id; } known[] = {
                            {"linear", FY_CONVECTION_LINEAR}, {"upwind", FY_CONVECTION_UPWIND}, {"linearUpwind", FY_CONVECTION_LINEAR_UPWIND},
                            {"limitedLinear", FY_CONVECTION_LIMITED_LINEAR}, {"vanLeer", FY_CONVECTION_VAN_LEER}, {"MUSCL", FY_CONVECTION_MUSCL},
                            {"Minmod", FY_CONVECTION_MINMOD}, {"SuperBee", FY_CONVECTION_SUPERBEE}, {"QUICK", FY_CONVECTION_QUICK}};
                        for (const auto& e : known) if (nm == e.name) sch = e.id;
                        if (sch == FY_CONVECTION_LIMITED_LINEAR && !(q + 2 < tk->size() && fy::foam_tok_is_number((*tk)[q + 2], &lim_k) && lim_k >= 0 && lim_k <= 1))
                            return fail(FY_ERR_INVALID, "%s: divSchemes.%s = '%s': limitedLinear takes a coefficient in [0, 1]", path.c_str(), k.c_str(), joined.c_str());
                    }
                }
                const bool ok = is_div ? (sch >= 0 || joined.find("none") == 0)
                              : ((joined.find(w.must) != std::string::npos || (w.alt && joined.find(w.alt) != std::string::npos) || joined.find("none") == 0) &&
                                 !(w.forbid && joined.find(w.forbid) != std::string::npos) && joined.find("limited") == std::string::npos &&
                                 joined.find("vanLeer") == std::string::npos && joined.find("QUICK") == std::string::npos);
                if (!ok) return fail(FY_ERR_UNSUPPORTED, "%s: %s.%s = '%s' is not supported (Euler; Gauss linear; div(phi,U) Gauss linear | upwind | linearUpwind | limitedLinear k | vanLeer | MUSCL | Minmod | SuperBee | QUICK)", path.c_str(), w.dict, k.c_str(), joined.c_str());
                if (is_div && joined.find("none") != 0) {
                    // only the convection terms select the scheme (icoFoamYade.C:82 div(phi,U), UcEqn.H:5-6 div(alphaPhic,Uc), or `default`);
                    // every other entry (the explicit stress term div(((alpha*nuEff)*dev2(T(grad(U))))) ...) must be plain Gauss linear
                    // (the fields' registered names are alphaPhi.<phase>, U.<phase>, k.<phase>: pimpleFoamYade/createFields.H:35-45,238-246)
                    const bool ico_term = k == "div(phi,U)";
                    const bool pimple_term = k == "div(alphaPhic,Uc)" || k == "div(phic,Uc)" || k == "div(alphaPhi." + c->phase + ",U." + c->phase + ")";
                    if ((ico_term && c->solver != FY_SOLVER_ICO) || (pimple_term && c->solver != FY_SOLVER_PIMPLE)) continue;      // (the other executable's term)
                    const bool convection = k == "default" || ico_term || pimple_term;
                    const bool k_convection = k == "div(alphaPhic,k)" || k == "div(alphaPhi." + c->phase + ",k." + c->phase + ")";
                    if (k == "div(alphaPhic,epsilon)" || k == "div(alphaPhi." + c->phase + ",epsilon." + c->phase + ")") {     // fvm::div(alphaRhoPhi, epsilon)
                        if (sch >= FY_CONVECTION_LINEAR_UPWIND) return fail(FY_ERR_UNSUPPORTED, "%s: divSchemes.%s = '%s': Gauss linear or Gauss upwind for epsilon", path.c_str(), k.c_str(), joined.c_str());
                        c->desc.eps_convection_scheme = sch;
                        continue;
                    }
                    if (k == "div(phi,T)" || k == "div(alphaPhic,T)" || k == "div(alphaPhi." + c->phase + ",T." + c->phase + ")") {      // the temperature equation's convection (heatTransfer)
                        if (sch >= FY_CONVECTION_LINEAR_UPWIND) return fail(FY_ERR_UNSUPPORTED, "%s: divSchemes.%s = '%s': [bounded] Gauss linear | upwind for T", path.c_str(), k.c_str(), joined.c_str());
                        if (c->desc.thermal.on) c->desc.thermal.T_convection_scheme = sch;
                        t_div_named = true;
                        continue;
                    }
                    if (k_convection) {                                  // fvm::div(alphaRhoPhi, k) of the kEqn / kEpsilon models
                        if (sch >= FY_CONVECTION_LINEAR_UPWIND) return fail(FY_ERR_UNSUPPORTED, "%s: divSchemes.%s = '%s': Gauss linear or Gauss upwind for k", path.c_str(), k.c_str(), joined.c_str());
                        c->desc.k_convection_scheme = sch;
                        continue;
                    }
                    if (!convection) {
                        if (sch != FY_CONVECTION_LINEAR) return fail(FY_ERR_UNSUPPORTED, "%s: divSchemes.%s = '%s': only the convection terms may be upwinded, this one must be Gauss linear", path.c_str(), k.c_str(), joined.c_str());
                        continue;
                    }
                    if (k == "default") { if (!n_div) { c->desc.convection_scheme = sch; c->desc.convection_limiter_k = lim_k; } c->desc.k_convection_scheme = c->desc.eps_convection_scheme = sch == FY_CONVECTION_LINEAR ? sch : FY_CONVECTION_UPWIND; t_div_default = true; if (c->desc.thermal.on && !t_div_named) c->desc.thermal.T_convection_scheme = c->desc.k_convection_scheme; continue; }      // a named convection entry overrides it
                    if (n_div++ && sch != c->desc.convection_scheme) return fail(FY_ERR_UNSUPPORTED, "%s: divSchemes mixes different convection schemes", path.c_str());
                    c->desc.convection_scheme = sch;
                    c->desc.convection_limiter_k = lim_k;
                }
            }
        }
        if (c->desc.thermal.on && !t_div_named && !t_div_default)      // (`default none;` and no entry for T: OpenFOAM stops at the first fvm::div of T)
            return fail(FY_ERR_UNSUPPORTED, "%s: divSchemes has no entry for %s and `default none`, but constant/couplingProperties has heatTransfer active; accepted: [bounded] Gauss linear | upwind",
                        path.c_str(), c->solver == FY_SOLVER_PIMPLE ? "div(alphaPhic,T)" : "div(phi,T)");
    }
    {
        const std::string path = join(c->dir, "system/fvSolution");
        FoamDict d;
        FY_TRY(need_file(path, &d));
        const char* alg = c->solver == FY_SOLVER_PIMPLE ? "PIMPLE" : "PISO";
        const FoamDict* a = d.subdict(alg);
        if (!a) return fail(FY_ERR_INVALID, "%s: no %s dictionary", path.c_str(), alg);
        a->integer("nCorrectors", &c->desc.n_correctors);
        a->integer("nNonOrthogonalCorrectors", &c->desc.n_non_orth_correctors);
        a->integer("nOuterCorrectors", &c->desc.n_outer_correctors);
        bool mp;
        if (a->boolean("momentumPredictor", &mp)) c->desc.momentum_predictor = mp ? 1 : 0;
        a->integer("pRefCell", &c->desc.p_ref_cell);
        a->scalar("pRefValue", &c->desc.p_ref_value);
        const FoamDict* sv = d.subdict("solvers");
        if (!sv) return fail(FY_ERR_INVALID, "%s: no solvers dictionary", path.c_str());
        const FoamDict* ps = sv->subdict("p");
        if (!ps) return fail(FY_ERR_INVALID, "%s: solvers.p missing", path.c_str());
        ps->scalar("tolerance", &c->desc.p_tol); ps->scalar("relTol", &c->desc.p_rel_tol); ps->integer("maxIter", &c->desc.p_max_iter);
        std::string sname, pre;
        ps->word("solver", &sname); ps->word("preconditioner", &pre);
        c->desc.p_solver = (sname == "GAMG" || pre == "GAMG") ? FY_PSOLVER_PCG_MG : FY_PSOLVER_PCG_JACOBI;    // the two pressure solvers this library has
        c->desc.p_final_tol = c->desc.p_tol; c->desc.p_final_rel_tol = 0.0;
        if (const FoamDict* pf = sv->subdict("pFinal")) { pf->scalar("tolerance", &c->desc.p_final_tol); pf->scalar("relTol", &c->desc.p_final_rel_tol); }
        const FoamDict* us = sv->subdict(c->u_name);
        if (!us)
            for (const std::string& k : sv->order)
                if (k.find(c->u_name) != std::string::npos || (k.find("U") != std::string::npos && k.find("Final") == std::string::npos)) { us = sv->subdict(k); if (us) break; }
        if (us) { us->scalar("tolerance", &c->desc.u_tol); us->scalar("relTol", &c->desc.u_rel_tol); us->integer("maxIter", &c->desc.u_max_iter); }
        if (c->desc.turbulence_model == FY_TURBULENCE_KEPSILON) {      // solvers.epsilon.<phase> (or a pattern naming epsilon)
            c->desc.eps_tol = c->desc.u_tol; c->desc.eps_rel_tol = c->desc.u_rel_tol; c->desc.eps_max_iter = c->desc.u_max_iter;
            const std::string en = "epsilon." + c->phase;
            const FoamDict* es = sv->subdict(en);
            if (!es)
                for (const std::string& key : sv->order)
                    if (key.find("epsilon") != std::string::npos) { es = sv->subdict(key); if (es) break; }
            if (!es) return fail(FY_ERR_INVALID, "%s: solvers has no entry for %s (kEpsilon solves a transport equation for it)", path.c_str(), en.c_str());
            es->scalar("tolerance", &c->desc.eps_tol); es->scalar("relTol", &c->desc.eps_rel_tol); es->integer("maxIter", &c->desc.eps_max_iter);
        }
        if (c->desc.turbulence_model == FY_TURBULENCE_KEQN || c->desc.turbulence_model == FY_TURBULENCE_KEPSILON) {          // solvers.k.<phase> (or a pattern naming k, e.g. "(U.water|k.water)")
            c->desc.k_tol = c->desc.u_tol; c->desc.k_rel_tol = c->desc.u_rel_tol; c->desc.k_max_iter = c->desc.u_max_iter;
            const std::string kn = "k." + c->phase;
            const FoamDict* ks = sv->subdict(kn);
            if (!ks)
                for (const std::string& key : sv->order)
                    if (key.find(kn) != std::string::npos || key.find("|k|") != std::string::npos || key.find("|k)") != std::string::npos) { ks = sv->subdict(key); if (ks) break; }
            if (!ks) return fail(FY_ERR_INVALID, "%s: solvers has no entry for %s (kEqn solves a transport equation for it)", path.c_str(), kn.c_str());
            ks->scalar("tolerance", &c->desc.k_tol); ks->scalar("relTol", &c->desc.k_rel_tol); ks->integer("maxIter", &c->desc.k_max_iter);
        }
        if (c->desc.thermal.on) {                                      // solvers.T | T.<phase> (or a pattern naming it)
            const std::string tn = field_name(c, F_T);
            const FoamDict* ts = sv->subdict(tn);
            if (!ts) ts = sv->subdict("T");
            if (!ts)
                for (const std::string& key : sv->order)
                    if (key.find(tn) != std::string::npos || key.find("|T|") != std::string::npos || key.find("|T)") != std::string::npos || key.find("(T|") != std::string::npos) { ts = sv->subdict(key); if (ts) break; }
            if (!ts) return fail(FY_ERR_UNSUPPORTED, "%s: solvers has no entry for %s, but constant/couplingProperties has heatTransfer active (tolerance, relTol, maxIter of the Jacobi solve)", path.c_str(), tn.c_str());
            c->desc.thermal.T_tol = c->desc.u_tol; c->desc.thermal.T_rel_tol = c->desc.u_rel_tol; c->desc.thermal.T_max_iter = c->desc.u_max_iter;
            ts->scalar("tolerance", &c->desc.thermal.T_tol); ts->scalar("relTol", &c->desc.thermal.T_rel_tol); ts->integer("maxIter", &c->desc.thermal.T_max_iter);
        }
        // relaxationFactors: equations { <U>; <U>Final; ".*" } for UcEqn.relax() (UcEqn.H:12), fields { p; pFinal } for p.relax() (pEqn.H:41).
        // No entry = the call does nothing [OF-6 fvMatrix::relax(), GeometricField::relax()]; icoFoamYade relaxes nothing.
        c->desc.u_relax = c->desc.u_relax_final = c->desc.p_relax = c->desc.p_relax_final = 0.0;
        if (const FoamDict* rf = d.subdict("relaxationFactors")) {
            if (c->solver == FY_SOLVER_PIMPLE) {
                auto lookup = [&](const FoamDict* sd, const std::string& name, double* out) {
                    if (!sd) return;
                    double v = 0;
                    if (sd->scalar(name, &v) || sd->scalar("\"" + name + "\"", &v)) { *out = v; return; }
                    for (const std::string& k : sd->order) {            // the catch-all patterns the tutorials use
                        const bool any = k == "\".*\"" || k == ".*" || k == "\"(.*)\"";
                        const bool fin = k == "\".*Final\"" || k == "\"(.*)Final\"";
                        const bool is_final = name.size() > 5 && name.compare(name.size() - 5, 5, "Final") == 0;
                        if ((fin && is_final) || (any && sd->scalar(k, &v))) { if (sd->scalar(k, &v)) *out = v; }
                    }
                };
                lookup(rf->subdict("equations"), c->u_name, &c->desc.u_relax);
                lookup(rf->subdict("equations"), c->u_name + "Final", &c->desc.u_relax_final);
                if (c->desc.turbulence_model == FY_TURBULENCE_KEQN || c->desc.turbulence_model == FY_TURBULENCE_KEPSILON) lookup(rf->subdict("equations"), "k." + c->phase, &c->desc.k_relax);
                if (c->desc.turbulence_model == FY_TURBULENCE_KEPSILON) lookup(rf->subdict("equations"), "epsilon." + c->phase, &c->desc.eps_relax);
                lookup(rf->subdict("fields"), "p", &c->desc.p_relax);
                lookup(rf->subdict("fields"), "pFinal", &c->desc.p_relax_final);
                for (double v : {c->desc.u_relax, c->desc.u_relax_final, c->desc.p_relax, c->desc.p_relax_final})
                    if (v > 1.0) return fail(FY_ERR_INVALID, "%s: relaxationFactors above 1", path.c_str());
            }
        }
    }
    return read_functions(c, control_dict, join(c->dir, "system/controlDict"));
}

// An inlet patch in a written time directory keeps its entry as read -- type, function dictionary -- with `value` as the faces' current values (u_boundary_now: the
// solver's "U_boundary"), in the patch's own face order, so that a run restarted from the directory continues the function at its own time.  false: not an inlet patch,
// or no solver behind the write (fy_foam_case_write_fields: the entry as read)
bool inlet_entry(const fy_foam_case* c, const std::string& pn, const std::string& as_read, std::string* text) {
    if (c->u_boundary_now.empty()) return false;
    const std::vector<double>& ub = c->u_boundary_now;
    std::vector<double> v;
    bool inlet = false;
    if (c->general) {
        std::vector<int> with_value;                          // the inlet patches, and the open ones (inletOutlet, pressureInletOutletVelocity): the faces' values as they are now
        for (const auto& in : c->inlets) with_value.push_back(in.patch);
        for (size_t q = 0; q < c->bcs[F_U].bc.size(); ++q) if (c->bcs[F_U].bc[q] >= FY_BC_U_INLET_OUTLET) with_value.push_back((int)q);
        for (int pa : with_value) if (c->g_patch_name[(size_t)pa] == pn) {
            inlet = true;
            const size_t b0 = (size_t)(c->g_patch_start[(size_t)pa] - c->g_internal), n = (size_t)c->g_patch_size[(size_t)pa];
            if (3 * (b0 + n) > ub.size()) return false;
            v.assign(ub.begin() + 3 * b0, ub.begin() + 3 * (b0 + n));
        }
    } else {
        for (const auto& in : c->inlets) inlet = inlet || c->patch_of_side[in.patch] == pn;
        if (!inlet) return false;
        size_t total = 0, base = 0;
        for (int s = 0; s < 6; ++s) if (c->patch_of_side[s] == pn) total += side_size(c, s);
        v.assign(3 * total, 0.0);
        for (int s = 0; s < 6; ++s) {
            const size_t n = side_size(c, s);
            if (c->patch_of_side[s] == pn)
                for (size_t r = 0; r < n; ++r) {
                    const size_t at = c->side_face_src[s].empty() ? r : (size_t)c->side_face_src[s][r];      // (blockMeshDict alone: a one-side patch in the side's own order)
                    if (at < total && 3 * (base + r) + 2 < ub.size()) for (int q = 0; q < 3; ++q) v[3 * at + q] = ub[3 * (base + r) + q];
                }
            base += n;
        }
    }
    if (!inlet) return false;
    text->clear();
    size_t pos = 0;
    while (pos < as_read.size()) {                            // the entry as read, line by line, without its value
        const size_t e = as_read.find(";\n", pos);
        const size_t end = e == std::string::npos ? as_read.size() : e + 2;
        if (as_read.compare(pos, 14, "        value ") != 0) text->append(as_read, pos, end - pos);
        pos = end;
    }
    char buf[128];
    std::snprintf(buf, sizeof(buf), "        value           nonuniform List<vector> %zu", v.size() / 3);
    *text += buf;
    if (c->write_binary) {
        *text += "(";
        text->append((const char*)v.data(), v.size() * sizeof(double));
        *text += ");\n";
    } else {
        *text += "\n(\n";
        for (size_t q = 0; q + 2 < v.size(); q += 3) { std::snprintf(buf, sizeof(buf), "(%.*g %.*g %.*g)\n", c->write_precision, v[q], c->write_precision, v[q + 1], c->write_precision, v[q + 2]); *text += buf; }
        *text += ");\n";
    }
    return true;
}

int write_field(const fy_foam_case* c, const std::string& tdir, const std::string& tname, const std::string& name, const char* cls, const char* dims, int ncomp,
                const std::vector<double>& v, const PatchField* bcs, const char* default_bc, const std::vector<std::pair<std::string, std::string> >& extras) {
    const std::string path = tdir + "/" + name;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return fail(FY_ERR_INVALID, "cannot write %s", path.c_str());
    const size_t n = v.size() / (size_t)ncomp;
    std::fprintf(f, "FoamFile\n{\n    version     2.0;\n    format      %s;\n", c->write_binary ? "binary" : "ascii");
    if (c->write_binary) std::fprintf(f, "    arch        \"LSB;label=32;scalar=64\";\n");
    std::fprintf(f, "    class       %s;\n    location    \"%s\";\n    object      %s;\n}\n\n", cls, tname.c_str(), name.c_str());
    std::fprintf(f, "dimensions      %s;\n\ninternalField   nonuniform List<%s> %zu\n(", dims, ncomp == 6 ? "symmTensor" : ncomp == 3 ? "vector" : "scalar", n);
    std::vector<double> vf;                                // lattice order -> the mesh's cell numbers
    if (!c->file_cell.empty() && n == c->file_cell.size()) {
        vf.resize(v.size());
        for (size_t L = 0; L < n; ++L) for (int q = 0; q < ncomp; ++q) vf[(size_t)c->file_cell[L] * ncomp + q] = v[L * ncomp + q];
    }
    const std::vector<double>& v_out = vf.empty() ? v : vf;
    if (c->write_binary) {
        // the list's values as they lie in memory, between the parentheses [OF-6 UList<T>::writeEntry, binary stream]
        if (std::fwrite(v_out.data(), sizeof(double), v_out.size(), f) != v_out.size()) { std::fclose(f); return fail(FY_ERR_INVALID, "cannot write %s", path.c_str()); }
    } else {
        const int pr = c->write_precision;
        std::fputc('\n', f);
        for (size_t q = 0; q < n; ++q) {
            if (ncomp == 3) std::fprintf(f, "(%.*g %.*g %.*g)\n", pr, v_out[3 * q], pr, v_out[3 * q + 1], pr, v_out[3 * q + 2]);
            else if (ncomp == 6) std::fprintf(f, "(%.*g %.*g %.*g %.*g %.*g %.*g)\n", pr, v_out[6 * q], pr, v_out[6 * q + 1], pr, v_out[6 * q + 2], pr, v_out[6 * q + 3], pr, v_out[6 * q + 4], pr, v_out[6 * q + 5]);
            else std::fprintf(f, "%.*g\n", pr, v_out[q]);
        }
    }
    std::fprintf(f, ")\n;\n\nboundaryField\n{\n");
    // every patch in the mesh's order with its entry as read (a field without a start-time file -- alpha -- or without an entry: default_bc)
    const std::vector<std::string> names = field_patches(c);
    for (const std::string& pn : c->patch_order) {
        size_t pa = names.size();
        for (size_t q = 0; q < names.size(); ++q) if (names[q] == pn) pa = q;
        const bool known = bcs && pa < bcs->text.size() && !bcs->text[pa].empty();
        std::string inlet_text;
        if (known && bcs == &c->bcs[F_U] && inlet_entry(c, pn, bcs->text[pa], &inlet_text)) {
            std::fprintf(f, "    %s\n    {\n", pn.c_str());
            std::fwrite(inlet_text.data(), 1, inlet_text.size(), f);      // (a binary list: not a C string)
            std::fprintf(f, "    }\n");
            continue;
        }
        std::fprintf(f, "    %s\n    {\n%s    }\n", pn.c_str(), known ? bcs->text[pa].c_str() : default_bc);
    }
    // a decomposed case's processor patches, as the start time's file had them (fields without a start-time file: those of U, type only)
    for (const auto& e : extras) std::fprintf(f, "    %s\n    {\n%s    }\n", e.first.c_str(), e.second.c_str());
    std::fprintf(f, "}\n");
    std::fclose(f);
    return FY_OK;
}

// the fields the case has, read from a solver (read(name, host) in the given order: it decides which field a solver of another model is first missing) and written
template <class Read>
int write_solver_fields(const fy_foam_case* c, const char* time_name, std::initializer_list<int> order, Read read) {
    static const char* const solver_name[] = {"U", "p", "nut", "k", "epsilon", "alpha"};
    std::vector<double> v[6];
    for (int F : order)
        if (has_field(c, F)) { v[F].resize((F == F_U ? 3 : 1) * c->fcells); FY_TRY(read(solver_name[F], v[F].data())); }
    auto ptr = [&](int F) { return v[F].empty() ? nullptr : v[F].data(); };
    return fy_foam_case_write_fields(c, time_name, ptr(F_U), ptr(F_P), ptr(F_ALPHA), ptr(F_NUT), ptr(F_K), ptr(F_EPS));
}

// the dimension sets of the case's fields, and their squares for prime2Mean
const int* field_dims(int F, const std::string& solver_name) {
    static const int U[7] = {0, 1, -1, 0, 0, 0, 0}, p[7] = {0, 2, -2, 0, 0, 0, 0}, none[7] = {0, 0, 0, 0, 0, 0, 0}, nut[7] = {0, 2, -1, 0, 0, 0, 0}, eps[7] = {0, 2, -3, 0, 0, 0, 0},
                     acc[7] = {0, 1, -2, 0, 0, 0, 0};
    switch (F) {
        case F_U: return U;
        case F_P: case F_K: return p;
        case F_NUT: return nut;
        case F_EPS: return eps;
        case F_ALPHA: return none;
        case F_T: { static const int temp[7] = {0, 0, 0, 1, 0, 0, 0}; return temp; }
        default: {                                                // volSource, uParticle (createFields.H of both solvers); the solid statistics' fields
            static const int perVol[7] = {0, -3, 0, 0, 0, 0, 0}, len[7] = {0, 1, 0, 0, 0, 0, 0}, temp[7] = {0, 0, 0, 1, 0, 0, 0};
            if (solver_name == "nParticle") return perVol;
            if (solver_name == "solidFraction") return none;
            if (solver_name == "granularTemperature") return p;
            if (solver_name == "dSauter") return len;
            if (solver_name == "TParticle") return temp;
            return solver_name == "uSource" ? acc : U;
        }
    }
}
std::string dims_text(const int* d, int power) {
    std::string t = "[";
    for (int q = 0; q < 7; ++q) t += std::to_string(power * d[q]) + (q < 6 ? " " : "]");
    return t;
}

// the solid statistics' part of runTime.write(), when the solver forms them (count(name, &n) succeeds): nParticle, solidFraction, uSolid, granularTemperature, dSauter
// and, with heat transfer, TParticle -- patches `calculated`, as <field>Prime2Mean is written
template <class Count, class Read>
int write_solid_stats(const fy_foam_case* c, const char* time_name, Count count, Read read) {
    static const struct { const char* name; int ncomp; const char* dims; } fields[] = {
        {"nParticle", 1, "[0 -3 0 0 0 0 0]"}, {"solidFraction", 1, "[0 0 0 0 0 0 0]"}, {"uSolid", 3, "[0 1 -1 0 0 0 0]"},
        {"granularTemperature", 1, "[0 2 -2 0 0 0 0]"}, {"dSauter", 1, "[0 1 0 0 0 0 0]"}, {"TParticle", 1, "[0 0 0 1 0 0 0]"}};
    const std::vector<std::pair<std::string, std::string> > none;
    for (const auto& f : fields) {
        int64_t n = 0;
        if (count(f.name, &n) != FY_OK || (size_t)n != c->fcells * (size_t)f.ncomp) continue;      // statistics off on this solver, or (TParticle) no heat transfer
        std::vector<double> v((size_t)n);
        FY_TRY(read(f.name, v.data()));
        FY_TRY(write_field(c, join(c->fdir, time_name), time_name, f.name, f.ncomp == 3 ? "volVectorField" : "volScalarField", f.dims, f.ncomp, v, nullptr,
                           f.ncomp == 3 ? "        type            calculated;\n        value           uniform (0 0 0);\n" : "        type            calculated;\n        value           uniform 0;\n", none));
    }
    return FY_OK;
}

// fieldAverage's part of runTime.write(): the case's object, when the solver averages its fields (a solver made from this case's descriptor: item i = avg_fields[i]).
// count(name, &n) / read(name, host) / state(i, &N, &T) are the solver's accessors; dt the deltaT of the step just finished
template <class Count, class Read, class State>
int write_averages(const fy_foam_case* c, const char* time_name, double dt, Count count, Read read, State state) {
    if (c->avg_fields.empty()) return FY_OK;
    for (const auto& a : c->avg_fields) {             // averaging off on this solver (or other items than the case's): nothing beyond the fields
        int64_t n = 0;
        if (count((a.solver_name + "Mean").c_str(), &n) != FY_OK || (size_t)n != c->fcells * (size_t)a.ncomp) return FY_OK;
        if (a.prime2 && count((a.solver_name + "Prime2Mean").c_str(), &n) != FY_OK) return FY_OK;
    }
    const std::string tdir = join(c->fdir, time_name);
    const std::vector<std::pair<std::string, std::string> > none;
    std::string props = "FoamFile\n{\n    version     2.0;\n    format      ascii;\n    class       dictionary;\n    location    \"" + std::string(time_name) + "/uniform\";\n    object      " +
                        c->avg_name + "Properties;\n}\n\n";
    for (size_t i = 0; i < c->avg_fields.size(); ++i) {
        const auto& a = c->avg_fields[i];
        const int* dims = field_dims(a.F, a.solver_name);
        std::vector<double> v(c->fcells * (size_t)a.ncomp);
        FY_TRY(read((a.solver_name + "Mean").c_str(), v.data()));
        const PatchField* r = a.F >= 0 && a.F != F_ALPHA ? &c->bcs[a.F] : nullptr;
        FY_TRY(write_field(c, tdir, time_name, a.file + "Mean", a.ncomp == 3 ? "volVectorField" : "volScalarField", dims_text(dims, 1).c_str(), a.ncomp, v, r,
                           "        type            zeroGradient;\n", r ? r->extra : none));
        if (a.prime2) {
            const int pc = a.ncomp == 3 ? 6 : 1;
            v.assign(c->fcells * (size_t)pc, 0.0);
            FY_TRY(read((a.solver_name + "Prime2Mean").c_str(), v.data()));
            FY_TRY(write_field(c, tdir, time_name, a.file + "Prime2Mean", pc == 6 ? "volSymmTensorField" : "volScalarField", dims_text(dims, 2).c_str(), pc, v, nullptr,
                               pc == 6 ? "        type            calculated;\n        value           uniform (0 0 0 0 0 0);\n" : "        type            calculated;\n        value           uniform 0;\n", none));
        }
        int64_t N = 0; double T = 0.0;
        FY_TRY(state((int)i, &N, &T));
        // totalIter / totalTime: OpenFOAM's convention as recalled (N + 1, T + deltaT; unpinned); samples / timeAveraged: this library's own N and T,
        // written with 17 digits so that a restart continues exactly (T + deltaT - deltaT need not give T back)
        char buf[512];
        std::snprintf(buf, sizeof(buf), "%s\n{\n    totalIter       %lld;\n    totalTime       %.17g;\n    samples         %lld;\n    timeAveraged    %.17g;\n}\n\n", a.file.c_str(),
                      (long long)(N + 1), T + dt, (long long)N, T);
        props += buf;
    }
    const std::string udir = join(tdir, "uniform");
    if (mkdir(udir.c_str(), 0777) != 0) {
        struct stat st;
        if (stat(udir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) return fail(FY_ERR_INVALID, "cannot create %s", udir.c_str());
    }
    const std::string ppath = join(udir, c->avg_name + "Properties");
    FILE* f = std::fopen(ppath.c_str(), "wb");
    if (!f) return fail(FY_ERR_INVALID, "cannot write %s", ppath.c_str());
    std::fputs(props.c_str(), f);
    std::fclose(f);
    return FY_OK;
}

// the start time directory's averages -> a new solver: per item, when the Properties file has its entry and its mean (and prime2Mean) file is there
template <class Write, class SetState>
int restore_averages(const fy_foam_case* c, double dt, int* restored, Write write, SetState set_state) {
    if (restored) *restored = 0;
    if (c->avg_fields.empty() || c->avg_restart_on_restart) return FY_OK;
    const std::string sdir = join(c->fdir, c->start_name);
    const std::string ppath = join(sdir, "uniform/" + c->avg_name + "Properties");
    if (!file_exists(ppath)) return FY_OK;
    FoamDict props;
    FY_TRY(need_file(ppath, &props));
    for (size_t i = 0; i < c->avg_fields.size(); ++i) {
        const auto& a = c->avg_fields[i];
        const FoamDict* pd = props.subdict(a.file);
        const std::string mpath = join(sdir, a.file + "Mean"), qpath = join(sdir, a.file + "Prime2Mean");
        if (!pd || !file_exists(mpath) || (a.prime2 && !file_exists(qpath))) continue;
        double N = 0, T = 0;
        if (!(pd->scalar("samples", &N) && pd->scalar("timeAveraged", &T))) {      // a directory OpenFOAM wrote: its convention, inverted
            if (!pd->scalar("totalIter", &N) || !pd->scalar("totalTime", &T)) return fail(FY_ERR_INVALID, "%s: %s needs totalIter and totalTime", ppath.c_str(), a.file.c_str());
            N -= 1; T -= dt;
        }
        if (N < 0 || T < 0) return fail(FY_ERR_INVALID, "%s: %s: totalIter / totalTime below one step", ppath.c_str(), a.file.c_str());
        std::vector<double> v;
        FoamDict mf;
        FY_TRY(need_file(mpath, &mf));
        FY_TRY(read_internal(mf, mpath, a.ncomp, c->fcells, &v, c->general ? nullptr : &c->file_cell));
        FY_TRY(write((a.solver_name + "Mean").c_str(), v.data()));
        if (a.prime2) {
            FoamDict qf;
            FY_TRY(need_file(qpath, &qf));
            FY_TRY(read_internal(qf, qpath, a.ncomp == 3 ? 6 : 1, c->fcells, &v, c->general ? nullptr : &c->file_cell));
            FY_TRY(write((a.solver_name + "Prime2Mean").c_str(), v.data()));
        }
        FY_TRY(set_state((int)i, (int64_t)std::llround(N), T));
        if (restored) ++*restored;
    }
    return FY_OK;
}

}  // namespace

namespace {
// The rows the solver's monitors have gathered since the last call -> postProcessing/<object>/<start time name>/volFieldValue.dat | surfaceFieldValue.dat (the layout of
// OpenFOAM-6's fieldValue files as recalled: '#' header lines, then one row per sample -- time, values, a vector as (x y z)).  measure(i, &n, &total): the object's
// number of cells / faces and their total volume / area
template <class Layout, class Rows, class Measure>
int write_monitors(const fy_foam_case* c, Layout layout, Rows rows, Measure measure) {
    for (size_t q = 0; q < c->monitors.size(); ++q) {
        const fy_foam_case::MonMeta& m = c->monitors[q];
        int32_t nv = 0;
        FY_TRY(layout((int)q, &nv));
        int64_t have = 0;
        FY_TRY(rows((int)q, m.rows_written, 0, nullptr, nullptr, &have));
        std::string dir = join(c->dir, "postProcessing");
        for (const std::string& part : {std::string(), m.name, c->start_name}) {
            if (!part.empty()) dir = join(dir, part);
            if (mkdir(dir.c_str(), 0777) != 0 && errno != EEXIST) return fail(FY_ERR_INVALID, "cannot create %s", dir.c_str());
        }
        const std::string path = join(dir, m.vol ? "volFieldValue.dat" : "surfaceFieldValue.dat");
        FILE* f = std::fopen(path.c_str(), m.rows_written == 0 ? "w" : "a");
        if (!f) return fail(FY_ERR_INVALID, "cannot write %s", path.c_str());
        const int pr = c->write_precision;
        if (m.rows_written == 0) {
            int64_t n = 0; double total = 0;
            const int rc = measure((int)q, &n, &total);
            if (rc != FY_OK) { std::fclose(f); return rc; }
            std::fprintf(f, "# Region type : %s%s\n", m.vol ? "all" : "patch ", m.vol ? "" : m.region.c_str());
            std::fprintf(f, "# %s       : %lld\n", m.vol ? "Cells" : "Faces", (long long)n);
            std::fprintf(f, "# %s      : %.*g\n", m.vol ? "Volume" : "Area  ", pr, total);
            std::fprintf(f, "# Time");
            for (const std::string& file : m.files) std::fprintf(f, "\t%s(%s)", monitor_op_word(c->desc.monitors.objects[q].operation), file.c_str());
            std::fprintf(f, "\n");
        }
        if (have > 0) {
            std::vector<double> t((size_t)have), v((size_t)have * (size_t)nv);
            int64_t got = 0;
            const int rc = rows((int)q, m.rows_written, have, t.data(), v.data(), &got);
            if (rc != FY_OK) { std::fclose(f); return rc; }
            for (int64_t r = 0; r < got; ++r) {
                std::fprintf(f, "%.*g", pr, t[(size_t)r]);
                const double* x = v.data() + (size_t)r * nv;
                for (int nc : m.ncomp) {
                    if (nc == 3) std::fprintf(f, "\t(%.*g %.*g %.*g)", pr, x[0], pr, x[1], pr, x[2]);
                    else std::fprintf(f, "\t%.*g", pr, x[0]);
                    x += nc;
                }
                std::fprintf(f, "\n");
            }
            m.rows_written += got;
        }
        if (std::fclose(f) != 0) return fail(FY_ERR_INVALID, "cannot write %s", path.c_str());
    }
    return FY_OK;
}

// The rows the solver's wall loads have gathered since the last call -> postProcessing/<object>/<start time name>/forces.dat | wallShearStress.dat | yPlus.dat (the
// layout of OpenFOAM-6's files as recalled, unpinned: '#' header lines, then per sample -- forces: time and the four vectors Fp Fv Mp Mv as (x y z); wallShearStress:
// one line per patch, time, patch, min vector, max vector; yPlus: one line per patch, time, patch, min, max, average)
template <class Layout, class Rows>
int write_wall_loads(const fy_foam_case* c, Layout layout, Rows rows) {
    const std::vector<const fy_foam_case::WlMeta*> metas = c->wall_loads();
    for (size_t q = 0; q < metas.size(); ++q) {
        const fy_foam_case::WlMeta& m = *metas[q];
        int32_t nv = 0;
        FY_TRY(layout((int)q, &nv));
        const int per = m.kind == 0 ? 12 : m.kind == 1 ? 6 : 3;
        if (nv != (m.kind == 0 ? 12 : per * (int)m.patches.size())) return fail(FY_ERR_INVALID, "fy_foam_case_write_wall_loads: object '%s' has %d values in the solver (was it created from this case?)", m.name.c_str(), nv);
        int64_t have = 0;
        FY_TRY(rows((int)q, m.rows_written, 0, nullptr, nullptr, &have));
        std::string dir = join(c->dir, "postProcessing");
        for (const std::string& part : {std::string(), m.name, c->start_name}) {
            if (!part.empty()) dir = join(dir, part);
            if (mkdir(dir.c_str(), 0777) != 0 && errno != EEXIST) return fail(FY_ERR_INVALID, "cannot create %s", dir.c_str());
        }
        const std::string path = join(dir, m.kind == 0 ? "forces.dat" : m.kind == 1 ? "wallShearStress.dat" : "yPlus.dat");
        FILE* f = std::fopen(path.c_str(), m.rows_written == 0 ? "w" : "a");
        if (!f) return fail(FY_ERR_INVALID, "cannot write %s", path.c_str());
        const int pr = c->write_precision;
        if (m.rows_written == 0) {
            if (m.kind == 0) {
                const fy_forces_object& fo = c->desc.wall_loads.forces[q];
                std::fprintf(f, "# Forces\n# CofR       : (%.*g %.*g %.*g)\n# rhoInf     : %.*g\n# pRef       : %.*g\n# patches    :", pr, fo.cofr[0], pr, fo.cofr[1], pr, fo.cofr[2], pr, fo.rho, pr, fo.p_ref);
                for (const std::string& pn : m.patches) std::fprintf(f, " %s", pn.c_str());
                std::fprintf(f, "\n# Time\tforces(pressure viscous)\tmoment(pressure viscous)\n");
            } else if (m.kind == 1) std::fprintf(f, "# Wall shear stress\n# Time\tpatch\tmin\tmax\n");
            else std::fprintf(f, "# y+ ()\n# Time\tpatch\tmin\tmax\taverage\n");
        }
        if (have > 0) {
            std::vector<double> t((size_t)have), v((size_t)have * (size_t)nv);
            int64_t got = 0;
            const int rc = rows((int)q, m.rows_written, have, t.data(), v.data(), &got);
            if (rc != FY_OK) { std::fclose(f); return rc; }
            for (int64_t r = 0; r < got; ++r) {
                const double* x = v.data() + (size_t)r * nv;
                if (m.kind == 0) {
                    std::fprintf(f, "%.*g", pr, t[(size_t)r]);
                    for (int g = 0; g < 4; ++g) std::fprintf(f, "\t(%.*g %.*g %.*g)", pr, x[3 * g], pr, x[3 * g + 1], pr, x[3 * g + 2]);
                    std::fprintf(f, "\n");
                    continue;
                }
                for (size_t p = 0; p < m.patches.size(); ++p, x += per) {
                    std::fprintf(f, "%.*g\t%s", pr, t[(size_t)r], m.patches[p].c_str());
                    if (m.kind == 1) std::fprintf(f, "\t(%.*g %.*g %.*g)\t(%.*g %.*g %.*g)\n", pr, x[0], pr, x[1], pr, x[2], pr, x[3], pr, x[4], pr, x[5]);
                    else std::fprintf(f, "\t%.*g\t%.*g\t%.*g\n", pr, x[0], pr, x[1], pr, x[2]);
                }
            }
            m.rows_written += got;
        }
        if (std::fclose(f) != 0) return fail(FY_ERR_INVALID, "cannot write %s", path.c_str());
    }
    return FY_OK;
}
}  // namespace

extern "C" {

static int open_case(const char* case_dir, int solver, int rank, int nranks, fy_foam_case** out) {
    if (!case_dir || !out) return fail(FY_ERR_INVALID, "fy_foam_case_open: null argument");
    if (solver != FY_SOLVER_ICO && solver != FY_SOLVER_PIMPLE) return fail(FY_ERR_INVALID, "fy_foam_case_open: solver must be FY_SOLVER_ICO or FY_SOLVER_PIMPLE");
    *out = nullptr;
    fy_foam_case* c = new (std::nothrow) fy_foam_case();
    if (!c) return fail(FY_ERR_INVALID, "out of host memory");
    c->dir = case_dir;
    c->fdir = c->dir;
    c->solver = solver;
    fy_case_defaults(&c->desc, solver);
    // the mesh: constant/polyMesh when the case has one (what the reference's solvers read), else system/blockMeshDict (what blockMesh would make of it)
    int rc = file_exists(join(c->dir, "constant/polyMesh/points")) ? read_poly_mesh(c) : read_block_mesh(c);
    if (rc == FY_ERR_UNSUPPORTED && file_exists(join(c->dir, "constant/polyMesh/points")) && file_exists(join(c->dir, "system/blockMeshDict"))) {
        // a polyMesh this reader does not take (binary, or not a lattice of hexahedra): the dictionary it was made from may still describe the block
        const std::string why = fy_last_error();
        *c = fy_foam_case();
        c->dir = case_dir; c->fdir = c->dir; c->solver = solver;
        fy_case_defaults(&c->desc, solver);
        rc = read_block_mesh(c);
        if (rc != FY_OK) rc = fail(rc, "%s (constant/polyMesh was refused first: %s)", std::string(fy_last_error()).c_str(), why.c_str());
    }
    if (rc == FY_OK) {
        c->fcells = (size_t)c->desc.nx * c->desc.ny * c->desc.nz;
        if (nranks > 0) {
            // processorR of a decomposed case = the R-th of nranks equal z-slabs (decomposePar, simple (1 1 N)), cells in the global order
            struct stat st;
            const std::string pd = join(c->dir, "processor" + std::to_string(rank));
            if (rank < 0 || rank >= nranks) rc = fail(FY_ERR_INVALID, "fy_foam_case_open_processor: rank %d of %d", rank, nranks);
            else if (stat(pd.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) rc = fail(FY_ERR_INVALID, "%s: no such processor directory (decomposePar first, or open the undecomposed case)", pd.c_str());
            else if (stat(join(c->dir, "processor" + std::to_string(nranks)).c_str(), &st) == 0) rc = fail(FY_ERR_INVALID, "%s is decomposed into more than %d parts", c->dir.c_str(), nranks);
            else if (c->desc.nz % nranks != 0) rc = fail(FY_ERR_UNSUPPORTED, "%s: %d planes do not split into %d equal z-slabs", c->dir.c_str(), c->desc.nz, nranks);
            else if (!c->file_cell.empty()) rc = fail(FY_ERR_UNSUPPORTED, "%s: a decomposed case whose mesh numbers its cells block by block is not supported", c->dir.c_str());
            else {
                c->fdir = pd; c->proc_rank = rank; c->proc_count = nranks;
                c->fcells /= (size_t)nranks; c->foffset = c->fcells * (size_t)rank;
            }
        }
    }
    if (rc == FY_OK) rc = read_controls(c);
    if (rc == FY_OK) rc = read_fields(c);
    if (rc != FY_OK) { delete c; return rc; }
    *out = c;
    return FY_OK;
}

int fy_foam_case_open(const char* case_dir, int solver, fy_foam_case** out) { return open_case(case_dir, solver, 0, 0, out); }
int fy_foam_case_open_processor(const char* case_dir, int solver, int rank, int nranks, fy_foam_case** out) {
    if (nranks < 1) return fail(FY_ERR_INVALID, "fy_foam_case_open_processor: nranks must be positive");
    return open_case(case_dir, solver, rank, nranks, out);
}

int fy_foam_case_desc(const fy_foam_case* c, fy_case_desc* out) {
    if (!c || !out) return fail(FY_ERR_INVALID, "fy_foam_case_desc: null argument");
    if (c->general) return fail(FY_ERR_UNSUPPORTED, "fy_foam_case_desc: the case holds a general mesh: fy_foam_case_poly_mesh + fy_foam_case_ldu_desc for fy_ldu_solver_create");
    *out = c->desc;
    inlets_desc(c, &out->inlets);
    return FY_OK;
}

int fy_foam_case_info_get(const fy_foam_case* c, fy_foam_case_info* out) {
    if (!c || !out) return fail(FY_ERR_INVALID, "fy_foam_case_info_get: null argument");
    std::memset(out, 0, sizeof(*out));
    out->start_time = c->start_time; out->end_time = c->end_time; out->delta_t = c->desc.dt;
    out->write_interval_steps = c->write_interval_steps;
    out->n_cells = c->general ? (int64_t)c->g_cells : (int64_t)c->desc.nx * c->desc.ny * c->desc.nz;
    out->field_cells = (int64_t)c->fcells; out->field_offset = (int64_t)c->foffset;
    std::snprintf(out->u_name, sizeof(out->u_name), "%s", c->u_name.c_str());
    std::snprintf(out->phase, sizeof(out->phase), "%s", c->phase.c_str());
    std::snprintf(out->start_name, sizeof(out->start_name), "%s", c->start_name.c_str());
    for (int s = 0; s < 6; ++s) std::snprintf(out->patch_of_side[s], sizeof(out->patch_of_side[s]), "%s", c->patch_of_side[s].c_str());
    out->n_ignored_functions = (int32_t)c->ignored_functions.size();
    return FY_OK;
}

int fy_foam_case_initial_fields(const fy_foam_case* c, double* U, double* p) {
    if (!c) return fail(FY_ERR_INVALID, "fy_foam_case_initial_fields: null case");
    if (U) std::memcpy(U, c->U0.data(), c->U0.size() * sizeof(double));
    if (p) std::memcpy(p, c->p0.data(), c->p0.size() * sizeof(double));
    return FY_OK;
}

int fy_foam_case_initial_nut(const fy_foam_case* c, double* nut) {
    if (!c || !nut) return fail(FY_ERR_INVALID, "fy_foam_case_initial_nut: null argument");
    if (c->nut0.empty()) return fail(FY_ERR_INVALID, "fy_foam_case_initial_nut: the case has no turbulence model");
    std::memcpy(nut, c->nut0.data(), c->nut0.size() * sizeof(double));
    return FY_OK;
}

int fy_foam_case_initial_k(const fy_foam_case* c, double* k) {
    if (!c || !k) return fail(FY_ERR_INVALID, "fy_foam_case_initial_k: null argument");
    if (c->k0.empty()) return fail(FY_ERR_INVALID, "fy_foam_case_initial_k: the case has no k equation");
    std::memcpy(k, c->k0.data(), c->k0.size() * sizeof(double));
    return FY_OK;
}

int fy_foam_case_initial_epsilon(const fy_foam_case* c, double* eps) {
    if (!c || !eps) return fail(FY_ERR_INVALID, "fy_foam_case_initial_epsilon: null argument");
    if (c->eps0.empty()) return fail(FY_ERR_INVALID, "fy_foam_case_initial_epsilon: the case has no epsilon equation");
    std::memcpy(eps, c->eps0.data(), c->eps0.size() * sizeof(double));
    return FY_OK;
}

int fy_foam_case_initial_T(const fy_foam_case* c, double* T) {
    if (!c || !T) return fail(FY_ERR_INVALID, "fy_foam_case_initial_T: null argument");
    if (c->T0.empty()) return fail(FY_ERR_INVALID, "fy_foam_case_initial_T: the case has no heat transfer");
    std::memcpy(T, c->T0.data(), c->T0.size() * sizeof(double));
    return FY_OK;
}

int fy_foam_case_write_fields(const fy_foam_case* c, const char* time_name, const double* U, const double* p, const double* alpha, const double* nut,
                              const double* k, const double* epsilon) {
    if (!c || !time_name || !*time_name || !U || !p) return fail(FY_ERR_INVALID, "fy_foam_case_write_fields: null argument");
    const std::string tdir = join(c->fdir, time_name);
    if (mkdir(tdir.c_str(), 0777) != 0) {
        struct stat st;
        if (stat(tdir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) return fail(FY_ERR_INVALID, "cannot create %s", tdir.c_str());
    }
    const size_t n = c->fcells;
    // (a field the start time had no file for -- alpha -- takes the processor patches of U with their type alone)
    std::vector<std::pair<std::string, std::string> > bare;
    for (const auto& e : c->bcs[F_U].extra) {
        const size_t a = e.second.find("type");
        const size_t b = a == std::string::npos ? a : e.second.find('\n', a);
        bare.emplace_back(e.first, (a == std::string::npos ? e.second : e.second.substr(0, b + 1)) + "        value uniform 1;\n");      // (alphac = 1 where nothing was deposited)
    }
    const char* zg = "        type            zeroGradient;\n";
    auto vec = [&](const double* src, int nc) { return std::vector<double>(src, src + n * (size_t)nc); };
    // alphac is AUTO_WRITE (pimpleFoamYade/createFields.H:139-150) and is written BEFORE setSourceZero resets it (pimpleFoamYade.C:106-108):
    // run the solver with fy_solver_hold_sources(s, 1) to get that.  eddyViscosity::nut_ is AUTO_WRITE, and so are k_ and epsilon_
    const struct { int F; const double* v; const char* dims; } out[] = {{F_U, U, "[0 1 -1 0 0 0 0]"}, {F_P, p, "[0 2 -2 0 0 0 0]"}, {F_ALPHA, alpha, "[0 0 0 0 0 0 0]"},
                                                                     {F_NUT, nut, "[0 2 -1 0 0 0 0]"}, {F_EPS, epsilon, "[0 2 -3 0 0 0 0]"}, {F_K, k, "[0 2 -2 0 0 0 0]"}};
    for (const auto& o : out) {
        if (!o.v || !has_field(c, o.F)) continue;
        const int nc = o.F == F_U ? 3 : 1;
        const PatchField* r = o.F == F_ALPHA ? nullptr : &c->bcs[o.F];
        FY_TRY(write_field(c, tdir, time_name, field_name(c, o.F), nc == 3 ? "volVectorField" : "volScalarField", o.dims, nc, vec(o.v, nc), r, zg, r ? r->extra : bare));
    }
    if (c->purge_write > 0) {
        // purgeWrite [OF-6 Time::writeObject]: once more than N time directories have been written, the oldest of them goes
        bool known = false;
        for (const std::string& w : c->written) known = known || w == time_name;
        if (!known) c->written.push_back(time_name);
        while ((int)c->written.size() > c->purge_write) {
            const std::string old = join(c->fdir, c->written.front());
            c->written.erase(c->written.begin());
            if (DIR* dd = opendir(old.c_str())) {
                while (struct dirent* de = readdir(dd)) {
                    const std::string nm = de->d_name;
                    if (nm == "." || nm == "..") continue;
                    if (nm == "uniform") {                               // <time>/uniform/<object>Properties of a fieldAverage object
                        if (DIR* ud = opendir(join(old, nm).c_str())) {
                            while (struct dirent* ue = readdir(ud)) if (std::strcmp(ue->d_name, ".") != 0 && std::strcmp(ue->d_name, "..") != 0) ::unlink(join(join(old, nm), ue->d_name).c_str());
                            closedir(ud);
                        }
                        ::rmdir(join(old, nm).c_str());
                    } else ::unlink(join(old, nm).c_str());
                }
                closedir(dd);
                ::rmdir(old.c_str());
            }
        }
    }
    return FY_OK;
}

int fy_foam_case_write_time(const fy_foam_case* c, fy_solver* s, const char* time_name) {
    if (!c || !s || !time_name || !*time_name) return fail(FY_ERR_INVALID, "fy_foam_case_write_time: null argument");
    int64_t cnt = 0;
    FY_TRY(fy_solver_field_count(s, "p", &cnt));
    if ((size_t)cnt != c->fcells) return fail(FY_ERR_UNSUPPORTED, "fy_foam_case_write_time: the solver holds %lld cells, the case's field files %zu (a slab of an undecomposed case: gather the slabs and use fy_foam_case_write_fields)", (long long)cnt, c->fcells);
    c->u_boundary_now.clear();
    if (!c->inlets.empty()) {                             // the inlet patches' `value`: the faces' current values
        int64_t nb = 0;
        FY_TRY(fy_solver_field_count(s, "U_boundary", &nb));
        c->u_boundary_now.resize((size_t)nb);
        FY_TRY(fy_solver_read_field_host(s, "U_boundary", c->u_boundary_now.data()));
    }
    const int wrc = write_solver_fields(c, time_name, {F_U, F_P, F_ALPHA, F_NUT, F_EPS, F_K}, [s](const char* nm, double* v) { return fy_solver_read_field_host(s, nm, v); });
    c->u_boundary_now.clear();
    FY_TRY(wrc);
    if (has_field(c, F_T)) {                              // T | T.<phase> beside them, with the start time's patch entries
        std::vector<double> T(c->fcells);
        FY_TRY(fy_solver_read_field_host(s, "T", T.data()));
        FY_TRY(write_field(c, join(c->fdir, time_name), time_name, field_name(c, F_T), "volScalarField", "[0 0 0 1 0 0 0]", 1, T, &c->bcs[F_T], "        type            zeroGradient;\n",
                           c->bcs[F_T].extra));
    }
    FY_TRY(write_solid_stats(c, time_name, [s](const char* nm, int64_t* n) { return fy_solver_field_count(s, nm, n); }, [s](const char* nm, double* v) { return fy_solver_read_field_host(s, nm, v); }));
    fy_step_stats st;
    FY_TRY(fy_solver_get_stats(s, &st));
    return write_averages(c, time_name, st.delta_t > 0 ? st.delta_t : c->desc.dt, [s](const char* nm, int64_t* n) { return fy_solver_field_count(s, nm, n); },
                          [s](const char* nm, double* v) { return fy_solver_read_field_host(s, nm, v); },
                          [s](int i, int64_t* N, double* T) { return fy_solver_get_average_state(s, i, N, T); });
}

int fy_foam_case_restore_averages(const fy_foam_case* c, fy_solver* s, int* restored) {
    if (!c || !s) return fail(FY_ERR_INVALID, "fy_foam_case_restore_averages: null argument");
    if (c->general) return fail(FY_ERR_INVALID, "fy_foam_case_restore_averages: the case holds a general mesh (fy_foam_case_restore_averages_ldu)");
    return restore_averages(c, c->desc.dt, restored, [s](const char* nm, const double* v) { return fy_solver_write_field_host(s, nm, v); },
                            [s](int i, int64_t N, double T) { return fy_solver_set_average_state(s, i, N, T); });
}

int fy_foam_case_ignored_function(const fy_foam_case* c, int i, char* out, int cap) {
    if (!c || !out || cap < 1) return fail(FY_ERR_INVALID, "fy_foam_case_ignored_function: null argument");
    if (i < 0 || (size_t)i >= c->ignored_functions.size()) return fail(FY_ERR_INVALID, "fy_foam_case_ignored_function: object %d of %zu", i, c->ignored_functions.size());
    std::snprintf(out, (size_t)cap, "%s", c->ignored_functions[(size_t)i].c_str());
    return FY_OK;
}

int fy_foam_case_open_general(const char* case_dir, int solver, fy_foam_case** out) {
    if (!case_dir || !out) return fail(FY_ERR_INVALID, "fy_foam_case_open_general: null argument");
    if (solver != FY_SOLVER_ICO && solver != FY_SOLVER_PIMPLE) return fail(FY_ERR_INVALID, "fy_foam_case_open_general: solver must be FY_SOLVER_ICO or FY_SOLVER_PIMPLE");
    *out = nullptr;
    fy_foam_case* c = new (std::nothrow) fy_foam_case();
    if (!c) return fail(FY_ERR_INVALID, "out of host memory");
    c->dir = case_dir; c->fdir = c->dir; c->solver = solver; c->general = true;
    fy_case_defaults(&c->desc, solver);
    int rc = read_general_mesh(c);
    if (rc == FY_OK) { c->fcells = (size_t)c->g_cells; rc = read_controls(c); }
    if (rc == FY_OK) rc = check_general_schemes(c);
    if (rc == FY_OK) rc = read_general_fields(c);
    if (rc != FY_OK) { delete c; return rc; }
    *out = c;
    return FY_OK;
}

int fy_foam_case_poly_mesh(const fy_foam_case* c, fy_poly_mesh* out) {
    if (!c || !out) return fail(FY_ERR_INVALID, "fy_foam_case_poly_mesh: null argument");
    if (!c->general) return fail(FY_ERR_INVALID, "fy_foam_case_poly_mesh: the case was opened as a block (fy_foam_case_open): use fy_foam_case_desc, or open it with fy_foam_case_open_general");
    std::memset(out, 0, sizeof(*out));
    out->n_points = (int32_t)(c->g_points.size() / 3); out->points = c->g_points.data();
    out->n_faces = (int32_t)c->g_own.size(); out->n_internal_faces = c->g_internal;
    out->face_offsets = c->g_face_off.data(); out->face_points = c->g_face_pts.data();
    out->owner = c->g_own.data(); out->neighbour = c->g_nei.data();
    out->n_cells = c->g_cells;
    out->n_patches = (int32_t)c->g_patch_name.size(); out->patch_start = c->g_patch_start.data(); out->patch_size = c->g_patch_size.data();
    out->patch_neighbour = nullptr;
    for (int32_t v : c->g_patch_neighbour) if (v >= 0) out->patch_neighbour = c->g_patch_neighbour.data();
    return FY_OK;
}

int fy_foam_case_ldu_desc(const fy_foam_case* c, fy_ldu_case* out) {
    if (!c || !out) return fail(FY_ERR_INVALID, "fy_foam_case_ldu_desc: null argument");
    if (!c->general) return fail(FY_ERR_INVALID, "fy_foam_case_ldu_desc: the case was opened as a block (fy_foam_case_open)");
    fy_ldu_case_defaults(out);
    const fy_case_desc& d = c->desc;
    out->dt = d.dt; out->nu = d.nu; out->rho_fluid = d.rho_fluid; out->rho_particle = d.rho_particle;
    out->n_correctors = d.n_correctors; out->n_non_orth_correctors = d.n_non_orth_correctors; out->momentum_predictor = d.momentum_predictor;
    out->p_ref_cell = d.p_ref_cell; out->p_ref_value = d.p_ref_value;
    out->p_tol = d.p_tol; out->p_rel_tol = d.p_rel_tol; out->p_final_tol = d.p_final_tol; out->p_final_rel_tol = d.p_final_rel_tol; out->p_max_iter = d.p_max_iter;
    out->u_tol = d.u_tol; out->u_rel_tol = d.u_rel_tol; out->u_max_iter = d.u_max_iter; out->p_solver = d.p_solver;
    out->solver = c->solver; out->n_outer_correctors = d.n_outer_correctors;
    for (int a = 0; a < 3; ++a) out->g[a] = d.g[a];
    out->u_relax = d.u_relax; out->u_relax_final = d.u_relax_final; out->p_relax = d.p_relax; out->p_relax_final = d.p_relax_final;
    out->adjust_time_step = d.adjust_time_step; out->max_co = d.max_co; out->max_delta_t = d.max_delta_t;
    out->turbulence_model = d.turbulence_model; out->les_ck = d.les_ck; out->les_ce = d.les_ce; out->les_delta_coeff = d.les_delta_coeff; out->nut_initial = d.nut_initial;
    const PatchField &U = c->bcs[F_U], &p = c->bcs[F_P], &nut = c->bcs[F_NUT], &k = c->bcs[F_K], &eps = c->bcs[F_EPS];      // (nut, k, epsilon: NULL where the case has no such field)
    out->nut_bc = nut.bc.empty() ? nullptr : nut.bc.data(); out->nut_value = nut.val.empty() ? nullptr : nut.val.data();
    out->convection_scheme = d.convection_scheme; out->convection_limiter_k = d.convection_limiter_k;
    out->k_initial = d.k_initial; out->k_bc = k.bc.empty() ? nullptr : k.bc.data(); out->k_value = k.val.empty() ? nullptr : k.val.data();
    out->k_convection_scheme = d.k_convection_scheme; out->k_tol = d.k_tol; out->k_rel_tol = d.k_rel_tol; out->k_max_iter = d.k_max_iter; out->k_relax = d.k_relax;
    out->ras_cmu = d.ras_cmu; out->ras_c1 = d.ras_c1; out->ras_c2 = d.ras_c2; out->ras_c3 = d.ras_c3; out->ras_sigmak = d.ras_sigmak; out->ras_sigmaeps = d.ras_sigmaeps;
    out->eps_initial = d.eps_initial; out->eps_bc = eps.bc.empty() ? nullptr : eps.bc.data(); out->eps_value = eps.val.empty() ? nullptr : eps.val.data();
    out->eps_convection_scheme = d.eps_convection_scheme; out->eps_tol = d.eps_tol; out->eps_rel_tol = d.eps_rel_tol; out->eps_max_iter = d.eps_max_iter; out->eps_relax = d.eps_relax;
    out->wf_kappa = d.wf_kappa; out->wf_E = d.wf_E;
    out->drag_law = d.drag_law; out->force_models = d.force_models; out->solid_stats = d.solid_stats;
    out->average = d.average;
    out->monitors = d.monitors;
    out->wall_loads = d.wall_loads;
    out->flow_control = c->flow;
    inlets_desc(c, &out->inlets);
    out->u_bc = U.bc.data(); out->u_value = U.val.data(); out->p_bc = p.bc.data(); out->p_value = p.val.data();
    return FY_OK;
}

int fy_foam_case_patch_name(const fy_foam_case* c, int patch, char* out, int cap) {
    if (!c || !out || cap < 1) return fail(FY_ERR_INVALID, "fy_foam_case_patch_name: null argument");
    const std::vector<std::string>& names = c->general ? c->g_patch_name : c->patch_order;
    if (patch < 0 || (size_t)patch >= names.size()) return fail(FY_ERR_INVALID, "fy_foam_case_patch_name: patch %d of %zu", patch, names.size());
    std::snprintf(out, (size_t)cap, "%s", names[(size_t)patch].c_str());
    return FY_OK;
}

int fy_foam_case_write_time_ldu(const fy_foam_case* c, fy_ldu_solver* s, const char* time_name) {
    if (!c || !s || !time_name || !*time_name) return fail(FY_ERR_INVALID, "fy_foam_case_write_time_ldu: null argument");
    if (!c->general) return fail(FY_ERR_INVALID, "fy_foam_case_write_time_ldu: the case was opened as a block (fy_foam_case_open)");
    int64_t cnt = 0;
    FY_TRY(fy_ldu_solver_field_count(s, "p", &cnt));
    if ((size_t)cnt != c->fcells) return fail(FY_ERR_INVALID, "fy_foam_case_write_time_ldu: the solver holds %lld cells, the case %zu", (long long)cnt, c->fcells);
    // (alpha: with fy_ldu_solver_hold_sources, before setSourceZero)
    c->u_boundary_now.clear();
    bool open_u = false;
    for (int32_t b : c->bcs[F_U].bc) open_u = open_u || b >= FY_BC_U_INLET_OUTLET;
    if (!c->inlets.empty() || open_u) {                   // the inlet patches' and the open patches' `value`: the faces' current values
        int64_t nb = 0;
        FY_TRY(fy_ldu_solver_field_count(s, "U_boundary", &nb));
        c->u_boundary_now.resize((size_t)nb);
        FY_TRY(fy_ldu_solver_read_field_host(s, "U_boundary", c->u_boundary_now.data()));
    }
    const int wrc = write_solver_fields(c, time_name, {F_U, F_P, F_ALPHA, F_NUT, F_K, F_EPS}, [s](const char* nm, double* v) { return fy_ldu_solver_read_field_host(s, nm, v); });
    c->u_boundary_now.clear();
    FY_TRY(wrc);
    FY_TRY(write_solid_stats(c, time_name, [s](const char* nm, int64_t* n) { return fy_ldu_solver_field_count(s, nm, n); }, [s](const char* nm, double* v) { return fy_ldu_solver_read_field_host(s, nm, v); }));
    fy_step_stats st;
    FY_TRY(fy_ldu_solver_get_stats(s, &st));
    FY_TRY(write_averages(c, time_name, st.delta_t > 0 ? st.delta_t : c->desc.dt, [s](const char* nm, int64_t* n) { return fy_ldu_solver_field_count(s, nm, n); },
                          [s](const char* nm, double* v) { return fy_ldu_solver_read_field_host(s, nm, v); },
                          [s](int i, int64_t* N, double* T) { return fy_ldu_solver_get_average_state(s, i, N, T); }));
    // meanVelocityForce's restart file [OF-6 meanVelocityForce::writeProps, as recalled]: the gradient the next assembly would use, 17 digits (a restart continues exactly)
    double gradient = 0.0;
    if (c->flow.on && fy_ldu_solver_get_flow_control(s, &gradient, nullptr, nullptr, nullptr, nullptr) == FY_OK) {      // (a solver with the control switched off: no file)
        const std::string udir = join(join(c->fdir, time_name), "uniform");
        if (mkdir(udir.c_str(), 0777) != 0) {
            struct stat sb;
            if (stat(udir.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode)) return fail(FY_ERR_INVALID, "cannot create %s", udir.c_str());
        }
        const std::string ppath = join(udir, "meanVelocityForceProperties");
        FILE* f = std::fopen(ppath.c_str(), "wb");
        if (!f) return fail(FY_ERR_INVALID, "cannot write %s", ppath.c_str());
        std::fprintf(f, "FoamFile\n{\n    version     2.0;\n    format      ascii;\n    class       dictionary;\n    location    \"%s/uniform\";\n    object      meanVelocityForceProperties;\n}\n\n"
                        "gradient        %.17g;\n", time_name, gradient);
        std::fclose(f);
    }
    return FY_OK;
}

int fy_foam_case_restore_averages_ldu(const fy_foam_case* c, fy_ldu_solver* s, int* restored) {
    if (!c || !s) return fail(FY_ERR_INVALID, "fy_foam_case_restore_averages_ldu: null argument");
    if (!c->general) return fail(FY_ERR_INVALID, "fy_foam_case_restore_averages_ldu: the case was opened as a block (fy_foam_case_restore_averages)");
    return restore_averages(c, c->desc.dt, restored, [s](const char* nm, const double* v) { return fy_ldu_solver_write_field_host(s, nm, v); },
                            [s](int i, int64_t N, double T) { return fy_ldu_solver_set_average_state(s, i, N, T); });
}

int fy_foam_case_monitor_count(const fy_foam_case* c) { return c ? (int)c->monitors.size() : 0; }

int fy_foam_case_write_monitors(const fy_foam_case* c, fy_solver* s) {
    if (!c || !s) return fail(FY_ERR_INVALID, "fy_foam_case_write_monitors: null argument");
    if (c->general) return fail(FY_ERR_INVALID, "fy_foam_case_write_monitors: the case holds a general mesh (fy_foam_case_write_monitors_ldu)");
    const fy_case_desc& d = c->desc;
    auto h = [&](int a, int q) { return c->grading[a].empty() ? d.dx : c->grading[a][(size_t)q]; };
    return write_monitors(c, [s](int q, int32_t* nv) { return fy_solver_monitor_layout(s, q, nv, nullptr, 0); },
                          [s](int q, int64_t first, int64_t mx, double* t, double* v, int64_t* n) { return fy_solver_get_monitor_rows(s, q, first, mx, t, v, n); },
                          [&](int q, int64_t* n, double* total) -> int {
                              const int ext[3] = {d.nx, d.ny, d.nz};
                              double len[3] = {0, 0, 0};
                              for (int a = 0; a < 3; ++a) for (int k = 0; k < ext[a]; ++k) len[a] += h(a, k);
                              if (c->monitors[(size_t)q].vol) { *n = (int64_t)d.nx * d.ny * d.nz; *total = len[0] * len[1] * len[2]; return FY_OK; }
                              *n = 0; *total = 0;
                              for (int side = 0; side < 6; ++side)
                                  if (d.monitors.objects[q].patch >> side & 1) {
                                      const int a = side / 2, b1 = (a + 1) % 3, b2 = (a + 2) % 3;
                                      *n += (int64_t)ext[b1] * ext[b2]; *total += len[b1] * len[b2];
                                  }
                              return FY_OK;
                          });
}

int fy_foam_case_write_monitors_ldu(const fy_foam_case* c, fy_ldu_solver* s) {
    if (!c || !s) return fail(FY_ERR_INVALID, "fy_foam_case_write_monitors_ldu: null argument");
    if (!c->general) return fail(FY_ERR_INVALID, "fy_foam_case_write_monitors_ldu: the case was opened as a block (fy_foam_case_write_monitors)");
    return write_monitors(c, [s](int q, int32_t* nv) { return fy_ldu_solver_monitor_layout(s, q, nv, nullptr, 0); },
                          [s](int q, int64_t first, int64_t mx, double* t, double* v, int64_t* n) { return fy_ldu_solver_get_monitor_rows(s, q, first, mx, t, v, n); },
                          [&](int q, int64_t* n, double* total) -> int {
                              const bool vol = c->monitors[(size_t)q].vol;
                              int64_t cnt = 0, no = 0;
                              FY_TRY(fy_ldu_solver_field_count(s, vol ? "V" : "magSf", &cnt));
                              std::vector<double> m((size_t)cnt);
                              FY_TRY(fy_ldu_solver_read_field_host(s, vol ? "V" : "magSf", m.data()));
                              *n = 0; *total = 0;
                              if (vol) { *n = cnt; for (double x : m) *total += x; return FY_OK; }
                              // the solver's face f was made from the case's face orig_face[f] (a mesh with folded cyclic pairs); without such pairs the numbering is the case's
                              FY_TRY(fy_ldu_solver_field_count(s, "orig_face", &no));
                              std::vector<double> of((size_t)no);
                              if (no) FY_TRY(fy_ldu_solver_read_field_host(s, "orig_face", of.data()));
                              const int pa = c->desc.monitors.objects[q].patch;
                              const int64_t f0 = c->g_patch_start[(size_t)pa], f1 = f0 + c->g_patch_size[(size_t)pa];
                              for (int64_t f = 0; f < cnt; ++f) {
                                  const int64_t orig = no ? (int64_t)of[(size_t)f] : f;
                                  if (orig >= f0 && orig < f1) { *n += 1; *total += m[(size_t)f]; }
                              }
                              return FY_OK;
                          });
}

int fy_foam_case_wall_loads_count(const fy_foam_case* c) { return c ? (int)c->wall_loads().size() : 0; }

int fy_foam_case_write_wall_loads(const fy_foam_case* c, fy_solver* s) {
    if (!c || !s) return fail(FY_ERR_INVALID, "fy_foam_case_write_wall_loads: null argument");
    if (c->general) return fail(FY_ERR_INVALID, "fy_foam_case_write_wall_loads: the case holds a general mesh (fy_foam_case_write_wall_loads_ldu)");
    return write_wall_loads(c, [s](int q, int32_t* nv) { return fy_solver_wall_loads_layout(s, q, nv, nullptr, 0); },
                            [s](int q, int64_t first, int64_t mx, double* t, double* v, int64_t* n) { return fy_solver_get_wall_load_rows(s, q, first, mx, t, v, n); });
}

int fy_foam_case_write_wall_loads_ldu(const fy_foam_case* c, fy_ldu_solver* s) {
    if (!c || !s) return fail(FY_ERR_INVALID, "fy_foam_case_write_wall_loads_ldu: null argument");
    if (!c->general) return fail(FY_ERR_INVALID, "fy_foam_case_write_wall_loads_ldu: the case was opened as a block (fy_foam_case_write_wall_loads)");
    return write_wall_loads(c, [s](int q, int32_t* nv) { return fy_ldu_solver_wall_loads_layout(s, q, nv, nullptr, 0); },
                            [s](int q, int64_t first, int64_t mx, double* t, double* v, int64_t* n) { return fy_ldu_solver_get_wall_load_rows(s, q, first, mx, t, v, n); });
}

int fy_foam_case_porous_zones(const fy_foam_case* c, fy_porous_desc* out) {
    if (!c || !out) return fail(FY_ERR_INVALID, "fy_foam_case_porous_zones: null argument");
    std::memset(out, 0, sizeof(*out));
    out->n_zones = (int32_t)c->porous.size();
    for (size_t z = 0; z < c->porous.size(); ++z) {
        const fy_foam_case::PorousMeta& m = c->porous[z];
        fy_porous_zone& Z = out->zones[z];
        std::snprintf(Z.name, sizeof(Z.name), "%s", m.name.c_str());
        for (int a = 0; a < 3; ++a) { Z.d[a] = m.d[a]; Z.f[a] = m.f[a]; }
        Z.n_cells = (int32_t)m.cells.size(); Z.cells = m.cells.data();
    }
    return FY_OK;
}

int fy_foam_case_make_solver(const fy_foam_case* c, const fy_transport* tr, int device_ordinal, fy_solver** out) {
    if (!c || !out) return fail(FY_ERR_INVALID, "fy_foam_case_make_solver: null argument");
    fy_case_desc cd;
    fy_porous_desc pz;
    FY_TRY(fy_foam_case_desc(c, &cd));
    FY_TRY(fy_foam_case_porous_zones(c, &pz));
    FY_TRY(fy_solver_create(&cd, tr, device_ordinal, out));
    const int rc = pz.n_zones ? fy_solver_set_porous_zones(*out, &pz) : FY_OK;
    if (rc != FY_OK) { fy_solver_destroy(*out); *out = nullptr; }
    return rc;
}

int fy_foam_case_make_ldu_solver(const fy_foam_case* c, const fy_transport* tr, int device_ordinal, fy_ldu_solver** out) {
    if (!c || !out) return fail(FY_ERR_INVALID, "fy_foam_case_make_ldu_solver: null argument");
    fy_poly_mesh pm;
    fy_ldu_case lc;
    fy_porous_desc pz;
    FY_TRY(fy_foam_case_poly_mesh(c, &pm));
    FY_TRY(fy_foam_case_ldu_desc(c, &lc));
    FY_TRY(fy_foam_case_porous_zones(c, &pz));
    FY_TRY(fy_ldu_solver_create(&pm, &lc, tr, device_ordinal, out));
    const int rc = pz.n_zones ? fy_ldu_solver_set_porous_zones(*out, &pz) : FY_OK;
    if (rc != FY_OK) { fy_ldu_solver_destroy(*out); *out = nullptr; }
    return rc;
}

int fy_foam_case_close(fy_foam_case* c) {
    delete c;
    return FY_OK;
}

}  // extern "C"
