"""nutkWallFunction / epsilonWallFunction / kqRWallFunction on the general polyhedral mesh (fy_ldu_solver): nearWallDist on arbitrary faces, the wall value of nut,
the wall cells' imposed epsilon and production, fvMatrix::setValues on face-addressed coefficients; the case reader's rules for them (DESIGN_FV.md, wall functions)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import poly_meshes as pm
from test_ldu_case import CASES, prod  # noqa: F401  (the fixture)

WF = 2                                   # FY_BC_WALL_FUNCTION


# ---- the case reader (no GPU) -----------------------------------------------------------------------------------------------------------------------------------

def wf_bed(tmp_path, types=None, nut_walls="nutkWallFunction; kappa 0.4; E 9.0; value uniform 0;", eps_walls="epsilonWallFunction; value uniform 2e-3;",
           k_walls="kqRWallFunction; value uniform 3e-4;", model="RAS { RASModel kEpsilon; turbulence on; }"):
    """tests/golden/cases/bed_pimple on a wavy polyhedral mesh (bottom, top: patch; walls: wall), RAS kEpsilon with the wall functions on `walls`"""
    dst = tmp_path / "bed"
    shutil.copytree(os.path.join(CASES, "bed_pimple"), dst)
    os.remove(dst / "system/blockMeshDict")
    L = (0.06, 0.06, 0.12)
    wav = pm.wavy(0.15 * 0.005, L)
    mesh = pm.hex_block(12, 12, 24, L, lambda P: wav(P) + np.array([-0.03, -0.03, 0.0]), patches=[("bottom", [4]), ("top", [5]), ("walls", [0, 1, 2, 3])])
    pm.write_poly_mesh_files(dst, mesh, types or {"bottom": "patch", "top": "patch", "walls": "wall"})
    sim = "RAS" if "RAS" in model else "LES"
    (dst / "constant/turbulenceProperties.water").write_text("simulationType %s;\n%s\n" % (sim, model))
    head = "FoamFile { version 2.0; format ascii; class volScalarField; object %s; }\ndimensions %s;\ninternalField uniform %s;\nboundaryField\n{\n"
    (dst / "0/nut.water").write_text(head % ("nut.water", "[0 2 -1 0 0 0 0]", "2e-6") + "    bottom { type zeroGradient; }\n    top { type zeroGradient; }\n"
                                     "    walls { type %s }\n}\n" % nut_walls)
    (dst / "0/k.water").write_text(head % ("k.water", "[0 2 -2 0 0 0 0]", "3e-4") + "    bottom { type fixedValue; value uniform 3e-4; }\n    top { type zeroGradient; }\n"
                                   "    walls { type %s }\n}\n" % k_walls)
    (dst / "0/epsilon.water").write_text(head % ("epsilon.water", "[0 2 -3 0 0 0 0]", "2e-3") + "    bottom { type fixedValue; value uniform 2e-3; }\n"
                                         "    top { type zeroGradient; }\n    walls { type %s }\n}\n" % eps_walls)
    return dst, mesh


def test_general_case_with_wall_functions_is_read(prod, tmp_path):  # noqa: F811
    dst, _ = wf_bed(tmp_path)
    fc = prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)
    lc = fc.ldu_case
    w = fc.patch_names.index("walls")
    assert lc.turbulence_model == prod.TURBULENCE_KEPSILON
    assert lc.nut_bc[w] == prod.BC_WALL_FUNCTION and lc.eps_bc[w] == prod.BC_WALL_FUNCTION and lc.k_bc[w] == 0
    assert [lc.nut_bc[q] for q in range(3) if q != w] == [0, 0] and [lc.eps_bc[q] for q in range(3) if q != w] == [1, 0]
    assert (lc.wf_kappa, lc.wf_E) == (0.4, 9.0)
    fc.close()


def test_wall_function_defaults(prod, tmp_path):  # noqa: F811
    """without kappa / E in the patch entry: OpenFOAM's 0.41 / 9.8; fy_ldu_case_defaults agrees"""
    dst, _ = wf_bed(tmp_path, nut_walls="nutkWallFunction; value uniform 0;")
    fc = prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)
    assert (fc.ldu_case.wf_kappa, fc.ldu_case.wf_E) == (0.41, 9.8)
    fc.close()
    prod.LduSolver._bind()
    c = prod.LduCase()
    prod.lib().fy_ldu_case_defaults(ctypes.byref(c))
    assert (c.wf_kappa, c.wf_E) == (0.41, 9.8)


@pytest.mark.parametrize("kw,needle", [
    (dict(types={"bottom": "patch", "top": "patch", "walls": "patch"}), "'walls': nutkWallFunction is a wall function.*'patch'"),
    (dict(nut_walls="zeroGradient;"), "'walls': epsilonWallFunction takes its constants"),
    (dict(types={"bottom": "wall", "top": "patch", "walls": "wall"}), "different kappa"),
    (dict(eps_walls="epsilonLowReWallFunction; value uniform 2e-3;"), "epsilonLowReWallFunction"),
    (dict(model="LES { LESModel Smagorinsky; delta cubeRootVol; turbulence on; cubeRootVolCoeffs { deltaCoeff 1; } }"), "nutkWallFunction"),
    (dict(nut_walls="nutkWallFunction; Cmu 0.1; value uniform 0;"), "Cmu"),
])
def test_what_the_wall_functions_cannot_do_is_refused_by_name(prod, tmp_path, kw, needle):  # noqa: F811
    dst, _ = wf_bed(tmp_path, **kw)
    if kw.get("types", {}).get("bottom") == "wall":           # a second wall patch with its own constants
        t = (dst / "0/nut.water").read_text()
        (dst / "0/nut.water").write_text(t.replace("bottom { type zeroGradient; }", "bottom { type nutkWallFunction; kappa 0.41; E 9.0; value uniform 0; }"))
    with pytest.raises(prod.FoamYadeError, match=needle):
        prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)


def test_epsilon_wall_function_on_a_patch_is_refused_by_name(prod, tmp_path):  # noqa: F811
    dst, _ = wf_bed(tmp_path)
    t = (dst / "0/epsilon.water").read_text()
    (dst / "0/epsilon.water").write_text(t.replace("top { type zeroGradient; }", "top { type epsilonWallFunction; value uniform 2e-3; }"))
    with pytest.raises(prod.FoamYadeError, match="'top': epsilonWallFunction is a wall function.*'patch'"):
        prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)


# ---- the solver (GPU) -------------------------------------------------------------------------------------------------------------------------------------------

def close(a, b, rtol, what):
    sc = np.abs(b).max() + 1e-300
    assert np.abs(a - b).max() <= rtol * sc, (what, np.abs(a - b).max() / sc)


def bed_particles(rs, npart, box, dx):
    rec = np.zeros((npart, 10))
    rec[:, 0:3] = rs.random_sample((npart, 3)) * np.array([box, box, 0.6 * box]) + np.array([0.0, 0.0, 0.05 * box])
    rec[:, 3:6] = 0.05 * rs.standard_normal((npart, 3))
    rec[:, 9] = 0.2 * dx
    return rec


def boundary_faces(mesh, patches):
    """solver boundary-face indices (f - n_internal) of the given patches"""
    ni = len(mesh["neighbour"])
    return np.concatenate([np.arange(mesh["patch_start"][q], mesh["patch_start"][q] + mesh["patch_size"][q]) - ni for q in patches])


def face_centre(P):
    """[OF-6 face::centre]: a triangle's centroid; otherwise the area-weighted centroid of the fan about the point average"""
    if len(P) == 3:
        return P.mean(axis=0)
    c0 = P.mean(axis=0)
    Q = np.roll(P, -1, axis=0)
    a = np.linalg.norm(np.cross(P - c0, Q - c0), axis=1)
    return (a[:, None] * (P + Q + c0)).sum(axis=0) / (3.0 * a.sum())


def nearest_on_triangle(p, a, b, c):
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = ab @ ap, ac @ ap
    if d1 <= 0 and d2 <= 0:
        return a
    bp = p - b
    d3, d4 = ab @ bp, ac @ bp
    if d3 >= 0 and d4 <= d3:
        return b
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        return a + d1 / (d1 - d3) * ab
    cp = p - c
    d5, d6 = ab @ cp, ac @ cp
    if d6 >= 0 and d5 <= d6:
        return c
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        return a + d2 / (d2 - d6) * ac
    va = d3 * d6 - d5 * d4
    if va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
        return b + (d4 - d3) / ((d4 - d3) + (d5 - d6)) * (c - b)
    r = 1.0 / (va + vb + vc)
    return a + vb * r * ab + vc * r * ac


def near_wall_dist(mesh, C, patches):
    """nearWallDist restated [OF-6 nearWallDist::correct, cellDistFuncs::getPointNeighbours / smallestDist, face::nearestPointClassify]: per boundary face of the
    patches the distance from its owner's centre to the nearest point of the faces of the same patch sharing a point with it"""
    ni, nb = len(mesh["neighbour"]), len(mesh["owner"]) - len(mesh["neighbour"])
    y = np.zeros(nb)
    pts, off, fp = mesh["points"], mesh["face_offsets"], mesh["face_points"]
    verts = lambda f: fp[off[f]:off[f + 1]]
    for q in patches:
        faces = range(mesh["patch_start"][q], mesh["patch_start"][q] + mesh["patch_size"][q])
        by_point = {}
        for f in faces:
            for v in verts(f):
                by_point.setdefault(int(v), set()).add(f)
        for f in faces:
            p = C[mesh["owner"][f]]
            best = np.inf
            for g in set().union(*(by_point[int(v)] for v in verts(f))):
                P = pts[verts(g)]
                if len(P) == 3:
                    tris = [(P[0], P[1], P[2])]
                else:
                    ctr = face_centre(P)
                    tris = [(P[a], P[(a + 1) % len(P)], ctr) for a in range(len(P))]
                best = min(best, min(np.linalg.norm(p - nearest_on_triangle(p, *t)) for t in tris))
            y[f - ni] = best
    return y


RAS = dict(turbulence_model=3, eps_initial=1.2e-4, eps_tol=1e-13, k_initial=2e-4, k_tol=1e-13, nut_initial=3e-5, ras_cmu=0.085, ras_c1=1.4, ras_c2=1.9, ras_c3=-0.33,
           ras_sigmak=1.1, ras_sigmaeps=1.25, eps_convection_scheme=1, eps_relax=0.7, k_convection_scheme=1, k_relax=0.8)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["kEpsilon", "kEpsilon_graded", "kEqn"])
def test_wall_functions_on_a_lattice_equal_the_structured_hip_solver(prod, variant):  # noqa: F811
    """the wall functions through both HIP solvers on the same block (as test_ldu_parity.py's kEqn / kEpsilon lattice test: the general side is given the structured
    coupling's alpha / drag / source), nutkWallFunction (and epsilonWallFunction) on four sides and the lid: epsilon, k, nut, U after each of three steps; on a graded
    block the corner cells average unequal wall distances.  nearWallDist is the half cell width on every wall face"""
    n, box = 12, 0.1
    dx = box / n
    wall = [0, 1, 2, 3, 4]
    if variant == "kEpsilon_graded":
        sizes = [np.geomspace(1.0, r, n) for r in (2.5, 0.5, 1.8)]
        sizes = [box * s / s.sum() for s in sizes]
        nodes = [np.concatenate([[0.0], np.cumsum(s)]) for s in sizes]
        nodes = [np.concatenate([x[:-1], [box]]) for x in nodes]
        vm = lambda P: np.stack([nodes[a][np.rint(P[:, a] / (box / n)).astype(int)] for a in range(3)], axis=1)
        mesh = pm.hex_block(n, n, n, (box, box, box), vm)
        sizes = [np.diff(x) for x in nodes]
    else:
        mesh = pm.hex_block(n, n, n, (box, box, box))
    kw = dict(p_tol=1e-11, p_rel_tol=0.0, p_final_tol=1e-11, u_tol=1e-11)
    u_val = [(0, 0, 0)] * 6
    u_val[3] = (0.3, 0, 0.1)
    nut_bc = [WF if q in wall else 0 for q in range(6)]
    nut_val = [1e-5 if q in wall else 0.0 for q in range(6)]
    if variant == "kEqn":
        turb = dict(turbulence_model=2, nut_initial=3e-5, les_delta_coeff=0.8, k_initial=2e-4, k_tol=1e-13, k_convection_scheme=1, k_relax=0.8)
        fkw = dict(nut_bc=nut_bc, nut_value=nut_val)
        gkw = dict(nut_bc=nut_bc, nut_val=nut_val)
    else:
        turb = dict(RAS)
        eps_bc = [WF if q in wall else 0 for q in range(6)]
        fkw = dict(nut_bc=nut_bc, nut_value=nut_val, eps_bc=eps_bc, eps_value=[0.0] * 6)
        gkw = dict(nut_bc=nut_bc, nut_val=nut_val, eps_bc=eps_bc, eps_val=[0.0] * 6)
    turb.update(wf_kappa=0.4, wf_E=9.0, k_initial=5e-3)            # (y+ about 16 at the walls: above yPlusLam, the logarithmic branch)
    if variant != "kEqn":
        turb.update(eps_initial=1e-3)
    grading = dict(grading=sizes) if variant == "kEpsilon_graded" else {}
    case = prod.make_case(1, n, n, n, dx, 2e-4, 1e-5, g=(0, 0, -9.81), u_val=u_val, p_bc=[2] * 6, p_solver=0, n_outer_correctors=2, n_correctors=2, p_max_iter=5000,
                          **grading, **turb, **fkw, **kw)
    f = prod.Solver(case)
    g = prod.LduSolver(mesh, 2e-4, 1e-5, [0] * 6, u_val, [2] * 6, solver=1, g=(0, 0, -9.81), n_outer_correctors=2, n_correctors=2, p_max_iter=5000, **turb, **gkw, **kw)
    y = g.get("nearWallDist")
    b = boundary_faces(mesh, wall)
    dc = g.geometry("dcNO")[len(mesh["neighbour"]):]
    close(y[b], 1.0 / dc[b], 1e-13, "nearWallDist = n . (Cf - C)")
    if variant != "kEpsilon_graded":
        close(y[b], np.full(len(b), dx / 2), 1e-13, "nearWallDist = h / 2")
    assert not y[boundary_faces(mesh, [5])].any()
    f.hold_sources(True)
    rs = np.random.RandomState(17)
    for step in range(3):
        f.set_particles(bed_particles(rs, 3000, box, dx))
        f.step()
        g.set("alpha", f.get("alpha")); g.set("uSourceDrag", f.get("uSourceDrag")); g.set("uSource", f.get("uSource"))
        g.step()
        if variant != "kEqn":
            close(g.get("epsilon"), f.get("epsilon"), 1e-6, "epsilon step %d" % step)
        close(g.get("k"), f.get("k"), 1e-6, "k step %d" % step)
        close(g.get("nut"), f.get("nut"), 1e-6, "nut step %d" % step)
        close(g.get("U").reshape(-1, 3), f.get("U").reshape(-1, 3), 1e-6, "U step %d" % step)
    assert not np.allclose(f.get("k"), 5e-3, rtol=1e-3)
    nb = g.get("nut_boundary")[b]
    assert nb.max() > 0                                                         # (the wall value above yPlusLam somewhere)
    f.close(); g.close()


def merge_patches(mesh, a, b):
    """the mesh with patch b's faces moved behind patch a's and the two made one patch (numbered a; the later patches move down by one)"""
    ni = len(mesh["neighbour"])
    ps, pz = list(mesh["patch_start"]), list(mesh["patch_size"])
    groups = [list(range(ps[q], ps[q] + pz[q])) for q in range(len(ps))]
    groups[a] += groups[b]
    del groups[b]
    order = list(range(ni)) + [f for g in groups for f in g]
    off, fp = np.asarray(mesh["face_offsets"]), np.asarray(mesh["face_points"])
    out = dict(mesh)
    out["face_points"] = np.concatenate([fp[off[f]:off[f + 1]] for f in order]).astype(np.int32)
    out["face_offsets"] = np.concatenate([[0], np.cumsum([off[f + 1] - off[f] for f in order])]).astype(np.int32)
    out["owner"] = np.asarray(mesh["owner"])[order]
    out["patch_size"] = np.array([len(g) for g in groups], np.int32)
    out["patch_start"] = (ni + np.concatenate([[0], np.cumsum(out["patch_size"])[:-1]])).astype(np.int32)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["wavy_hex", "prisms", "tets"])
def test_near_wall_dist_on_skewed_cells_equals_the_restatement(prod, kind):  # noqa: F811
    """nearWallDist against the restatement above on wavy hexahedra, prisms (triangles and quadrilaterals on the walls) and Kuhn tetrahedra -- there with xmin and ymax
    one patch, so that a cell along their edge has two faces on one wall patch and cells have W > 1 wall faces"""
    box = 0.1
    vm = pm.wavy(0.003, (box, box, box))
    mesh = {"wavy_hex": lambda: pm.hex_block(6, 5, 4, (box, box, box), vm, renumber_seed=3), "prisms": lambda: pm.prism_block(5, 4, 3, (box, box, box), vm),
            "tets": lambda: merge_patches(pm.tet_block(3, 3, 3, (box, box, box), vm), 0, 3)}[kind]()
    npat = len(mesh["patch_start"])
    wall = list(range(npat - 1))
    s = prod.LduSolver(mesh, 1e-4, 1e-5, [0] * npat, [(0, 0, 0)] * npat, [2] * npat, solver=1, nut_bc=[WF] * (npat - 1) + [0], eps_bc=[WF] * (npat - 1) + [0], **RAS)
    y = s.get("nearWallDist")
    ref = near_wall_dist(mesh, s.geometry("C"), wall)
    b = boundary_faces(mesh, wall)
    assert len(y) == len(ref) and (ref[b] > 0).all() and not y[boundary_faces(mesh, [npat - 1])].any()
    np.testing.assert_allclose(y, ref, rtol=1e-12, atol=0)
    if kind == "tets":
        own = np.asarray(mesh["owner"])[b + len(mesh["neighbour"])]
        pa = np.searchsorted(np.asarray(mesh["patch_start"]), b + len(mesh["neighbour"]), side="right") - 1
        assert np.bincount(own).max() > 1                                     # W > 1
        assert len(set(zip(own.tolist(), pa.tolist()))) < len(own)             # a cell with two faces on one patch
    s.close()


def wall_cells(mesh, patches):
    ni = len(mesh["neighbour"])
    b = boundary_faces(mesh, patches)
    own = np.asarray(mesh["owner"])[b + ni]
    return b, own


@pytest.mark.gpu
def test_wall_function_invariants_on_a_wavy_mesh_with_a_cloud(prod):  # noqa: F811
    """kEpsilon with the wall functions on five sides of a wavy box, relaxation, upwind, a cloud: after each step epsilon in every wall cell is the average over its wall
    faces of Cmu^3/4 k^3/2 / (kappa y) with the k of the step's start; nut on the wall faces is nutkWallFunction's on the k after the step (the file's value before the
    first); k, epsilon > 0, continuity closes; the zero-gradient case differs; without a cloud two runs agree bit for bit"""
    n, box = 10, 0.1
    dx = box / n
    mesh = pm.hex_block(n, n, n, (box, box, box), pm.wavy(0.2 * dx, (box, box, box)), renumber_seed=8)
    wall = [0, 1, 2, 3, 4]
    nu, kappa, E, cmu = 1e-6, 0.4, 9.0, RAS["ras_cmu"]
    lidv = [(0, 0, 0)] * 6
    lidv[3] = (0.3, 0, 0.1)
    kw = dict(solver=1, g=(0, 0, -9.81), n_non_orth=1, n_outer_correctors=2, n_correctors=2, p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10, p_max_iter=5000,
              u_relax=0.8, u_relax_final=1.0, p_relax=0.7, p_relax_final=1.0, wf_kappa=kappa, wf_E=E, **RAS)
    nut_file = [2e-5 if q in wall else 0.0 for q in range(6)]
    wfkw = dict(nut_bc=[WF if q in wall else 0 for q in range(6)], nut_val=nut_file, eps_bc=[WF if q in wall else 0 for q in range(6)], eps_val=[0.0] * 6)

    def run(patches, cloud, steps=3, check=False):
        s = prod.LduSolver(mesh, 2e-4, nu, [0] * 6, lidv, [2] * 6, **patches, **kw)
        s.hold_sources(True)
        rs = np.random.RandomState(23)
        b, own = wall_cells(mesh, wall)
        y = s.get("nearWallDist")[b]
        ypl = 11.0
        for _ in range(10):
            ypl = np.log(max(E * ypl, 1.0)) / kappa
        if check:
            nb0 = s.get("nut_boundary")
            np.testing.assert_array_equal(nb0[b], 2e-5)
        for step in range(steps):
            if cloud:
                s.set_particles(bed_particles(rs, 1500, box, dx))
            kb = s.get("k")
            s.step()
            if not check:
                continue
            k, e = s.get("k"), s.get("epsilon")
            W = np.bincount(own, minlength=len(k))
            ew = np.bincount(own, weights=cmu ** 0.75 * kb[own] ** 1.5 / (kappa * y), minlength=len(k))
            cells = np.unique(own)
            np.testing.assert_allclose(e[cells], ew[cells] / W[cells], rtol=1e-12, atol=0, err_msg="epsilon in the wall cells, step %d" % step)
            yp = cmu ** 0.25 * y * np.sqrt(k[own]) / nu
            nutw = np.where(yp > ypl, nu * (yp * kappa / np.log(E * yp) - 1.0), 0.0)
            assert (nutw > 0).any()
            np.testing.assert_allclose(s.get("nut_boundary")[b], nutw, rtol=1e-12, atol=1e-300, err_msg="nut_w, step %d" % step)
            assert k.min() > 0 and e.min() > 0
            assert abs(s.stats()["cont_err_sum_local"]) < 1e-8
        out = {q: s.get(q) for q in ("U", "p", "k", "epsilon", "nut")}
        s.close()
        return out

    a = run(wfkw, True, check=True)
    zg = run(dict(nut_bc=[0] * 6, eps_bc=[0] * 6), True)
    assert not np.allclose(a["epsilon"], zg["epsilon"], rtol=1e-3)
    r1, r2 = run(wfkw, False), run(wfkw, False)
    for q in r1:
        np.testing.assert_array_equal(r1[q], r2[q], err_msg=q)


@pytest.mark.gpu
def test_foamYadeHip_runs_a_general_case_with_wall_functions(prod, tmp_path):  # noqa: F811
    """foamYadeHip -solver pimple on the wavy bed with nutkWallFunction / epsilonWallFunction / kqRWallFunction on its walls: runs controlDict's steps, exits 0, writes
    nut.water, k.water and epsilon.water with the walls' wall-function entries"""
    dst, _ = wf_bed(tmp_path)
    exe = os.path.join(os.path.dirname(prod.__file__), "bin", "foamYadeHip")
    out = subprocess.run([exe, "-solver", "pimple", "-case", str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "general polyhedral mesh" in out.stdout and out.stdout.rstrip().endswith("End")
    for nm, ty in (("nut.water", "nutkWallFunction"), ("k.water", "kqRWallFunction"), ("epsilon.water", "epsilonWallFunction")):
        t = (dst / "0.002" / nm).read_text()
        assert ty in t and "walls" in t and "nonuniform" in t, nm
    assert "kappa" in (dst / "0.002/nut.water").read_text()
    e = (dst / "0.002/epsilon.water").read_text()
    assert "nan" not in e.lower()
