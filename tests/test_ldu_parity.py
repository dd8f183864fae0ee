"""fy_ldu_solver (icoFoamYade's loop body on a general polyhedral mesh, HIP: csrc/ldu_*.{cpp,hip}) against oracle/ldu_oracle.cpp, the CPU restatement, and
against the structured HIP solver on a lattice.  FV parity is unpinned (OpenFOAM-6 is not here): what the restatement itself is held to is in
tests/test_ldu_oracle.py.  Tolerances: geometry 1e-13; matrices of the first step 1e-10; fields after a few steps 2e-6 (both sides converge the same
linear systems to their tolerances with the same algorithms, summed in another order).

What is held to ROUNDING is in tests/test_ldu_sweeps_parity.py: with every iteration count frozen the kernels of ldu_kernels.hip and the driver are compared field by
field with this restatement compiled in long double, within 50 x the double restatement's own distance from it (tests/ldu_sweep_cases.py: mesh kinds, convection
schemes, patches, loop counts, closures).  This file keeps the converged runs: more steps, larger meshes, the multigrid preconditioner, the cloud on each mesh kind."""
import numpy as np
import pytest

import poly_meshes as pm

pytestmark = pytest.mark.gpu


def pair(product, oracle, mesh, dt, nu, u_bc, u_val, p_bc, p_val=None, **kw):
    okw = dict(kw)
    h = product.LduSolver(mesh, dt, nu, u_bc, u_val, p_bc, p_val, **kw)
    o = oracle.LduSolver(mesh, dt, nu, u_bc, u_val, p_bc, p_val, **okw)
    return h, o


def close(a, b, rtol, what):
    sc = np.abs(b).max() + 1e-300
    assert np.abs(a - b).max() <= rtol * sc, (what, np.abs(a - b).max() / sc)


def lid(n_patches=6, lid_patch=3):
    v = [(0, 0, 0)] * n_patches
    v[lid_patch] = (1.0, 0, 0)
    return v


def test_geometry_equals_the_restatement(product, oracle):
    mesh = pm.hex_block(5, 4, 6, (1.0, 0.8, 1.2), pm.wavy(0.04, (1.0, 0.8, 1.2)), renumber_seed=4)
    h, o = pair(product, oracle, mesh, 1e-3, 0.01, [0] * 6, lid(), [0] * 6)
    for nm in ("C", "V", "Cf", "Sf", "magSf", "w", "dcNO", "kvec"):
        np.testing.assert_allclose(h.geometry(nm), o.geometry(nm), rtol=0, atol=1e-13, err_msg=nm)
    h.close(); o.close()


@pytest.mark.parametrize("kind", ["lattice", "sheared", "wavy_renumbered", "prisms", "tetrahedra", "wavy_upwind", "wavy_linear_upwind", "wavy_vanLeer", "wavy_limitedLinear"])
def test_cavity_matches_the_restatement(product, oracle, kind):
    """lid-driven cavity, four steps, two non-orthogonal correctors: first-step matrices, then fields and counters.  prisms: triangular prisms on a wavy
    lattice (triangular and quadrilateral faces, five-faced cells)"""
    n = 10
    vm, seed = {"lattice": (None, None), "sheared": (pm.shear(0.3, 0.0, 0.2), None), "wavy_renumbered": (pm.wavy(0.03), 9), "prisms": (pm.wavy(0.02), None), "tetrahedra": (None, None),
                "wavy_upwind": (pm.wavy(0.03), 9), "wavy_linear_upwind": (pm.wavy(0.03), 9), "wavy_vanLeer": (pm.wavy(0.03), 9),
                "wavy_limitedLinear": (pm.wavy(0.03), 9)}[kind]
    if kind == "tetrahedra":            # Kuhn tetrahedra on a wavy lattice: triangles only, four-faced cells, non-orthogonality around 50 degrees
        mesh = pm.tet_block(6, 6, 5, vertex_map=pm.wavy(0.02))
    else:
        mesh = pm.prism_block(n, n, 6, vertex_map=vm) if kind == "prisms" else pm.hex_block(n, n, n, vertex_map=vm, renumber_seed=seed)
    kw = dict(n_non_orth=2, p_tol=1e-9, p_rel_tol=0.0, p_final_tol=1e-9, u_tol=1e-9, p_max_iter=5000)
    if kind.startswith("wavy_") and kind != "wavy_renumbered":          # Gauss upwind / linearUpwind grad(U) / vanLeer / limitedLinear 0.5
        kw["convection_scheme"] = {"wavy_upwind": 1, "wavy_linear_upwind": 2, "wavy_vanLeer": 4, "wavy_limitedLinear": 3}[kind]
        kw["convection_limiter_k"] = 0.5
    h, o = pair(product, oracle, mesh, 0.4 / n, 0.01, [0] * 6, lid(), [0] * 6, **kw)
    U0 = np.random.RandomState(3).rand(mesh["n_cells"], 3) * 0.05
    h.set("U", U0); o.set("U", U0)
    h.step(); o.step()
    ni = len(mesh["neighbour"])
    close(h.get("mom_lower"), o.get("mom_lower"), 1e-10, "lower"); close(h.get("mom_upper"), o.get("mom_upper"), 1e-10, "upper")
    close(h.get("p_coef")[:ni], o.get("p_coef")[:ni], 1e-8, "p_coef")
    for _ in range(3):
        h.step(); o.step()
    sh, so = h.stats(), o.stats()
    assert abs(sh["p_iters_total"] - so["p_iters_total"]) <= max(3, so["p_iters_total"] // 20) and abs(sh["u_iters_total"] - so["u_iters_total"]) <= 1
    assert sh["courant_max"] == pytest.approx(so["courant_max"], rel=1e-6)
    close(h.get("U"), o.get("U"), 2e-6, "U")
    ph, po = h.get("p"), o.get("p")
    close(ph - ph.mean(), po - po.mean(), 1e-5, "p")
    close(h.get("phi"), o.get("phi"), 5e-6, "phi")
    h.close(); o.close()


def test_through_flow_with_fixed_pressure_and_a_momentum_source(product, oracle):
    """inlet fixedValue U, outlet fixedValue p, zeroGradient elsewhere on the in/outlet pair, walls, and an external momentum source: every boundary branch"""
    mesh = pm.hex_block(8, 6, 4, (2.0, 1.0, 0.5), pm.wavy(0.03, (2.0, 1.0, 0.5)), patches=[("inlet", [0]), ("outlet", [1]), ("walls", [2, 3]), ("sides", [4, 5])], renumber_seed=1)
    kw = dict(n_non_orth=1, p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10, p_max_iter=5000)
    h, o = pair(product, oracle, mesh, 0.05, 0.02, [0, 1, 0, 1], [(0.5, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)], [0, 1, 0, 0], [0, 0.0, 0, 0], **kw)
    src = np.random.RandomState(8).standard_normal((mesh["n_cells"], 3)) * 0.3
    for _ in range(5):
        h.step(src); o.step(src)
    close(h.get("U"), o.get("U"), 2e-6, "U"); close(h.get("p"), o.get("p"), 1e-5, "p"); close(h.get("phi"), o.get("phi"), 5e-6, "phi")
    assert h.stats()["cont_err_sum_local"] < 1e-10
    h.close(); o.close()


def test_lattice_block_equals_the_structured_hip_solver(product):
    """the same cavity through both HIP solvers: fy_solver on the block (Jacobi-preconditioned PCG) and fy_ldu_solver on the block written as a polyhedral mesh"""
    n = 12
    mesh = pm.hex_block(n, n, n, renumber_seed=6)
    g = product.LduSolver(mesh, 0.4 / n, 0.01, [0] * 6, lid(), [0] * 6, p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10, p_max_iter=5000)
    case = product.make_case(0, n, n, n, 1.0 / n, 0.4 / n, 0.01, u_bc=[0] * 6, u_val=lid(), p_solver=0, p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10)
    f = product.Solver(case)
    U0 = np.random.RandomState(2).rand(n ** 3, 3) * 0.05
    f.set("U", U0)
    Ug = np.zeros_like(U0); Ug[mesh["perm"]] = U0
    g.set("U", Ug)
    for _ in range(4):
        f.step(); g.step()
    Uf = f.get("U").reshape(-1, 3)
    close(pm.to_lattice(mesh, g.get("U").reshape(-1, 3)), Uf, 1e-7, "U")
    pf, pg = f.get("p"), pm.to_lattice(mesh, g.get("p"))
    close(pg - pg.mean(), pf - pf.mean(), 1e-6, "p")
    f.close(); g.close()


def test_point_force_coupling_on_a_general_mesh(product, oracle):
    """mesh.findCell (FoamYade.C:251) on a non-lattice mesh = nearest centre + a walk across faces: every particle lands in a cell one of whose face-fan tetrahedra
    holds it (OpenFOAM's CELL_TETS decomposition, checked by brute force in long double from the mesh dictionary: tests/find_cell_ref.py -- the half-spaces through
    Cf along Sf, which this test used before, do not tile a mesh with warped faces: 13 of these 2 243 interior points lie in another cell by them), particles outside
    the mesh are not found, and the Stokes drag / torque and the momentum source follow FoamYade.C:437-453 from that cell's U and grad U.  The adversarial inputs
    (vertices, faces, other cell shapes, cyclic halves) are tests/test_ldu_find_cell.py's"""
    import find_cell_ref as fr
    n = 8
    mesh = pm.hex_block(n, n, n, vertex_map=pm.wavy(0.04), renumber_seed=12)
    nu, rho = 0.01, 1000.0
    s = product.LduSolver(mesh, 1e-3, nu, [0] * 6, lid(), [0] * 6, rho_f=rho)
    U0 = np.random.RandomState(4).rand(n ** 3, 3) * 0.2
    s.set("U", U0)
    rs = np.random.RandomState(5)
    npart = 3000
    rec = np.zeros((npart, 10))
    rec[:, 0:3] = rs.random_sample((npart, 3)) * 1.1 - 0.05          # some of them outside the unit box
    rec[:, 3:9] = rs.standard_normal((npart, 6)) * 0.1
    rec[:, 9] = 0.01
    s.set_particles(rec)
    # the step's grad U is that of U0; the source is consumed by the step, so look at the forces
    s.step()
    F, found, cells = s.forces(), s.found(), s.particle_cells()
    inside_box = np.all((rec[:, 0:3] > 1e-9) & (rec[:, 0:3] < 1 - 1e-9), axis=1)
    assert np.all(found[inside_box] == 1) and np.all(found[~inside_box & np.any((rec[:, 0:3] < -1e-9) | (rec[:, 0:3] > 1 + 1e-9), axis=1)] == -1)
    o = oracle.LduSolver(mesh, 1e-3, nu, [0] * 6, lid(), [0] * 6)
    ref = fr.FindCellRef(mesh, o.geometry("C"))
    o.close()
    # brute force: the cell with a tetrahedron that holds the point (exactly one for each of these points)
    idx = np.where(inside_box)[0]
    holds = ref.cells_of(rec[idx, 0:3])
    assert all(len(h) == 1 for h in holds)
    for i, h in zip(idx, holds):
        c = int(cells[i])
        assert c in h
        dia = 2 * rec[i, 9]
        drag = 3 * np.pi * dia * nu * rho * (U0[c] - rec[i, 3:6])
        np.testing.assert_allclose(F[i, 0:3], drag, rtol=1e-10, atol=1e-16)
    s.close()


@pytest.mark.parametrize("kind", ["wavy", "prisms", "sheared_renumbered", "tetrahedra"])
def test_multigrid_preconditioned_pcg_solves_the_same_equations(product, oracle, kind):
    """p_solver = FY_PSOLVER_PCG_MG (fvSolution: GAMG): the agglomeration V-cycle changes the path to the solution, not the solution -- with the linear
    systems converged to 1e-10 the fields equal the restatement's (which runs PCG with the diagonal preconditioner), in far fewer iterations"""
    n = 12
    if kind == "prisms":
        mesh = pm.prism_block(n, n, 8, vertex_map=pm.wavy(0.02))
    elif kind == "tetrahedra":
        mesh = pm.tet_block(7, 7, 6, vertex_map=pm.wavy(0.02))
    else:
        mesh = pm.hex_block(n, n, n, vertex_map=pm.wavy(0.03) if kind == "wavy" else pm.shear(0.3, 0.1, 0.2), renumber_seed=None if kind == "wavy" else 21)
    kw = dict(n_non_orth=1, p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10, p_max_iter=5000)
    h = product.LduSolver(mesh, 0.4 / n, 0.01, [0] * 6, lid(), [0] * 6, p_solver=product.FY_PSOLVER_PCG_MG, **kw)
    o = oracle.LduSolver(mesh, 0.4 / n, 0.01, [0] * 6, lid(), [0] * 6, **kw)
    ih = io = 0
    for _ in range(3):
        h.step(); o.step()
        ih += h.stats()["p_iters_total"]; io += o.stats()["p_iters_total"]
    assert ih * 4 < io, (ih, io)
    close(h.get("U"), o.get("U"), 1e-7, "U")
    ph, po = h.get("p"), o.get("p")
    close(ph - ph.mean(), po - po.mean(), 1e-6, "p")
    h.close(); o.close()


def test_the_vcycle_is_a_symmetric_positive_definite_contraction(product):
    """what PCG needs of its preconditioner: (M^-1 a).b = (M^-1 b).a, a.M^-1 a > 0; and what makes it worth its cost: the error of one cycle,
    e - M^-1 A e, is a fraction of e in the energy norm for smooth and for rough e alike"""
    n = 16
    mesh = pm.hex_block(n, n, n, vertex_map=pm.wavy(0.03), renumber_seed=None)
    h = product.LduSolver(mesh, 0.4 / n, 0.01, [0] * 6, lid(), [0] * 6, p_solver=product.FY_PSOLVER_PCG_MG, n_non_orth=1)
    h.step()
    # the pairwise passes stack into 2 x 2 x 2 boxes on a (mildly distorted) lattice: the face areas differ by a few per cent there and count as ties
    assert h.mg_levels() == [(4096, 6), (512, 6), (64, 6)]
    rs = np.random.RandomState(8)
    a, b = rs.standard_normal(n ** 3), rs.standard_normal(n ** 3)
    Ma, Mb = h.apply("p_precondition", a), h.apply("p_precondition", b)
    assert abs(Ma @ b - Mb @ a) <= 1e-12 * (np.abs(Ma) @ np.abs(b)) and Ma @ a > 0 and Mb @ b > 0
    Aa, Ab = h.apply("p_matrix", a), h.apply("p_matrix", b)
    assert abs(Aa @ b - Ab @ a) <= 1e-12 * (np.abs(Aa) @ np.abs(b)) and Aa @ a > 0
    C = h.geometry("C")
    smooth = np.cos(np.pi * C[:, 0]) * np.cos(np.pi * C[:, 1]) * np.cos(2 * np.pi * C[:, 2])
    for e in (smooth, a):
        Ae = h.apply("p_matrix", e)
        e1 = e - h.apply("p_precondition", Ae)
        ratio = np.sqrt((e1 @ h.apply("p_matrix", e1)) / (e @ Ae))
        assert ratio < 0.6, ratio
    h.close()


def bed_particles(rs, npart, box, dx):
    rec = np.zeros((npart, 10))
    rec[:, 0:3] = rs.random_sample((npart, 3)) * np.array([box, box, 0.6 * box]) + np.array([0.0, 0.0, 0.05 * box])
    rec[:, 3:6] = 0.05 * rs.standard_normal((npart, 3))
    rec[:, 9] = 0.2 * dx
    return rec


@pytest.mark.parametrize("n_outer,relax,adjust,les", [(1, 0.0, 0, 0), (2, 0.7, 0, 0), (1, 0.0, 1, 0), (2, 0.0, 0, 1), (1, 0.0, 0, 2), (2, 0.0, 0, 3), (1, 0.0, 0, 6)])
def test_pimple_on_a_lattice_equals_the_structured_hip_solver(product, n_outer, relax, adjust, les):
    """pimpleFoamYade's equations (void-fraction-weighted UcEqn / pEqn, gravity, fixedFluxPressure walls, PIMPLE outer correctors, relaxation) through both HIP
    solvers: fy_solver on the block with particles, and fy_ldu_solver on the block written as a polyhedral mesh, fed the void fraction and the momentum sources the
    first one's coupling produced (the two k-d trees differ where a lattice's centres tie, so a cloud does not take the same improvement chains in both: the
    coupling on a general mesh is pinned by the graded-mesh goldens; here the equations are compared).  Velocity, pressure and flux over three steps"""
    n, box = 10, 0.1
    dx = box / n
    mesh = pm.hex_block(n, n, n, (box, box, box))
    kw = dict(p_tol=1e-11, p_rel_tol=0.0, p_final_tol=1e-11, u_tol=1e-11)
    rel = dict(u_relax=relax, u_relax_final=1.0 if relax else 0.0, p_relax=0.6 if relax else 0.0, p_relax_final=1.0 if relax else 0.0,
               adjust_time_step=adjust, max_co=0.4, max_delta_t=3.2e-4)          # (setDeltaT.H: the step grows by 1.2 per step while the Courant number allows)
    if les == 1:                                         # LES Smagorinsky
        rel.update(turbulence_model=1, nut_initial=3e-5, les_delta_coeff=0.8)
    if les >= 2:                                         # (the last variants: Gauss upwind, linearUpwind, MUSCL)
        rel.update(convection_scheme=les - 1)
    case = product.make_case(1, n, n, n, dx, 2e-4, 1e-5, g=(0, 0, -9.81), p_bc=[2] * 6, p_solver=0, n_outer_correctors=n_outer, n_correctors=2, p_max_iter=5000, **rel, **kw)
    f = product.Solver(case)
    f.hold_sources(True)
    h = product.LduSolver(mesh, 2e-4, 1e-5, [0] * 6, [(0, 0, 0)] * 6, [2] * 6, solver=1, g=(0, 0, -9.81), n_outer_correctors=n_outer, n_correctors=2, p_max_iter=5000, **rel, **kw)
    rs = np.random.RandomState(17)
    for step in range(3):
        f.set_particles(bed_particles(rs, 2000, box, dx))
        f.step()
        alpha = f.get("alpha")
        assert alpha.min() < 0.9
        h.set("alpha", alpha); h.set("uSourceDrag", f.get("uSourceDrag")); h.set("uSource", f.get("uSource"))
        h.step()
        close(h.get("U").reshape(-1, 3), f.get("U").reshape(-1, 3), 1e-6, "U step %d" % step)
        assert h.stats()["delta_t"] == f.stats()["delta_t"] and (f.stats()["delta_t"] > 2e-4) == bool(adjust)
    pf, ph = f.get("p"), h.get("p")
    close(ph - ph.mean(), pf - pf.mean(), 1e-6, "p")
    assert np.abs(f.get("U")).max() > 1e-4
    if les == 1:
        close(h.get("nut"), f.get("nut"), 1e-6, "nut")
        assert not np.allclose(f.get("nut"), 3e-5)
    f.close(); h.close()


def test_pimple_with_particles_on_a_wavy_mesh_conserves_what_it_should(product):
    """Gaussian 4-way coupling on a non-orthogonal mesh: every particle inside is found, the void fraction removes the particles' volume (up to the reference's chain quirks),
    continuity closes, and a closed box at rest under gravity stays at rest up to the skewness error"""
    n, box = 10, 0.1
    dx = box / n
    mesh = pm.hex_block(n, n, n, (box, box, box), pm.wavy(0.2 * dx, (box, box, box)), renumber_seed=4)
    h = product.LduSolver(mesh, 2e-4, 1e-5, [0] * 6, [(0, 0, 0)] * 6, [2] * 6, solver=1, g=(0, 0, -9.81), n_non_orth=1, n_correctors=2, p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10,
                          u_tol=1e-10, p_max_iter=5000, p_solver=product.FY_PSOLVER_PCG_MG)
    h.hold_sources(True)
    for _ in range(2):                                   # no particles: gravity against the pressure gradient.  On a skewed mesh the balance is discrete only up to the
        h.step()                                         # lagged non-orthogonal correction: spurious velocities three orders under g dt = 2e-3 m/s (zero on a lattice)
    assert np.abs(h.get("U")).max() < 1e-5
    rs = np.random.RandomState(3)
    rec = bed_particles(rs, 1500, box, dx)
    h.set_particles(rec)
    h.step()
    assert np.all(h.found() == 1)
    V = h.geometry("V")
    pvol = (4.0 / 3.0) * np.pi * rec[:, 9] ** 3
    dep = ((1.0 - h.get("alpha")) * V).sum()             # the deposited volume: the cloud's, less the particles the improvement chain leaves without a stencil (quirk Q2)
    assert 0.97 * pvol.sum() < dep <= pvol.sum() * (1 + 1e-12)
    st = h.stats()
    assert st["cont_err_sum_local"] < 1e-9 and np.abs(h.get("U")).max() > 1e-5
    h.close()


@pytest.mark.parametrize("kind", ["wavy_renumbered", "prisms", "wavy_les"])
def test_pimple_with_a_cloud_matches_the_restatement(product, oracle, kind):
    """pimpleFoamYade on non-orthogonal meshes, HIP against the CPU restatement: the HIP solver runs the coupled step with its cloud; the restatement is given the
    void fraction, the drag coefficient and the explicit source that coupling left and solves the same equations.  Compared: the coupling's input fields
    (ddtU_f, divT, gradP: corrected laplacian and gradients on skewed cells), velocity, pressure, flux -- two outer correctors, relaxation, one non-orthogonal pass"""
    n, box = 10, 0.1
    dx = box / n
    if kind == "prisms":
        mesh = pm.prism_block(n, n, 6, (box, box, box), pm.wavy(0.15 * dx, (box, box, box)))
    else:
        mesh = pm.hex_block(n, n, n, (box, box, box), pm.wavy(0.2 * dx, (box, box, box)), renumber_seed=8)
    npatch = 6
    kw = dict(p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10, p_max_iter=5000)
    if kind == "wavy_les":                                # LES Smagorinsky on skewed cells (delta from each cell's volume), one patch with a fixed nut
        kw.update(turbulence_model=1, nut_initial=2e-5, les_delta_coeff=1.0, nut_bc=[0, 0, 0, 1, 0, 0], nut_val=[0, 0, 0, 4e-5, 0, 0])
    rel = dict(u_relax=0.8, u_relax_final=1.0, p_relax=0.7, p_relax_final=1.0)
    lidv = [(0, 0, 0)] * npatch
    lidv[3] = (0.05, 0, 0)                                # a moving wall too, so that the velocity gradients are not the cloud's alone
    h = product.LduSolver(mesh, 2e-4, 1e-5, [0] * npatch, lidv, [2] * npatch, solver=1, g=(0, 0, -9.81), n_non_orth=1, n_outer_correctors=2, n_correctors=2, **rel, **kw)
    o = oracle.LduSolver(mesh, 2e-4, 1e-5, [0] * npatch, lidv, [2] * npatch, solver=1, g=(0, 0, -9.81), n_non_orth=1, n_outer=2, n_correctors=2, **rel, **kw)
    h.hold_sources(True)
    rs = np.random.RandomState(23)
    for step in range(3):
        h.set_particles(bed_particles(rs, 1500, box, dx))
        h.step()
        alpha = h.get("alpha")
        assert alpha.min() < 0.95
        o.step(source=h.get("uSourceCoupling"), alpha=alpha, drag=h.get("uSourceDrag"))
        if step == 2:
            for nm in ("ddtU", "divT", "gradP"):
                close(h.get(nm), o.get(nm), 1e-6, nm)
        close(h.get("U"), o.get("U"), 2e-6, "U step %d" % step)
    ph, po = h.get("p"), o.get("p")
    close(ph - ph.mean(), po - po.mean(), 1e-5, "p")
    close(h.get("phi"), o.get("phi"), 1e-5, "phi")
    if kind == "wavy_les":
        close(h.get("nut"), o.get("nut"), 1e-6, "nut")
    assert np.abs(h.get("ddtU")).max() > 0 and np.abs(h.get("divT")).max() > 0
    h.close(); o.close()


def _turn(a=0.5, b=-0.35, c=0.8):
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


@pytest.mark.parametrize("kind", ["ico_oblique_wavy", "pimple_cloud", "pimple_les_oblique"])
def test_symmetry_sides_match_the_restatement(product, oracle, kind):
    """symmetryPlane / symmetry / slip patches (FY_BC_U_SLIP) on the HIP solver against the restatement: a wavy cavity turned in space (every face of a symmetry patch with
    its own oblique normal: per-component boundary diagonal (|n_x|, |n_y|, |n_z|) deltaCoeffs, explicit remainder, A() with their average, H() with the rest), and
    pimpleFoamYade with a cloud, relaxation (cmptMax / cmptMin of the vector coefficient in fvMatrix::relax) and two outer correctors"""
    n, box = 10, 0.1
    dx = box / n
    u_bc = [2, 2, 2, 0, 0, 0]
    kw = dict(p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10, p_max_iter=5000)
    R = _turn()
    if kind == "ico_oblique_wavy":
        wv = pm.wavy(0.03)
        mesh = pm.hex_block(n, n, n, vertex_map=lambda P: wv(P) @ R.T, renumber_seed=12)
        u_val = [(0, 0, 0)] * 6
        u_val[3] = tuple(R @ np.array([1.0, 0, 0.3]))
        h, o = pair(product, oracle, mesh, 0.4 / n, 0.01, u_bc, u_val, [0] * 6, n_non_orth=2, **kw)
        U0 = np.random.RandomState(3).rand(mesh["n_cells"], 3) * 0.05
        h.set("U", U0); o.set("U", U0)
        for _ in range(4):
            h.step(); o.step()
        Sf, ni = h.geometry("Sf"), len(mesh["neighbour"])
        sl = np.concatenate([np.arange(mesh["patch_start"][q], mesh["patch_start"][q] + mesh["patch_size"][q]) for q in range(3)])
        assert np.abs(Sf[sl] / np.linalg.norm(Sf[sl], axis=1)[:, None]).max() < 0.97 and sl.min() >= ni
        assert np.abs(h.get("phi")[sl]).max() < 1e-15 and np.abs(h.get("U")).max() > 0.1
    else:
        les = kind == "pimple_les_oblique"
        vm = pm.wavy(0.2 * dx, (box, box, box))
        mesh = pm.hex_block(n, n, n, (box, box, box), (lambda P: vm(P) @ R.T) if les else vm, renumber_seed=8)
        gv = tuple(R @ np.array([0, 0, -9.81])) if les else (0, 0, -9.81)
        if les:
            kw.update(turbulence_model=1, nut_initial=2e-5, les_delta_coeff=1.0)
        rel = dict(u_relax=0.8, u_relax_final=1.0, p_relax=0.7, p_relax_final=1.0)
        lidv = [(0, 0, 0)] * 6
        lidv[3] = tuple(R @ np.array([0.05, 0, 0.02])) if les else (0.05, 0, 0.02)
        p_bc = [0, 0, 0, 2, 2, 2]                          # (gravity along the symmetry sides: x and ymin)
        h = product.LduSolver(mesh, 2e-4, 1e-5, u_bc, lidv, p_bc, solver=1, g=gv, n_non_orth=1, n_outer_correctors=2, n_correctors=2, **rel, **kw)
        o = oracle.LduSolver(mesh, 2e-4, 1e-5, u_bc, lidv, p_bc, solver=1, g=gv, n_non_orth=1, n_outer=2, n_correctors=2, **rel, **kw)
        h.hold_sources(True)
        rs = np.random.RandomState(29)
        for step in range(3):
            rec = bed_particles(rs, 1500, box, dx)
            if les:
                rec[:, 0:3] = rec[:, 0:3] @ R.T; rec[:, 3:6] = rec[:, 3:6] @ R.T
            h.set_particles(rec)
            h.step()
            alpha = h.get("alpha")
            assert alpha.min() < 0.95
            o.step(source=h.get("uSourceCoupling"), alpha=alpha, drag=h.get("uSourceDrag"))
            close(h.get("U"), o.get("U"), 2e-6, "U step %d" % step)
        if les:
            close(h.get("nut"), o.get("nut"), 1e-6, "nut")
    ph, po = h.get("p"), o.get("p")
    close(ph - ph.mean(), po - po.mean(), 1e-5, "p")
    close(h.get("phi"), o.get("phi"), 1e-5, "phi")
    close(h.get("U"), o.get("U"), 2e-6, "U")
    h.close(); o.close()


@pytest.mark.parametrize("solver", ["ico", "pimple"])
def test_symmetry_sides_on_a_lattice_equal_the_structured_hip_solver(product, solver):
    """the same cavity with three symmetry sides through both HIP solvers"""
    n = 12
    u_bc = [2, 2, 2, 0, 0, 0]
    u_val = [(0, 0, 0)] * 6
    u_val[3] = (1.0, 0, 0.3)
    mesh = pm.hex_block(n, n, n, renumber_seed=6)
    tol = dict(p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10)
    if solver == "ico":
        g = product.LduSolver(mesh, 0.4 / n, 0.01, u_bc, u_val, [0] * 6, p_max_iter=5000, **tol)
        f = product.Solver(product.make_case(0, n, n, n, 1.0 / n, 0.4 / n, 0.01, u_bc=u_bc, u_val=u_val, p_solver=0, **tol))
    else:
        rel = dict(u_relax=0.7, u_relax_final=1.0, p_relax=0.6, p_relax_final=1.0)
        p_bc = [0, 0, 0, 2, 2, 2]
        g = product.LduSolver(mesh, 0.4 / n, 0.01, u_bc, u_val, p_bc, solver=1, g=(0, 0, -9.81), n_outer_correctors=2, n_correctors=2, p_max_iter=5000, **rel, **tol)
        f = product.Solver(product.make_case(1, n, n, n, 1.0 / n, 0.4 / n, 0.01, g=(0, 0, -9.81), u_bc=u_bc, u_val=u_val, p_bc=p_bc, p_solver=0, n_outer_correctors=2, n_correctors=2, p_max_iter=5000, **rel, **tol))
    U0 = np.random.RandomState(2).rand(n ** 3, 3) * 0.05
    f.set("U", U0)
    Ug = np.zeros_like(U0); Ug[mesh["perm"]] = U0
    g.set("U", Ug)
    for _ in range(4):
        f.step(); g.step()
    Uf = f.get("U").reshape(-1, 3)
    assert np.abs(Uf).max() > 0.1
    close(pm.to_lattice(mesh, g.get("U").reshape(-1, 3)), Uf, 1e-7, "U")
    pf, pg = f.get("p"), pm.to_lattice(mesh, g.get("p"))
    close(pg - pg.mean(), pf - pf.mean(), 1e-6, "p")
    f.close(); g.close()


@pytest.mark.parametrize("kind", ["ico_vanLeer", "ico_linear_upwind_mg", "pimple_cloud"])
def test_cyclic_patches_match_the_restatement(product, oracle, kind):
    """translational cyclic pairs (fy_poly_mesh.patch_neighbour) folded into internal faces, on a periodically distorted block: the folded geometry (weights,
    nonOrthDeltaCoeffs, correction vectors across the seam, the image offsets), then the flow -- a channel periodic in x and z between a fixed and a moving wall with a
    disturbance (limited / linearUpwind convection use the neighbour's IMAGE centre), and pimpleFoamYade with a cloud periodic in x and y under gravity"""
    n = 10
    L = (1.0, 1.0, 1.0) if kind != "pimple_cloud" else (0.1, 0.1, 0.1)
    vm = pm.wavy_periodic(0.025 * L[0], L)
    kw = dict(p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10, p_max_iter=5000)
    if kind != "pimple_cloud":
        mesh = pm.make_cyclic(pm.hex_block(n, n, n, L, vm, renumber_seed=10), [(0, 1), (4, 5)])
        u_val = [(0, 0, 0)] * 6
        u_val[3] = (1.0, 0, 0.4)
        if kind == "ico_vanLeer":
            kw.update(convection_scheme=4)
        else:
            kw.update(convection_scheme=2, p_solver=product.FY_PSOLVER_PCG_MG)
        okw = {k: v for k, v in kw.items() if k != "p_solver"}
        h = product.LduSolver(mesh, 0.4 / n, 0.01, [1, 1, 0, 0, 1, 1], u_val, [0] * 6, n_non_orth=2, **kw)
        o = oracle.LduSolver(mesh, 0.4 / n, 0.01, [1, 1, 0, 0, 1, 1], u_val, [0] * 6, n_non_orth=2, **okw)
        for nm in ("C", "V", "Cf", "Sf", "w", "dcNO", "kvec", "sep", "orig_face"):
            np.testing.assert_allclose(h.geometry(nm), o.geometry(nm), rtol=0, atol=1e-13, err_msg=nm)
        assert len(h.get("phi")) == len(mesh["owner"]) - 2 * n * n and len(h.get("mom_lower")) == len(mesh["neighbour"]) + 2 * n * n
        U0 = np.random.RandomState(3).rand(mesh["n_cells"], 3) * 0.2
        h.set("U", U0); o.set("U", U0)
        for _ in range(4):
            h.step(); o.step()
        assert np.abs(h.get("U")).max() > 0.3
        if kind == "ico_linear_upwind_mg":
            assert len(h.mg_levels()) >= 2 and h.stats()["p_iters_total"] < o.stats()["p_iters_total"]
    else:
        dx = L[0] / n
        mesh = pm.make_cyclic(pm.hex_block(n, n, n, L, vm, renumber_seed=8), [(0, 1), (2, 3)])
        rel = dict(u_relax=0.8, u_relax_final=1.0, p_relax=0.7, p_relax_final=1.0)
        h = product.LduSolver(mesh, 2e-4, 1e-5, [1, 1, 1, 1, 0, 0], [(0, 0, 0)] * 6, [0, 0, 0, 0, 2, 2], solver=1, g=(0, 0, -9.81), n_non_orth=1, n_outer_correctors=2, n_correctors=2, **rel, **kw)
        o = oracle.LduSolver(mesh, 2e-4, 1e-5, [1, 1, 1, 1, 0, 0], [(0, 0, 0)] * 6, [0, 0, 0, 0, 2, 2], solver=1, g=(0, 0, -9.81), n_non_orth=1, n_outer=2, n_correctors=2, **rel, **kw)
        h.hold_sources(True)
        rs = np.random.RandomState(23)
        for step in range(3):
            h.set_particles(bed_particles(rs, 1500, L[0], dx))
            h.step()
            alpha = h.get("alpha")
            assert alpha.min() < 0.95
            o.step(source=h.get("uSourceCoupling"), alpha=alpha, drag=h.get("uSourceDrag"))
            close(h.get("U"), o.get("U"), 2e-6, "U step %d" % step)
        assert np.abs(h.get("U")).max() > 1e-4
    ph, po = h.get("p"), o.get("p")
    close(ph - ph.mean(), po - po.mean(), 1e-5, "p")
    close(h.get("phi"), o.get("phi"), 1e-5, "phi")
    close(h.get("U"), o.get("U"), 2e-6, "U")
    h.close(); o.close()


def test_taylor_green_vortices_in_a_periodic_box_on_the_hip_solver(product):
    """tests/test_ldu_oracle.py::test_taylor_green_vortices_in_a_periodic_box on the HIP solver, one level finer (48 cells per period, distorted, no boundary face at
    all), with the multigrid preconditioner: the error keeps falling (0.022, 0.0041 on the restatement at 12 and 24)"""
    nu, T, n, dt = 0.1, 0.5, 48, 0.00125
    L = (2 * np.pi, 2 * np.pi, 0.75)
    mesh = pm.make_cyclic(pm.hex_block(n, n, 3, L, pm.wavy_periodic(0.03 * 12 / n, L)), [(0, 1), (2, 3), (4, 5)])
    s = product.LduSolver(mesh, dt, nu, [1] * 6, [(0, 0, 0)] * 6, [0] * 6, n_non_orth=2, p_tol=1e-11, p_rel_tol=0.0, p_final_tol=1e-11, u_tol=1e-11, p_max_iter=5000,
                          p_solver=product.FY_PSOLVER_PCG_MG)
    C = s.geometry("C")
    ex = lambda t: np.stack([np.sin(C[:, 0]) * np.cos(C[:, 1]), -np.cos(C[:, 0]) * np.sin(C[:, 1]), 0 * C[:, 0]], axis=1) * np.exp(-2 * nu * t)
    s.set("U", ex(0.0))
    for _ in range(int(round(T / dt))):
        s.step()
    err = np.abs(s.get("U").reshape(-1, 3) - ex(T)).max()
    assert err < 0.002, err
    assert s.stats()["cont_err_sum_local"] < 1e-10 and len(s.get("phi")) == len(s.get("mom_lower"))
    s.close()


@pytest.mark.parametrize("variant", ["plain", "upwind_relaxed_calculated", "kEpsilon"])
def test_les_kEqn_on_a_lattice_equals_the_structured_hip_solver(product, variant):
    """LESModel kEqn through both HIP solvers on the same block with the same cloud's fields (the general side is given the structured coupling's alpha / drag / source):
    k, nut and U after three steps"""
    n, box = 12, 0.1
    dx = box / n
    mesh = pm.hex_block(n, n, n, (box, box, box))
    kw = dict(p_tol=1e-11, p_rel_tol=0.0, p_final_tol=1e-11, u_tol=1e-11)
    les = dict(turbulence_model=2, nut_initial=3e-5, les_delta_coeff=0.8, k_initial=2e-4, k_tol=1e-13)
    u_val = [(0, 0, 0)] * 6
    u_val[3] = (0.3, 0, 0.1)
    fkw, gkw = {}, {}
    if variant != "plain":
        les.update(k_convection_scheme=1, k_relax=0.8)
        fkw = dict(k_bc=[0, 0, 0, 1, 0, 0], k_value=[0, 0, 0, 5e-4, 0, 0], nut_bc=[3, 0, 3, 3, 0, 1], nut_value=[3e-5, 0, 3e-5, 6e-5, 0, 2e-5])
        gkw = dict(k_bc=[0, 0, 0, 1, 0, 0], k_val=[0, 0, 0, 5e-4, 0, 0], nut_bc=[3, 0, 3, 3, 0, 1], nut_val=[3e-5, 0, 3e-5, 6e-5, 0, 2e-5])
    if variant == "kEpsilon":                            # RAS kEpsilon without wall functions: epsilon, then k, nut = Cmu k^2 / epsilon
        les.update(turbulence_model=3, eps_initial=1.2e-4, eps_tol=1e-13, ras_cmu=0.085, ras_c1=1.4, ras_c2=1.9, ras_c3=-0.33, ras_sigmak=1.1, ras_sigmaeps=1.25, eps_convection_scheme=1, eps_relax=0.7)
        fkw.update(eps_bc=[0, 0, 1, 1, 0, 0], eps_value=[0, 0, 2e-4, 3e-4, 0, 0]); gkw.update(eps_bc=[0, 0, 1, 1, 0, 0], eps_val=[0, 0, 2e-4, 3e-4, 0, 0])
    case = product.make_case(1, n, n, n, dx, 2e-4, 1e-5, g=(0, 0, -9.81), u_val=u_val, p_bc=[2] * 6, p_solver=0, n_outer_correctors=2, n_correctors=2, p_max_iter=5000, **les, **fkw, **kw)
    f = product.Solver(case)
    g = product.LduSolver(mesh, 2e-4, 1e-5, [0] * 6, u_val, [2] * 6, solver=1, g=(0, 0, -9.81), n_outer_correctors=2, n_correctors=2, p_max_iter=5000, **les, **gkw, **kw)
    f.hold_sources(True)
    rs = np.random.RandomState(17)
    for step in range(3):
        f.set_particles(bed_particles(rs, 3000, box, dx))
        f.step()
        g.set("alpha", f.get("alpha")); g.set("uSourceDrag", f.get("uSourceDrag")); g.set("uSource", f.get("uSource"))
        g.step()
        if variant == "kEpsilon":
            close(g.get("epsilon"), f.get("epsilon"), 1e-6, "epsilon step %d" % step)
        close(g.get("k"), f.get("k"), 1e-6, "k step %d" % step)
        close(g.get("nut"), f.get("nut"), 1e-6, "nut step %d" % step)
        close(g.get("U").reshape(-1, 3), f.get("U").reshape(-1, 3), 1e-6, "U step %d" % step)
    assert not np.allclose(f.get("k"), 2e-4, rtol=1e-3)
    f.close(); g.close()


def test_les_kEqn_on_a_wavy_mesh_matches_the_restatement(product, oracle):
    """the k equation on skewed cells (the corrected laplacian's explicit part with grad k, delta from each cell's volume), a fixed-value k patch, `calculated` nut
    patches, upwind convection of k and a relaxation factor, with a cloud: k, nut, U, p against the restatement"""
    n, box = 10, 0.1
    dx = box / n
    mesh = pm.hex_block(n, n, n, (box, box, box), pm.wavy(0.2 * dx, (box, box, box)), renumber_seed=8)
    kw = dict(p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10, p_max_iter=5000)
    les = dict(turbulence_model=2, nut_initial=2e-5, les_delta_coeff=1.0, k_initial=2e-4, k_tol=1e-12, k_convection_scheme=1, k_relax=0.9)
    pat = dict(k_bc=[0, 0, 0, 1, 0, 0], k_val=[0, 0, 0, 5e-4, 0, 0], nut_bc=[3, 0, 3, 3, 0, 1], nut_val=[2e-5, 0, 2e-5, 4e-5, 0, 1e-5])
    rel = dict(u_relax=0.8, u_relax_final=1.0, p_relax=0.7, p_relax_final=1.0)
    lidv = [(0, 0, 0)] * 6
    lidv[3] = (0.3, 0, 0.1)
    h = product.LduSolver(mesh, 2e-4, 1e-5, [0] * 6, lidv, [2] * 6, solver=1, g=(0, 0, -9.81), n_non_orth=1, n_outer_correctors=2, n_correctors=2, **les, **pat, **rel, **kw)
    o = oracle.LduSolver(mesh, 2e-4, 1e-5, [0] * 6, lidv, [2] * 6, solver=1, g=(0, 0, -9.81), n_non_orth=1, n_outer=2, n_correctors=2, **les, **pat, **rel, **kw)
    h.hold_sources(True)
    rs = np.random.RandomState(23)
    for step in range(3):
        h.set_particles(bed_particles(rs, 1500, box, dx))
        h.step()
        o.step(source=h.get("uSourceCoupling"), alpha=h.get("alpha"), drag=h.get("uSourceDrag"))
        close(h.get("k"), o.get("k"), 1e-6, "k step %d" % step)
        close(h.get("nut"), o.get("nut"), 1e-6, "nut step %d" % step)
        close(h.get("U"), o.get("U"), 2e-6, "U step %d" % step)
    ph, po = h.get("p"), o.get("p")
    close(ph - ph.mean(), po - po.mean(), 1e-5, "p")
    assert not np.allclose(h.get("k"), 2e-4, rtol=1e-3) and h.get("k").min() > 0
    h.close(); o.close()


def test_ras_kEpsilon_on_a_wavy_mesh_matches_the_restatement(product, oracle):
    """RAS kEpsilon without wall functions on skewed cells with a cloud: the epsilon equation, then k with the new epsilon, nut = Cmu k^2 / epsilon; fixed-value patches of
    both, `calculated` nut patches, upwind convection, relaxation -- epsilon, k, nut, U, p against the restatement"""
    n, box = 10, 0.1
    dx = box / n
    mesh = pm.hex_block(n, n, n, (box, box, box), pm.wavy(0.2 * dx, (box, box, box)), renumber_seed=8)
    kw = dict(p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10, p_max_iter=5000)
    ras = dict(turbulence_model=3, nut_initial=2e-5, k_initial=2e-4, eps_initial=1.2e-4, k_tol=1e-12, eps_tol=1e-12, ras_cmu=0.085, ras_c1=1.4, ras_c2=1.9, ras_c3=-0.33,
               ras_sigmak=1.1, ras_sigmaeps=1.25, k_convection_scheme=1, eps_convection_scheme=1, k_relax=0.9, eps_relax=0.8)
    pat = dict(k_bc=[0, 0, 0, 1, 0, 0], k_val=[0, 0, 0, 5e-4, 0, 0], eps_bc=[0, 0, 1, 1, 0, 0], eps_val=[0, 0, 2e-4, 3e-4, 0, 0], nut_bc=[3, 0, 3, 3, 0, 1], nut_val=[2e-5, 0, 2e-5, 4e-5, 0, 1e-5])
    rel = dict(u_relax=0.8, u_relax_final=1.0, p_relax=0.7, p_relax_final=1.0)
    lidv = [(0, 0, 0)] * 6
    lidv[3] = (0.3, 0, 0.1)
    h = product.LduSolver(mesh, 2e-4, 1e-5, [0] * 6, lidv, [2] * 6, solver=1, g=(0, 0, -9.81), n_non_orth=1, n_outer_correctors=2, n_correctors=2, **ras, **pat, **rel, **kw)
    o = oracle.LduSolver(mesh, 2e-4, 1e-5, [0] * 6, lidv, [2] * 6, solver=1, g=(0, 0, -9.81), n_non_orth=1, n_outer=2, n_correctors=2, **ras, **pat, **rel, **kw)
    h.hold_sources(True)
    rs = np.random.RandomState(23)
    for step in range(3):
        h.set_particles(bed_particles(rs, 1500, box, dx))
        h.step()
        o.step(source=h.get("uSourceCoupling"), alpha=h.get("alpha"), drag=h.get("uSourceDrag"))
        for nm in ("epsilon", "k", "nut"):
            close(h.get(nm), o.get(nm), 1e-6, "%s step %d" % (nm, step))
        close(h.get("U"), o.get("U"), 2e-6, "U step %d" % step)
    ph, po = h.get("p"), o.get("p")
    close(ph - ph.mean(), po - po.mean(), 1e-5, "p")
    assert not np.allclose(h.get("epsilon"), 1.2e-4, rtol=1e-3) and h.get("epsilon").min() > 0
    h.close(); o.close()


@pytest.mark.parametrize("solver", ["ico", "pimple_cloud"])
def test_two_to_one_refined_polyhedra_match_the_restatement(product, oracle, solver):
    """a distorted box with its upper layers refined 2 x 2: nine-faced polyhedra under the interface (slot tables nine wide), five-point side faces, strongly unequal
    weights across it -- geometry, the lid-driven cavity with the multigrid preconditioner (agglomeration across the interface), pimpleFoamYade with a cloud"""
    if solver == "ico":
        L = (1.0, 1.0, 0.9)
        mesh = pm.refined_block(6, 6, 8, 4, L, pm.wavy(0.02, L))
        u_val = [(0, 0, 0)] * 6
        u_val[5] = (1.0, 0.2, 0)
        kw = dict(n_non_orth=2, p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10, p_max_iter=5000)
        h = product.LduSolver(mesh, 0.02, 0.01, [0] * 6, u_val, [0] * 6, p_solver=product.FY_PSOLVER_PCG_MG, **kw)
        o = oracle.LduSolver(mesh, 0.02, 0.01, [0] * 6, u_val, [0] * 6, **kw)
        for nm in ("C", "V", "Cf", "Sf", "w", "dcNO", "kvec"):
            np.testing.assert_allclose(h.geometry(nm), o.geometry(nm), rtol=0, atol=1e-13, err_msg=nm)
        for _ in range(4):
            h.step(); o.step()
        assert len(h.mg_levels()) >= 2 and h.mg_levels()[0][1] == 9 and h.stats()["p_iters_total"] < o.stats()["p_iters_total"]
        assert np.abs(h.get("U")).max() > 0.05
    else:
        box = 0.1
        L = (box, box, box)
        mesh = pm.refined_block(5, 5, 10, 5, L, pm.wavy(0.01 * box, L))
        kw = dict(p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10, p_max_iter=5000)
        rel = dict(u_relax=0.8, u_relax_final=1.0, p_relax=0.7, p_relax_final=1.0)
        h = product.LduSolver(mesh, 2e-4, 1e-5, [0] * 6, [(0, 0, 0)] * 6, [2] * 6, solver=1, g=(0, 0, -9.81), n_non_orth=1, n_outer_correctors=2, n_correctors=2, **rel, **kw)
        o = oracle.LduSolver(mesh, 2e-4, 1e-5, [0] * 6, [(0, 0, 0)] * 6, [2] * 6, solver=1, g=(0, 0, -9.81), n_non_orth=1, n_outer=2, n_correctors=2, **rel, **kw)
        h.hold_sources(True)
        rs = np.random.RandomState(31)
        for step in range(3):
            rec = bed_particles(rs, 1500, box, box / 10)
            rec[:, 2] = 0.3 * box + 0.4 * box * rs.random_sample(1500)                 # the cloud across the interface
            h.set_particles(rec)
            h.step()
            alpha = h.get("alpha")
            assert alpha.min() < 0.97
            o.step(source=h.get("uSourceCoupling"), alpha=alpha, drag=h.get("uSourceDrag"))
            close(h.get("U"), o.get("U"), 2e-6, "U step %d" % step)
    ph, po = h.get("p"), o.get("p")
    close(ph - ph.mean(), po - po.mean(), 1e-5, "p")
    close(h.get("phi"), o.get("phi"), 1e-5, "phi")
    close(h.get("U"), o.get("U"), 2e-6, "U")
    h.close(); o.close()


def test_rayleigh_layer_on_a_distorted_mesh_on_the_hip_solver(product):
    """the transient known answer of tests/test_ldu_oracle.py::test_rayleigh_layer_on_a_distorted_mesh on the HIP solver with the multigrid preconditioner, one level finer
    (128 cells across, 131 072 cells): the error keeps falling (0.0025, 0.0011 on the restatement at 32 and 64)"""
    from math import erfc, sqrt
    nu, U0, t0, T = 0.01, 1.0, 0.5, 1.0
    L = (0.25, 1.0, 0.25)
    errs, cross = [], []
    for ny, dt in ((64, 0.00125), (128, 0.0003125)):
        k = ny // 16
        mesh = pm.hex_block_fast(4 * k, ny, 4 * k, L, pm.wavy(0.01, L))
        u_val = [(0, 0, 0)] * 6
        u_val[2] = (U0, 0, 0)
        s = product.LduSolver(mesh, dt, nu, [1, 1, 0, 1, 1, 1], u_val, [1, 1, 0, 0, 0, 0], n_non_orth=1, p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10,
                              p_solver=product.FY_PSOLVER_PCG_MG, p_max_iter=5000)
        C = s.geometry("C")
        prof = lambda t: np.array([U0 * erfc(y / (2 * sqrt(nu * t))) for y in C[:, 1]])
        Ui = np.zeros((len(C), 3)); Ui[:, 0] = prof(t0)
        s.set("U", Ui)
        for _ in range(int(round((T - t0) / dt))):
            s.step()
        U = s.get("U").reshape(-1, 3)
        errs.append(np.abs(U[:, 0] - prof(T)).max() / U0)
        cross.append((np.abs(U[:, 1]) + np.abs(U[:, 2])).max() / U0)
        s.close()
    assert abs(errs[0] - 1.128e-3) < 1e-4 and errs[1] < 0.7 * errs[0] and max(cross) < 1e-3, (errs, cross)


def test_malformed_meshes_and_cases_are_refused_by_name(product):
    """fy_ldu_solver_create checks what it is handed: addressing (owner < neighbour, patches covering the boundary faces once, faces of three points or more, cells that close),
    the reference cell, the solver / preconditioner / closure selectors -- an error with the reason, never a half-built solver"""
    base = pm.hex_block(4, 4, 4)
    ok = lambda: product.LduSolver(base, 1e-3, 0.01, [0] * 6, [(0, 0, 0)] * 6, [0] * 6)
    ok().close()

    def broken(**edit):
        m = dict(base)
        for k, v in edit.items():
            m[k] = v
        return m
    own = base["owner"].copy(); own[0], nei0 = base["neighbour"][0], base["owner"][0]
    nei = base["neighbour"].copy(); nei[0] = nei0
    cases = [
        (broken(owner=own, neighbour=nei), {}, "owner < neighbour"),
        (broken(patch_size=np.array([16, 16, 16, 16, 16, 15], np.int32)), {}, "belongs to no patch"),
        (broken(patch_start=base["patch_start"] - 1), {}, "patch"),
        (broken(points=base["points"] * np.array([1.0, 1.0, 0.0])), {}, "no area|no volume|flat"),
        (base, dict(p_ref_cell=64), "pRefCell"),
        (base, dict(p_solver=7), "p_solver"),
        (base, dict(solver=3), "solver"),
        (base, dict(turbulence_model=7, solver=1), "turbulence"),
        (base, dict(convection_scheme=9), "convection"),
    ]
    for mesh, kw, needle in cases:
        with pytest.raises(product.FoamYadeError, match=needle):
            product.LduSolver(mesh, 1e-3, 0.01, [0] * 6, [(0, 0, 0)] * 6, [0] * 6, **kw)
    with pytest.raises(product.FoamYadeError, match="patch type"):
        product.LduSolver(base, 1e-3, 0.01, [0] * 6, [(0, 0, 0)] * 6, [2] * 6)          # fixedFluxPressure belongs to pimpleFoamYade
    # cyclic pairs: partners that do not name each other, halves of different sizes, halves that are not translates (x-min against y-max), a box one cell thick
    cyc = pm.make_cyclic(base, [(0, 1)])
    one_sided = dict(cyc); one_sided["patch_neighbour"] = np.array([1, -1, -1, -1, -1, -1], np.int32)
    turned = dict(base); turned["patch_neighbour"] = np.array([3, -1, -1, 0, -1, -1], np.int32)
    thin = pm.make_cyclic(pm.hex_block(1, 4, 4), [(0, 1)])
    for mesh, needle in ((one_sided, "does not name it back"), (turned, "not translates"), (thin, "its own neighbour")):
        with pytest.raises(product.FoamYadeError, match=needle):
            product.LduSolver(mesh, 1e-3, 0.01, [1, 1, 0, 0, 0, 0], [(0, 0, 0)] * 6, [0] * 6)
    product.LduSolver(cyc, 1e-3, 0.01, [1, 1, 0, 0, 0, 0], [(0, 0, 0)] * 6, [0] * 6).close()
    ok().close()


def test_periodic_channel_with_a_symmetry_side_les_and_a_cloud(product, oracle):
    """the patch kinds together: a channel periodic in x (cyclic pair), a symmetry plane on one side, walls elsewhere, LES kEqn with a `calculated` nut wall patch, limited
    convection, a cloud -- on a periodically distorted mesh, HIP against the restatement"""
    n, box = 10, 0.1
    L = (box, box, box)
    dx = box / n
    w0 = pm.wavy_periodic(0.02 * box, L)
    vm = lambda P: (lambda Q: np.stack([Q[:, 0], P[:, 1] + (Q[:, 1] - P[:, 1]) * np.sin(np.pi * P[:, 1] / box) ** 2, P[:, 2] + (Q[:, 2] - P[:, 2]) * np.sin(np.pi * P[:, 2] / box) ** 2], axis=1))(w0(P))
    mesh = pm.make_cyclic(pm.hex_block(n, n, n, L, vm, renumber_seed=3), [(0, 1)])          # (the y and z sides stay planes: the symmetry side is one)
    kw = dict(p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10, p_max_iter=5000)
    les = dict(turbulence_model=2, nut_initial=2e-5, les_delta_coeff=1.0, k_initial=2e-4, k_tol=1e-12, k_convection_scheme=1, convection_scheme=4)
    u_bc = [1, 1, 2, 0, 0, 0]                                   # x: cyclic (codes unused); ymin: symmetry; ymax, zmin, zmax: walls (ymax moving)
    u_val = [(0, 0, 0)] * 6
    u_val[3] = (0.3, 0, 0.05)
    p_bc = [0, 0, 0, 2, 2, 2]
    pat = dict(nut_bc=[0, 0, 0, 3, 0, 0], nut_val=[0, 0, 0, 3e-5, 0, 0])
    rel = dict(u_relax=0.8, u_relax_final=1.0, p_relax=0.7, p_relax_final=1.0)
    h = product.LduSolver(mesh, 2e-4, 1e-5, u_bc, u_val, p_bc, solver=1, g=(0, 0, -9.81), n_non_orth=1, n_outer_correctors=2, n_correctors=2, **les, **pat, **rel, **kw)
    o = oracle.LduSolver(mesh, 2e-4, 1e-5, u_bc, u_val, p_bc, solver=1, g=(0, 0, -9.81), n_non_orth=1, n_outer=2, n_correctors=2, **les, **pat, **rel, **kw)
    h.hold_sources(True)
    rs = np.random.RandomState(41)
    for step in range(3):
        h.set_particles(bed_particles(rs, 1500, box, dx))
        h.step()
        o.step(source=h.get("uSourceCoupling"), alpha=h.get("alpha"), drag=h.get("uSourceDrag"))
        close(h.get("U"), o.get("U"), 2e-6, "U step %d" % step)
        close(h.get("k"), o.get("k"), 1e-6, "k step %d" % step)
    ph, po = h.get("p"), o.get("p")
    close(ph - ph.mean(), po - po.mean(), 1e-5, "p")
    close(h.get("phi"), o.get("phi"), 1e-5, "phi")
    close(h.get("nut"), o.get("nut"), 1e-6, "nut")
    h.close(); o.close()


def test_general_mesh_solver_at_the_bench_size(product):
    """the size tools/ldu_bench.py and bench.py's general_mesh record run at -- 128^3 wavy hexahedra, 2.1 M cells, pimpleFoamYade with a 1 M-particle cloud -- through
    properties that do not need the restatement: closed cells and the box's volume from the solver's own geometry, an agglomeration hierarchy of 2 x 2 x 2 boxes down to 64
    cells, every particle of the cloud found, the void fraction removing the cloud's volume (up to the chain quirks), continuity closed, the multigrid-preconditioned PCG
    converging in a handful of iterations, and the same step again giving the same bits (no atomics in the FV half; the particle scatters are order-dependent, so: no cloud)"""
    n, L = 128, 0.1
    mesh = pm.hex_block_fast(n, n, n, (L, L, L), pm.wavy(0.6 * L / n, (L, L, L)))
    mk = lambda: product.LduSolver(mesh, 1e-4, 1e-6, [0] * 6, [(0, 0, 0)] * 6, [2] * 6, solver=1, g=(0.0, 0.0, -9.81), n_non_orth=1, u_relax=1.0, p_solver=product.FY_PSOLVER_PCG_MG)
    s = mk()
    Sf, V = s.geometry("Sf"), s.geometry("V")
    own, nei = mesh["owner"], mesh["neighbour"]
    ni = len(nei)
    tot = np.zeros((mesh["n_cells"], 3))
    np.add.at(tot, own, Sf); np.subtract.at(tot, nei, Sf[:ni])
    assert np.abs(tot).max() < 1e-18 + 1e-12 * np.abs(Sf).max() and V.sum() == pytest.approx(L ** 3, rel=1e-12) and V.min() > 0
    assert s.mg_levels() == [(n ** 3 // 8 ** q, 6) for q in range(6)]
    s.hold_sources(True)
    rs = np.random.RandomState(5)
    rec = np.zeros((1_000_000, 10))
    rec[:, 0:3] = L * rs.rand(1_000_000, 3) * np.array([1.0, 1.0, 0.6]); rec[:, 9] = 0.2 * L / n
    s.set_particles(rec)
    for _ in range(2):
        s.step()
    st = s.stats()
    assert np.all(s.found() == 1) and st["cont_err_sum_local"] < 1e-9 and st["p_iters_total"] <= 12, st
    dep, pvol = ((1.0 - s.get("alpha")) * V).sum(), ((4.0 / 3.0) * np.pi * rec[:, 9] ** 3).sum()
    assert 0.97 * pvol < dep <= pvol * (1 + 1e-12)
    assert np.isfinite(s.get("U")).all() and np.abs(s.get("U")).max() > 0
    s.close()
    a, b = mk(), mk()
    lidU = np.zeros((n ** 3, 3)); lidU[:, 0] = 0.01 * np.sin(np.arange(n ** 3) * 1e-3)
    for q in (a, b):
        q.set("U", lidU)
        q.step(); q.step()
    np.testing.assert_array_equal(a.get("U"), b.get("U")); np.testing.assert_array_equal(a.get("p"), b.get("p"))
    a.close(); b.close()
