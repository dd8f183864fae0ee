"""Inlets on the device (fy_inlets_desc; DESIGN.md section 3 "Inlets"): fixed-value velocity sides (fy_solver) and patches (fy_ldu_solver) whose value varies over the
faces and in time, against tests/inlets_ref.py -- the time functions in numpy and the unchanged oracle on the mesh with the inlet patch split into one-face patches,
rebuilt before every step (held to a plain oracle run bit for bit in tests/test_inlets_ref.py).

  1. the per-face path is the uniform path: the same bits as a plain uniform value, while the side's own u_value holds something else
  2. a jet profile scaled by a table that changes every step, against the reference: the general-mesh solver at tests/test_ldu_parity.py's bounds (U 2e-6, p 1e-5,
     phi 5e-6 of the field's maximum), the block solver on the lattice at the same bounds, block against general-mesh solver at 1e-7 / 1e-6
     (and with kEqn, k too at 1e-7, once with each k scheme: the scheme is NAMED wherever the two solvers meet, their defaults differ)
  3. the value's timing: U_boundary after each step is the reference's value at start_time + sum dt to 1e-14, the flow-rate inlet's flux is -Q(t)
  4. refusals by name

Inflow on zmin (side / patch 4), fixed pressure on zmax, walls elsewhere.  Solver tolerances 1e-10, as tests/test_ldu_parity.py."""
import numpy as np
import pytest

import inlets_ref as ir
import poly_meshes as pm

pytestmark = pytest.mark.gpu

NX, NY, NZ, DX = 6, 5, 7, 0.1
DT, NU = 0.02, 0.01
ZMIN = 4
U_BC, P_BC = [0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 1]
V = (0.02, -0.01, 0.3)
TOL = dict(p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10, p_max_iter=5000)
HX, HY, HZ = DX * np.array([1.3, 1.1, 1.0, 0.9, 0.8, 0.9]), DX * np.array([0.8, 1.0, 1.2, 1.0, 1.1]), DX * np.array([0.7, 0.8, 0.9, 1.0, 1.1, 1.2, 1.3])
Z0 = 2 * (NY * NZ + NX * NZ)                 # where side z- starts in the block's "U_boundary"
U = 2.0 ** -53


def close(a, b, rtol, what):
    sc = np.abs(b).max() + 1e-300
    err = np.abs(np.asarray(a) - np.asarray(b)).max() / sc
    print(what, "relative difference", err, "bound", rtol)
    assert err <= rtol, (what, err)


def u_val(v=V):
    return [(0, 0, 0)] * 4 + [tuple(v), (0, 0, 0)]


def block_case(product, solver=0, graded=False, v=V, inlets=None, **kw):
    return product.make_case(solver, NX, NY, NZ, DX, DT, NU, u_bc=U_BC, u_val=u_val(v), p_bc=P_BC, p_solver=0, grading=(HX, HY, HZ) if graded else None, inlets=inlets, **TOL, **kw)


def lattice_mesh(graded=False):
    """the block as a polyhedral mesh in the lattice numbering (cells, and the zmin patch's faces, in the block's own order)"""
    vm = None
    if graded:
        cum = [np.concatenate([[0.0], np.cumsum(h)]) for h in (HX, HY, HZ)]
        vm = lambda P: np.stack([cum[a][np.rint(P[:, a]).astype(int)] for a in range(3)], axis=1)
    mesh = pm.hex_block(NX, NY, NZ, (NX, NY, NZ) if graded else (NX * DX, NY * DX, NZ * DX), vm)
    s, n = int(mesh["patch_start"][ZMIN]), int(mesh["patch_size"][ZMIN])
    assert np.array_equal(mesh["owner"][s:s + n], np.arange(n))
    return mesh


def general_mesh(kind):
    if kind == "wavy_renumbered":
        return pm.hex_block(4, 3, 5, (1.0, 0.8, 1.2), pm.wavy(0.03, (1.0, 0.8, 1.2)), renumber_seed=5)
    if kind == "prisms":
        return pm.prism_block(3, 3, 4, (1.0, 0.9, 1.1), vertex_map=pm.wavy(0.02, (1.0, 0.9, 1.1)))
    if kind == "tetrahedra":
        return pm.tet_block(3, 3, 3, (1.0, 0.9, 1.1), vertex_map=pm.wavy(0.02, (1.0, 0.9, 1.1)))
    return lattice_mesh(kind == "graded")


def patch_faces(mesh, patch=ZMIN):
    s, n = int(mesh["patch_start"][patch]), int(mesh["patch_size"][patch])
    return s, n


def jet_profile(mesh, seed=7):
    """[n_faces, 3]: a jet over the third of the inlet's faces with the smallest x, plus a seeded perturbation of every component"""
    s, n = patch_faces(mesh)
    off, fp, P = mesh["face_offsets"], mesh["face_points"], mesh["points"]
    x = np.array([P[fp[off[f]:off[f + 1]]].mean(axis=0)[0] for f in range(s, s + n)])
    S = np.zeros((n, 3))
    S[:, 2] = 0.1
    S[np.argsort(x, kind="stable")[:(n + 2) // 3], 2] = 0.6
    return S + np.random.RandomState(seed).uniform(-0.02, 0.02, (n, 3))


def step_table(dt=DT):
    """0.5, 0.75, 1.0, 1.25 at the four steps' times; 0.2 at the start time, so that the first step's value differs from the one the initial flux was formed with, in
    the normal component too: a kernel that read the boundary value before the step's update would carry the start time's into the step and miss the reference"""
    return dict(kind="table", points=[(0.0, 0.2), (dt, 0.5), (2 * dt, 0.75), (3 * dt, 1.0), (4 * dt, 1.25)])


def zmin_of(mesh, U_boundary):
    s, n = patch_faces(mesh)
    ni = len(mesh["neighbour"])
    return np.asarray(U_boundary).reshape(-1, 3)[s - ni:s - ni + n]


def block_phi_on_mesh(f, mesh):
    """the block solver's three face arrays as the lattice mesh's phi (owner -> neighbour / outward)"""
    px, py, pz = f.get("phi_x").reshape(NZ, NY, NX + 1), f.get("phi_y").reshape(NZ, NY + 1, NX), f.get("phi_z").reshape(NZ + 1, NY, NX)
    ni = len(mesh["neighbour"])
    own, nei = np.asarray(mesh["owner"]), np.asarray(mesh["neighbour"])
    ijk = lambda c: (c % NX, (c // NX) % NY, c // (NX * NY))
    out = np.zeros(len(own))
    for fc in range(ni):
        (i, j, k), d = ijk(own[fc]), int(nei[fc] - own[fc])
        out[fc] = px[k, j, i + 1] if d == 1 else py[k, j + 1, i] if d == NX else pz[k + 1, j, i]
    for side in range(6):
        s, n = patch_faces(mesh, side)
        for fc in range(s, s + n):
            i, j, k = ijk(own[fc])
            out[fc] = (-px[k, j, 0], px[k, j, NX], -py[k, 0, i], py[k, NY, i], -pz[0, j, i], pz[NZ, j, i])[side]
    return out


# ------------------------------------------------------------------------------------------------ 1. the per-face path is the uniform path
TURB = {"kEqn": dict(turbulence_model=2, nut_initial=2e-5, les_delta_coeff=1.0, k_initial=2e-4, k_tol=1e-12),
        # kEpsilon with wall functions ON THE INLET SIDE: k_assemble_turb's wall production reads the side's velocity (U_b - U_P)
        "kEpsilon_wall": dict(turbulence_model=3, nut_initial=2e-5, k_initial=2e-4, eps_initial=1.2e-4, k_tol=1e-12, eps_tol=1e-12, nut_bc=[0, 0, 0, 0, 2, 0],
                              nut_value=[0, 0, 0, 0, 2e-5, 0], eps_bc=[0, 0, 0, 0, 2, 0])}


@pytest.mark.parametrize("solver", [0, 1, "kEqn", "kEpsilon_wall"])
@pytest.mark.parametrize("graded", [False, True])
def test_block_per_face_path_is_the_uniform_path(product, solver, graded):
    """run A: a plain uniform value v; run B: one `constant 1` term whose per-face shape is v on every face, the side's u_value another finite vector.  Four steps, the
    same bits in U, p, phi and U_boundary: a read site that still looks at u_value fails this.  With kEqn and with kEpsilon and wall functions on the inlet side the
    turbulence sweeps' reads are among them (k, nut too)"""
    extra = dict(n_outer_correctors=2) if solver else {}
    turb = isinstance(solver, str)
    if turb:
        extra.update(TURB[solver])
        solver = 1
    a = product.Solver(block_case(product, solver, graded, **extra))
    b = product.Solver(block_case(product, solver, graded, v=(7.0, -3.0, 11.0), inlets=[dict(patch=ZMIN, terms=[dict(f=1.0, shape=np.tile(V, (NX * NY, 1)))])], **extra))
    U0 = np.random.RandomState(3).rand(NX * NY * NZ, 3) * 0.05
    a.set("U", U0); b.set("U", U0)
    for name in ("phi_z", "U_boundary"):
        assert np.array_equal(a.get(name), b.get(name)), name
    for _ in range(4):
        a.step(); b.step()
    for name in ("U", "p", "phi_x", "phi_y", "phi_z", "U_boundary") + (("k", "nut") if turb else ()):
        assert np.array_equal(a.get(name), b.get(name)), name
    assert np.abs(a.get("U")).max() > 0.1
    if turb:
        assert not np.allclose(a.get("k"), 2e-4, rtol=1e-3)
    a.close(); b.close()


@pytest.mark.parametrize("solver", [0, 1])
def test_general_mesh_per_face_path_is_the_uniform_path(product, solver):
    mesh = general_mesh("wavy_renumbered")
    n = patch_faces(mesh)[1]
    kw = dict(n_non_orth=1, solver=solver, **TOL)
    if solver:
        kw.update(n_outer_correctors=2)
    a = product.LduSolver(mesh, DT, NU, U_BC, u_val(), P_BC, **kw)
    b = product.LduSolver(mesh, DT, NU, U_BC, u_val((7.0, -3.0, 11.0)), P_BC, inlets=[dict(patch=ZMIN, terms=[dict(f=1.0, shape=np.tile(V, (n, 1)))])], **kw)
    U0 = np.random.RandomState(3).rand(mesh["n_cells"], 3) * 0.05
    a.set("U", U0); b.set("U", U0)
    assert np.array_equal(a.get("phi"), b.get("phi"))
    for _ in range(4):
        a.step(); b.step()
    for name in ("U", "p", "phi", "U_boundary"):
        assert np.array_equal(a.get(name), b.get(name)), name
    assert np.abs(a.get("U")).max() > 0.1
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 2. against the reference
VARIANTS = {
    "plain": (dict(), dict()),
    "upwind": (dict(convection_scheme=1), dict(convection_scheme=1)),
    "no_predictor": (dict(momentum_predictor=0), dict(momentum_predictor=0)),
    "pimple_two_outer": (dict(solver=1, n_outer_correctors=2), dict(solver=1, n_outer=2)),
    # (the k scheme is named on both sides: fy_case_defaults says upwind, fy_ldu_case_defaults and the oracle's LduSolver linear)
    "kEqn": (dict(solver=1, turbulence_model=2, nut_initial=2e-5, les_delta_coeff=1.0, k_initial=2e-4, k_tol=1e-12, k_convection_scheme=0),
             dict(solver=1, turbulence_model=2, nut_initial=2e-5, les_delta_coeff=1.0, k_initial=2e-4, k_tol=1e-12, k_convection_scheme=0)),
}


def reference_run(oracle, mesh, terms, variant, n_non_orth, steps=4):
    s, n = patch_faces(mesh)
    probe = oracle.LduSolver(mesh, DT, NU, U_BC, u_val(), P_BC)
    Sf = probe.geometry("Sf")[s:s + n]
    probe.close()
    U0 = np.random.RandomState(3).rand(mesh["n_cells"], 3) * 0.05
    run = ir.SplitPatchRun(oracle, mesh, ZMIN, DT, NU, U_BC, u_val((9.0, 9.0, 9.0)), P_BC, None, lambda t: ir.inlet_values(terms, t, Sf), U0=U0, n_non_orth=n_non_orth,
                           **TOL, **VARIANTS[variant][1])
    t = 0.0
    for _ in range(steps):
        t = t + DT
        run.step(t)
    return run, U0


_REF = {}


def reference(oracle, kind, variant):
    """the reference of (mesh kind, variant), computed once and shared"""
    key = (kind, variant)
    if key not in _REF:
        mesh = general_mesh(kind)
        terms = [dict(f=step_table(), shape=jet_profile(mesh))]
        run, U0 = reference_run(oracle, mesh, terms, variant, 0 if kind in ("lattice", "graded") else 1)
        _REF[key] = (mesh, terms, {f: run.get(f) for f in ("U", "p", "phi")}, U0)
    return _REF[key]


GENERAL_CASES = [("wavy_renumbered", v) for v in VARIANTS] + [(k, "plain") for k in ("lattice", "graded", "prisms", "tetrahedra")]


@pytest.mark.parametrize("kind,variant", GENERAL_CASES)
def test_general_mesh_jet_with_a_table_matches_the_reference(product, oracle, kind, variant):
    mesh, terms, ref, U0 = reference(oracle, kind, variant)
    h = product.LduSolver(mesh, DT, NU, U_BC, u_val((9.0, 9.0, 9.0)), P_BC, inlets=[dict(patch=ZMIN, terms=terms)], n_non_orth=0 if kind in ("lattice", "graded") else 1,
                          **TOL, **VARIANTS[variant][0])
    h.set("U", U0)
    for _ in range(4):
        h.step()
    close(h.get("U"), ref["U"], 2e-6, "U"); close(h.get("p"), ref["p"], 1e-5, "p"); close(h.get("phi"), ref["phi"], 5e-6, "phi")
    assert np.abs(ref["U"]).max() > 0.1
    h.close()


BLOCK_CASES = [("lattice", v) for v in VARIANTS] + [("graded", "plain")]


@pytest.mark.parametrize("kind,variant", BLOCK_CASES)
def test_block_jet_with_a_table_matches_the_reference(product, oracle, kind, variant):
    """the block solver against the same split-patch reference on the lattice, at the general-mesh solver's bounds"""
    mesh, terms, ref, U0 = reference(oracle, kind, variant)
    hk = dict(VARIANTS[variant][0])
    solver = hk.pop("solver", 0)
    f = product.Solver(block_case(product, solver, kind == "graded", v=(9.0, 9.0, 9.0), inlets=[dict(patch=ZMIN, terms=terms)], **hk))
    f.set("U", U0)
    for _ in range(4):
        f.step()
    close(f.get("U"), ref["U"], 2e-6, "U"); close(f.get("p"), ref["p"], 1e-5, "p"); close(block_phi_on_mesh(f, mesh), ref["phi"], 5e-6, "phi")
    f.close()


def test_block_equals_the_general_mesh_solver_on_the_lattice(product):
    """both HIP solvers with the same inlet, at test_lattice_block_equals_the_structured_hip_solver's bounds"""
    mesh = lattice_mesh()
    terms = [dict(f=step_table(), shape=jet_profile(mesh))]
    U0 = np.random.RandomState(3).rand(mesh["n_cells"], 3) * 0.05
    f = product.Solver(block_case(product, 0, False, inlets=[dict(patch=ZMIN, terms=terms)]))
    g = product.LduSolver(mesh, DT, NU, U_BC, u_val(), P_BC, inlets=[dict(patch=ZMIN, terms=terms)], **TOL)
    f.set("U", U0); g.set("U", U0)
    for _ in range(4):
        f.step(); g.step()
    close(g.get("U"), f.get("U"), 1e-7, "U"); close(g.get("p"), f.get("p"), 1e-6, "p")
    assert np.array_equal(zmin_of(mesh, g.get("U_boundary")), f.get("U_boundary").reshape(-1, 3)[Z0:Z0 + NX * NY])
    f.close(); g.close()


@pytest.mark.parametrize("scheme", [0, 1])
def test_block_kEqn_equals_the_general_mesh_solver_on_the_lattice(product, scheme):
    """both HIP solvers with LES kEqn, a plain uniform inlet and no inlet set, the k scheme named on both sides (0 linear, 1 upwind): k to 1e-7 of its maximum after
    the first step and after four, U and p at the bounds of the test above.  Left to each side's default the two run different schemes and k differs by 6e-4 here"""
    mesh = lattice_mesh()
    kw = dict(VARIANTS["kEqn"][0], k_convection_scheme=scheme)
    kw.pop("solver")
    U0 = np.random.RandomState(3).rand(mesh["n_cells"], 3) * 0.05
    f = product.Solver(block_case(product, 1, False, **kw))
    g = product.LduSolver(mesh, DT, NU, U_BC, u_val(), P_BC, solver=1, **TOL, **kw)
    f.set("U", U0); g.set("U", U0)
    for step in range(4):
        f.step(); g.step()
        if step in (0, 3):
            close(g.get("k"), f.get("k"), 1e-7, "k after step %d" % (step + 1))
    close(g.get("U"), f.get("U"), 1e-7, "U"); close(g.get("p"), f.get("p"), 1e-6, "p")
    assert not np.allclose(f.get("k"), 2e-4, rtol=1e-3) and np.abs(f.get("U")).max() > 0.1
    f.close(); g.close()


# ------------------------------------------------------------------------------------------------ 3. the value's timing
def timing_terms(kind, n):
    rs = np.random.RandomState(11)
    if kind == "sine_level":        # sine with scale and level: two terms, the level's function is `constant 1`
        return [dict(f=dict(kind="sine", amplitude=0.4, frequency=3.0, t0=0.1), shape=rs.uniform(0.1, 0.3, (n, 3))), dict(f=1.0, shape=(0.0, 0.01, 0.25))]
    if kind == "vector_table":      # a vector table: one scalar table per component with the shapes e_x, e_y, e_z
        tabs = [[(1.4, 0.0), (1.52, 0.05), (1.6, -0.02), (2.5, 0.03)], [(1.4, 0.01), (1.55, -0.03), (2.5, 0.02)], [(1.4, 0.2), (1.51, 0.3), (1.56, 0.15), (1.62, 0.35), (2.5, 0.1)]]
        return [dict(f=dict(kind="table", points=tabs[a]), shape=tuple(np.eye(3)[a])) for a in range(3)]
    return [dict(f=dict(kind="table", points=[(1.4, 0.002), (1.53, 0.006), (1.6, 0.003), (2.5, 0.005)]), shape="flow_rate")]


@pytest.mark.parametrize("which", ["block", "graded_block", "general"])
@pytest.mark.parametrize("kind", ["sine_level", "vector_table", "flow_rate"])
def test_value_is_the_reference_at_the_time_the_step_advances_to(product, which, kind):
    """pimpleFoamYade with adjustTimeStep (delta t differs from step to step) from start_time 1.5: after each of five steps U_boundary on the inlet equals the
    reference's value at start_time + sum dt to 1e-14 (a handful of double operations and one sin).  The flow-rate inlet: the surfaceFieldValue sum of phi over the
    patch is -Q(t) within tests/test_monitors.py's tolerance for a prescribed flux, 4 n u |Q| (n the patch's faces)"""
    start = 1.5
    ctl = dict(adjust_time_step=1, max_co=0.2, max_delta_t=0.05, n_outer_correctors=1)
    if which == "general":
        mesh = general_mesh("prisms")
        n = patch_faces(mesh)[1]
        terms = timing_terms(kind, n)
        s = product.LduSolver(mesh, DT, NU, U_BC, u_val(), P_BC, solver=1, n_non_orth=1, inlets=product.inlets_desc([dict(patch=ZMIN, terms=terms)], start_time=start), **ctl, **TOL)
        Sf = s.get("Sf")[patch_faces(mesh)[0]:][:n]
        inlet = lambda: zmin_of(mesh, s.get("U_boundary"))
        patch = ZMIN
    else:
        graded = which == "graded_block"
        n = NX * NY
        terms = timing_terms(kind, n)
        s = product.Solver(block_case(product, 1, graded, inlets=product.inlets_desc([dict(patch=ZMIN, terms=terms)], start_time=start), **ctl))
        A = np.outer(HY, HX).ravel() if graded else np.full(n, DX * DX)
        Sf = np.stack([np.zeros(n), np.zeros(n), -A], axis=1)
        inlet = lambda: s.get("U_boundary").reshape(-1, 3)[Z0:Z0 + n]
        patch = 1 << ZMIN
    s.set_monitors([dict(name="q", kind="surface", patch=patch, operation="sum", fields=["phi"])], start_time=start)
    want0 = ir.inlet_values(terms, start, Sf)
    assert np.abs(inlet() - want0).max() <= 1e-14 * np.abs(want0).max()            # the start time's value, as a create leaves it
    elapsed, dts, times = 0.0, [], []
    for _ in range(5):
        s.step()
        dt = s.stats()["delta_t"]
        t = (start + elapsed) + dt
        elapsed += dt
        dts.append(dt); times.append(t)
        want = ir.inlet_values(terms, t, Sf)
        err = np.abs(inlet() - want).max() / np.abs(want).max()
        print(which, kind, "t", t, "relative difference", err)
        assert err <= 1e-14, (t, err)
    assert len(set(dts)) == 5, dts                                                   # the steps differ
    if kind == "flow_rate":
        tt, rows = s.monitor_rows(0)
        np.testing.assert_allclose(tt, start + np.cumsum(dts), rtol=1e-14)
        for t, got in zip(times, rows[:, 0]):
            Q = ir.time_function(terms[0]["f"], t)
            print("flow rate", t, got, -Q, "relative difference", abs(got + Q) / Q, "bound", 4 * n * U)
            assert abs(got + Q) <= 4 * n * U * abs(Q), (t, got, Q)
    s.close()


@pytest.mark.parametrize("which", ["block", "general"])
def test_every_kernel_of_the_first_step_sees_the_new_value(product, which):
    """ordering: a table whose value at the start time is a wildly different vector and whose value from the first step's time on is v gives the bits of the plain
    uniform run.  phi is not touched by the update (it keeps the start time's boundary flux until the loop re-forms it), so the two start values share their normal
    component and differ, by four orders of magnitude, in the tangential ones: the inlet's faces are plane and normal to z, the fluxes equal to the bit"""
    wild = (V[0] + 3000.0, V[1] - 7000.0, V[2])
    step = lambda a: dict(kind="table", points=[(0.0, wild[a]), (DT, V[a]), (10.0, V[a])])
    terms = [dict(f=step(a), shape=tuple(np.eye(3)[a])) for a in range(3)]
    if which == "block":
        a = product.Solver(block_case(product, 0, False))
        b = product.Solver(block_case(product, 0, False, v=(5.0, 5.0, 5.0), inlets=[dict(patch=ZMIN, terms=terms)]))
        names = ("U", "p", "phi_x", "phi_y", "phi_z", "U_boundary")
        inlet = lambda s: s.get("U_boundary").reshape(-1, 3)[Z0:Z0 + NX * NY]
    else:
        mesh = general_mesh("wavy_renumbered")
        a = product.LduSolver(mesh, DT, NU, U_BC, u_val(), P_BC, n_non_orth=1, **TOL)
        b = product.LduSolver(mesh, DT, NU, U_BC, u_val((5.0, 5.0, 5.0)), P_BC, n_non_orth=1, inlets=[dict(patch=ZMIN, terms=terms)], **TOL)
        names = ("U", "p", "phi", "U_boundary")
        inlet = lambda s: zmin_of(mesh, s.get("U_boundary"))
    assert np.array_equal(inlet(b), np.tile(wild, (len(inlet(b)), 1)))
    for _ in range(3):
        a.step(); b.step()
    for name in names:
        assert np.array_equal(a.get(name), b.get(name)), name
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 4. refusals, the clock
def test_refusals_by_name(product):
    one = lambda patch, **t: [dict(patch=patch, terms=[dict(dict(f=1.0, shape=V), **t)])]
    f = product.Solver(block_case(product))
    for spec, word in ((one(5), "not a fixedValue"), (one(6), "does not exist"), ([dict(patch=ZMIN, terms=[])], "n_terms 0"), ([dict(patch=ZMIN, terms=[dict(f=1.0, shape=V)] * 4)], "n_terms 4"),
                       (one(ZMIN, f=dict(kind="table", points=[(0, 1), (0, 2)])), "do not increase"), (one(ZMIN, f=dict(kind="sine", frequency=0.0)), "frequency"),
                       (one(ZMIN, shape_kind=1, shape=None), "shape array is NULL"), (one(ZMIN) + one(ZMIN), "listed twice"),
                       (one(ZMIN, f=dict(kind="table", points=[(0, 1)], out_of_bounds=2)), "outOfBounds")):
        with pytest.raises(product.FoamYadeError, match=word):
            f.set_inlets(spec)
    f.set_inlets(one(ZMIN))
    f.set_inlets(None)                                                  # off again, and on: the setter may be called any number of times before the first step
    f.set_inlets(one(ZMIN))
    f.step()
    with pytest.raises(product.FoamYadeError, match="stepped already"):
        f.set_inlets(one(ZMIN))
    f.close()
    # an unbalanced closed box: no patch fixes the pressure, every velocity side is fixedValue, the inlet's shape carries a net flux
    closed = dict(u_bc=[0] * 6, p_bc=[0] * 6, p_solver=0)
    with pytest.raises(product.FoamYadeError, match="do not balance"):
        product.Solver(product.make_case(0, NX, NY, NZ, DX, DT, NU, inlets=one(ZMIN), **closed))
    lid = product.Solver(product.make_case(0, NX, NY, NZ, DX, DT, NU, inlets=one(ZMIN, shape=(1.0, 0.5, 0.0)), **closed))      # a tangential profile carries none
    lid.step()
    lid.close()
    # z-slabs: FY_ERR_UNSUPPORTED
    slabs = product.VirtualSlabs(product.make_case(0, 8, 8, 16, 0.1 / 8, 0.005, 0.01, u_bc=U_BC, u_val=u_val(), p_bc=P_BC), 2)
    for sl in slabs.solvers:
        with pytest.raises(product.FoamYadeError) as e:
            sl.set_inlets(one(ZMIN))
        assert "error 5" in str(e.value) and "slab" in str(e.value)
    slabs.close()
    # the general mesh: a patch that is not fixedValue, a cyclic patch, after the first step
    mesh = general_mesh("wavy_renumbered")
    g = product.LduSolver(mesh, DT, NU, U_BC, u_val(), P_BC, **TOL)
    with pytest.raises(product.FoamYadeError, match="not a fixedValue"):
        g.set_inlets(one(5))
    with pytest.raises(product.FoamYadeError, match="per-face or flow-rate shape on a side without faces|does not exist"):
        g.set_inlets(one(9))
    g.step()
    with pytest.raises(product.FoamYadeError, match="stepped already"):
        g.set_inlets(one(ZMIN))
    g.close()
    cyc = pm.make_cyclic(pm.hex_block(4, 3, 5, (1.0, 0.8, 1.2)), [(0, 1)])
    with pytest.raises(product.FoamYadeError, match="cyclic"):
        product.LduSolver(cyc, DT, NU, [0, 0, 0, 0, 0, 1], u_val(), P_BC, inlets=one(0), **TOL)
    with pytest.raises(product.FoamYadeError, match="do not balance"):
        product.LduSolver(mesh, DT, NU, [0] * 6, u_val(), [0] * 6, inlets=one(ZMIN), **TOL)


def test_one_launch_per_step_on_the_inlets_clock(product):
    mesh = general_mesh("prisms")
    n = patch_faces(mesh)[1]
    spec = [dict(patch=ZMIN, terms=[dict(f=step_table(), shape=np.tile(V, (n, 1)))])]
    g = product.LduSolver(mesh, DT, NU, U_BC, u_val(), P_BC, inlets=spec, **TOL)
    f = product.Solver(block_case(product, inlets=[dict(patch=ZMIN, terms=[dict(f=step_table(), shape=V)])]))
    for s in (g, f):
        s.enable_kernel_timing(True)
        for _ in range(3):
            s.step()
        ms, launches = s.kernel_timing("inlets")
        assert launches == 3 and ms > 0.0, (ms, launches)
        s.close()
    plain = product.LduSolver(mesh, DT, NU, U_BC, u_val(), P_BC, **TOL)
    with pytest.raises(product.FoamYadeError, match="unknown kernel clock 'inlets'"):
        plain.kernel_timing("inlets")
    plain.close()
