"""Wall loads (fy_solver_set_wall_loads, fy_ldu_solver_set_wall_loads): the forces / wallShearStress / yPlus objects on the device.  Every per-face value and every row
equals tests/wall_loads_ref.py (np.longdouble) fed the fields read back after the same step, within the bound derived there; the min / max columns equal the min / max of
the device's per-face field bit for bit.  Shapes: a uniform 6 x 5 x 4 and a graded 7 x 5 x 4 block (distinct extents, interior cells on every axis), 20 x 15 x 3 (a side of
300 faces: two 256-lane blocks, and sets that end mid-block); general meshes at the sizes test_monitors.py uses for them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import poly_meshes as pm
import wall_loads_ref as wr

pytestmark = pytest.mark.gpu
G = 9.81
KEPS_WF = dict(turbulence_model=3, nut_bc=[0, 2, 0, 2, 1, 0], nut_value=[0, 0, 0, 0, 1e-5, 0], nut_initial=2e-5, k_bc=[0, 0, 0, 0, 1, 0], k_value=[0, 0, 0, 0, 2e-3, 0],
               k_initial=4e-3, k_convection_scheme=1, k_tol=1e-9, eps_bc=[0, 2, 0, 2, 1, 0], eps_value=[0, 0, 0, 0, 0.05, 0], eps_initial=0.02, eps_convection_scheme=1, eps_tol=1e-9)


def sides_of(mask):
    return [q for q in range(6) if (mask >> q) & 1]


def cloud_in(lo, hi, count, radius, seed):
    rs = np.random.RandomState(seed)
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    base = np.zeros((count, 10))
    base[:, 0:3] = lo + (hi - lo) * rs.random_sample((count, 3))
    base[:, 3:6] = 0.05 * rs.standard_normal((count, 3))
    base[:, 9] = radius
    return base


def check_sample(s, m, forces, wss, yplus, nu, wall_fn_patches=(), cmu25=0.0, block=True):
    """the LAST row of every object and the per-face fields against the restatement of the fields as they stand now.  forces: the dicts given to the solver (patches as
    lists of patch / side indices under "set"); wss / yplus: lists of patch indices"""
    nb = m["patch"].size
    turb = len(wall_fn_patches) > 0 or s.get("nut_boundary").size == nb
    nutb = s.get("nut_boundary") if turb else np.zeros(nb)
    wall_fn = np.isin(m["patch"], list(wall_fn_patches))
    fl = wr.face_loads(m, s.get("U"), s.get("U_boundary"), s.get("p_boundary"), nutb, nu, k=s.get("k") if len(wall_fn_patches) else None, wall_fn=wall_fn, cmu25=cmu25)
    names = m["names"]
    for q, f in enumerate(forces):
        idx = np.flatnonzero(np.isin(m["patch"], f["set"]))
        want, bnd = wr.forces_row(fl, idx, f["rho"], f.get("p_ref", 0.0), f.get("cofr", (0, 0, 0)))
        got = s.wall_load_rows(q)[1][-1]
        print("forces", f["name"], "got", got, "want", want, "err", np.abs(got - want), "bound", bnd)
        assert s.wall_loads_layout(q) == wr.labels_forces()
        assert np.all(np.abs(got - want) <= bnd), (f["name"], got, want, np.abs(got - want), bnd)
    q = len(forces)
    if wss is not None:
        dev = s.get("wallShearStress_boundary").reshape(-1, 3)
        member = np.isin(m["patch"], wss)
        err, bnd = np.abs(dev - fl["wss"].astype(np.float64)), wr.wss_bound(fl)
        print("wss max err / bound", (err[member] / np.maximum(bnd[member], 1e-300)).max(), "max |wss|", np.abs(dev).max())
        assert np.all(err[member] <= bnd[member]), (err[member].max(), bnd[member].min())
        assert not dev[~member].any()                                                      # exactly 0 outside the set
        row = s.wall_load_rows(q)[1][-1]
        lab = s.wall_loads_layout(q)
        for p, pa in enumerate(wss):
            on = dev[m["patch"] == pa]
            assert np.array_equal(row[6 * p:6 * p + 3], on.min(axis=0)) and np.array_equal(row[6 * p + 3:6 * p + 6], on.max(axis=0)), (pa, row, on.min(axis=0), on.max(axis=0))
            assert lab[6 * p] == f"min({names[pa]})_x" and lab[6 * p + 5] == f"max({names[pa]})_z", lab
        q += 1
    if yplus is not None:
        dev = s.get("yPlus_boundary")
        member = np.isin(m["patch"], yplus)
        err, bnd = np.abs(dev - fl["yplus"].astype(np.float64)), wr.yplus_bound(fl)
        print("yPlus max err / bound", (err[member] / np.maximum(bnd[member], 1e-300)).max(), "range", dev[member].min(), dev[member].max())
        assert np.all(err[member] <= bnd[member]), (err[member].max(), bnd[member])
        assert not dev[~member].any()
        row = s.wall_load_rows(q)[1][-1]
        assert s.wall_loads_layout(q)[:3] == [f"{op}({names[yplus[0]]})" for op in ("min", "max", "average")]
        for p, pa in enumerate(yplus):
            idx = np.flatnonzero(m["patch"] == pa)
            avg, ab = wr.yplus_average(fl, idx)
            assert row[3 * p] == dev[idx].min() and row[3 * p + 1] == dev[idx].max(), (pa, row, dev[idx].min(), dev[idx].max())
            assert abs(row[3 * p + 2] - avg) <= ab, (pa, row[3 * p + 2], avg, ab)
    return fl


def block_case(product, solver, nx, ny, nz, dx=0.01, grading=None, **kw):
    """a fixedValue lid at y+ and inflow at z-, a noSlip wall at x+, a symmetryPlane at x-, zeroGradient at y- and z+ (where the pressure is fixed)"""
    pim = solver == 1
    return product.make_case(solver, nx, ny, nz, dx, 2e-4, 1e-5, g=(0, 0, -G) if pim else (0, 0, 0), u_bc=[2, 0, 1, 0, 0, 1], origin=(0.01, -0.02, 0.03),
                             u_val=[(0, 0, 0)] * 3 + [(0.05, 0, 0.02), (0.01, 0.0, 0.1), (0, 0, 0)], p_bc=[2 if pim else 0] * 5 + [1], p_val=[0, 0, 0, 0, 0, 2.5], grading=grading, **kw)


def block_forces(ext):
    return [dict(name="wall", patches=1 << 1, set=[1], rho=1000.0),
            dict(name="all", patches=63, set=list(range(6)), rho=998.2, p_ref=1.5, cofr=(0.3 * ext[0], -0.2 * ext[1], 1.7 * ext[2]))]


# ------------------------------------------------------------------------------------------------ 1. the block against the restatement
@pytest.mark.parametrize("solver,graded,turb", [(0, False, False), (1, False, False), (1, True, False), (0, True, False), (1, False, True), (1, True, True)])
def test_block_against_restatement(product, solver, graded, turb):
    if graded:
        nx, ny, nz = 7, 5, 4
        grading = (0.01 * 1.15 ** np.arange(nx), 0.012 * 0.9 ** np.arange(ny), 0.008 * 1.1 ** np.arange(nz))
        ext = [a.sum() for a in grading]
        m = wr.block_mesh(nx, ny, nz, grading=grading, origin=(0.01, -0.02, 0.03))
    else:
        nx, ny, nz, grading = 6, 5, 4, None
        ext = [0.06, 0.05, 0.04]
        m = wr.block_mesh(nx, ny, nz, dx=0.01, origin=(0.01, -0.02, 0.03))
    kw = dict(KEPS_WF) if turb else {}
    s = product.Solver(block_case(product, solver, nx, ny, nz, grading=grading, **kw))
    forces = block_forces(ext)
    s.set_wall_loads(forces, wall_shear_stress=63, y_plus=0b001010)
    cloud = cloud_in(0.2 * np.array(ext) + (0.01, -0.02, 0.03), 0.7 * np.array(ext) + (0.01, -0.02, 0.03), 30, 0.0015, 4)
    for step in range(3):
        if solver == 1:
            rec = cloud.copy(); rec[:, 2] -= 1e-4 * step
            s.set_particles(rec)
        s.step()
        fl = check_sample(s, m, forces, list(range(6)), [1, 3], 1e-5, wall_fn_patches=[1, 3] if turb else [], cmu25=0.09 ** 0.25)
    assert s.wall_load_rows(0)[1].shape == (3, 12) and np.abs(s.wall_load_rows(1)[1][:, 3:6]).max() > 0      # a viscous force was there
    assert np.abs(fl["wss"]).max() > 0 and np.array_equal(s.get("nearWallDist"), m["y"].astype(np.float64))
    assert (s.get("nut_boundary").max() > 0) == turb
    s.close()


# ------------------------------------------------------------------------------------------------ 2. general meshes against the restatement
MESHES = {"hex": lambda: pm.hex_block(5, 4, 3, (0.05, 0.04, 0.03), pm.shear(0.2, 0.1, 0.1)), "prism": lambda: pm.prism_block(4, 3, 4, (0.04, 0.03, 0.04)),
          "tet": lambda: pm.tet_block(3, 3, 3, (0.03, 0.03, 0.03)), "refined": lambda: pm.refined_block(4, 4, 4, 2, (0.04, 0.04, 0.04))}


def ldu_case(product, solver, mesh, **kw):
    pim = solver == 1
    ctl = dict(solver=solver, n_non_orth=1, p_max_iter=5000)
    if pim:
        ctl.update(g=(0, 0, -G), n_outer_correctors=1, n_correctors=2)
    ctl.update(kw)
    return product.LduSolver(mesh, 2e-4, 1e-5, [2, 0, 1, 0, 0, 1], [(0, 0, 0)] * 3 + [(0.05, 0, 0.02), (0.01, 0.0, 0.1), (0, 0, 0)], [2 if pim else 0] * 5 + [1], [0, 0, 0, 0, 0, 2.5], **ctl)


@pytest.mark.parametrize("solver,kind", [(0, "hex"), (1, "hex"), (1, "prism"), (0, "tet"), (1, "refined")])
def test_general_mesh_against_restatement(product, solver, kind):
    mesh = MESHES[kind]()
    s = ldu_case(product, solver, mesh)
    hi = np.asarray(mesh["points"]).max(axis=0)
    forces = [dict(name="walls", patches=[1, 3], set=[1, 3], rho=1000.0), dict(name="all", patches=list(range(6)), set=list(range(6)), rho=998.2, p_ref=1.5, cofr=tuple(0.4 * hi))]
    s.set_wall_loads(forces, wall_shear_stress=[0, 1, 3, 4], y_plus=[3, 1])
    m = wr.general_mesh(s, mesh["owner"], mesh["neighbour"], mesh["patch_size"])
    assert np.array_equal(np.flatnonzero(m["y"] > 0), np.flatnonzero(np.isin(m["patch"], [1, 3])))          # nearWallDist: now on the selected patches
    cloud = cloud_in(0.2 * hi, 0.7 * hi, 30, 0.001, 6)
    for step in range(3):
        if solver == 1:
            s.set_particles(cloud)
        s.step()
        check_sample(s, m, forces, [0, 1, 3, 4], [3, 1], 1e-5, block=False)
    s.close()


def test_general_mesh_keqn_wall_functions_and_cyclic(product):
    mesh = MESHES["hex"]()
    wall = [0, 3]
    u_val = [(0, 0, 0)] * 6
    u_val[5] = (0.3, 0, 0.1)
    turb = dict(turbulence_model=2, nut_initial=3e-5, les_delta_coeff=0.8, k_initial=5e-3, k_tol=1e-13, k_convection_scheme=1, k_relax=0.8, wf_kappa=0.4, wf_E=9.0)
    s = product.LduSolver(mesh, 2e-4, 1e-5, [0] * 6, u_val, [0, 0, 0, 0, 0, 1], solver=1, n_outer_correctors=1, n_correctors=2, p_max_iter=5000, n_non_orth=1,
                          nut_bc=[2 if q in wall else 0 for q in range(6)], nut_val=[1e-5 if q in wall else 0.0 for q in range(6)], **turb)
    forces = [dict(name="wf", patches=wall, set=wall, rho=1.2)]
    s.set_wall_loads(forces, wall_shear_stress=[0, 3, 5], y_plus=[0, 3, 1])
    m = wr.general_mesh(s, mesh["owner"], mesh["neighbour"], mesh["patch_size"])
    for _ in range(2):
        s.step()
        check_sample(s, m, forces, [0, 3, 5], [0, 3, 1], 1e-5, wall_fn_patches=wall, cmu25=0.09 ** 0.25, block=False)
    s.close()
    # a folded cyclic pair: its walls are accepted, the cyclic patches are refused by name
    mesh = pm.make_cyclic(pm.hex_block(4, 3, 5, (0.04, 0.03, 0.05)), [(0, 1)])
    s = product.LduSolver(mesh, 2e-4, 1e-5, [1, 1, 0, 0, 0, 0], [(0, 0, 0)] * 5 + [(0.1, 0, 0)], [0] * 6, n_non_orth=0)
    for patch, word in ((0, "cyclic"), (1, "cyclic"), (6, "does not exist")):
        with pytest.raises(product.FoamYadeError) as e:
            s.set_wall_loads([dict(name="wrap", patches=[2, patch], rho=1.0)])
        assert "error 1" in str(e.value) and "wrap" in str(e.value) and word in str(e.value), str(e.value)
    forces = [dict(name="lid", patches=[5, 4], set=[5, 4], rho=2.0, cofr=(0.01, 0.02, 0.03))]
    s.set_wall_loads(forces, wall_shear_stress=[2, 3, 4, 5], y_plus=[2, 5])
    own, nei, patch = wr.folded_addressing(mesh)                                             # the owners' gradients gather across the folded faces
    m = wr.general_mesh(s, own, nei, mesh["patch_size"], patch=patch)
    assert m["nI"] == len(mesh["neighbour"]) + 15 and patch.size == s.get("p_boundary").size
    for _ in range(2):
        s.step()
        check_sample(s, m, forces, [2, 3, 4, 5], [2, 5], 1e-5, block=False)
    assert s.wall_load_rows(0)[1][-1][3] != 0.0                                              # the lid drags the fluid along x
    s.close()


# ------------------------------------------------------------------------------------------------ 3. the fold across blocks and padding
def test_fold_across_blocks(product):
    """20 x 15 x 3: the z sides have 300 faces (two 256-lane blocks), the boundary 2 (45 + 60 + 300) = 810 faces in 4 blocks padded to 8; the sets {z-} = faces
    [210, 510) and {x+, y-, z+} start and end mid-block"""
    nx, ny, nz = 20, 15, 3
    s = product.Solver(block_case(product, 0, nx, ny, nz))
    m = wr.block_mesh(nx, ny, nz, dx=0.01, origin=(0.01, -0.02, 0.03))
    assert m["patch"].size == 810 and np.flatnonzero(m["patch"] == 4)[[0, -1]].tolist() == [210, 509]
    forces = [dict(name="zlo", patches=1 << 4, set=[4], rho=1000.0), dict(name="three", patches=0b100110, set=[1, 2, 5], rho=1.0, cofr=(0.1, 0.1, 0.1))]
    s.set_wall_loads(forces, wall_shear_stress=1 << 4, y_plus=0b100010)
    for _ in range(2):
        s.step()
        check_sample(s, m, forces, [4], [1, 5], 1e-5)
    s.close()


# ------------------------------------------------------------------------------------------------ 4. known answers
def couette_profile(C_y, y0, H, U0):
    U = np.zeros((C_y.size, 3))
    U[:, 0] = U0 * (C_y - y0) / H
    return U


@pytest.mark.parametrize("general", [False, True])
def test_couette(product, general):
    """U = U0 (y - y0) / H e_x between a fixed wall at y- and a wall moving with U0 e_x at y+, written as the initial field; one icoFoam step keeps it (it is the steady
    solution, exact for a linear profile on this lattice).  wallShearStress = -+ nu U0 / H along x (y-: -, y+: +), the viscous force on each wall rho nu U0 / H times its
    area (on the fixed wall along +x) with no normal component, yPlus = y sqrt(nu U0 / H) / nu: rtol 1e-12, values exact up to rounding"""
    nx, ny, nz, dx, nu, U0, rho = 4, 6, 3, 0.01, 1e-3, 0.2, 1000.0
    H, area = ny * dx, nx * nz * dx * dx
    u_bc, u_val, p_bc = [1, 1, 0, 0, 1, 1], [(0, 0, 0)] * 3 + [(U0, 0, 0)] + [(0, 0, 0)] * 2, [1, 1, 0, 0, 0, 0]
    if general:
        mesh = pm.hex_block(nx, ny, nz, (nx * dx, ny * dx, nz * dx))
        s = product.LduSolver(mesh, 1e-4, nu, u_bc, u_val, p_bc, n_non_orth=0)
        s.set("U", couette_profile(s.get("C")[:, 1], 0.0, H, U0))
        walls = [2, 3]
        patch = np.concatenate([np.full(z, q) for q, z in enumerate(mesh["patch_size"])])
    else:
        s = product.Solver(product.make_case(0, nx, ny, nz, dx, 1e-4, nu, u_bc=u_bc, u_val=u_val, p_bc=p_bc))
        yc = (np.arange(nx * ny * nz) // nx % ny + 0.5) * dx
        s.set("U", couette_profile(yc, 0.0, H, U0))
        walls, patch = 0b1100, wr.block_mesh(nx, ny, nz, dx=dx)["patch"]
    s.set_wall_loads([dict(name="lo", patches=[2] if general else 1 << 2, rho=rho), dict(name="hi", patches=[3] if general else 1 << 3, rho=rho)], wall_shear_stress=walls, y_plus=walls)
    s.step()
    tau = nu * U0 / H
    wss, yp = s.get("wallShearStress_boundary").reshape(-1, 3), s.get("yPlus_boundary")
    for pa, sign in ((2, -1.0), (3, 1.0)):
        on = wss[patch == pa]
        np.testing.assert_allclose(on[:, 0], sign * tau, rtol=1e-12)
        np.testing.assert_allclose(on[:, 1:], 0.0, atol=1e-12 * tau)
        np.testing.assert_allclose(yp[patch == pa], 0.5 * dx * np.sqrt(tau) / nu, rtol=1e-12)
    assert not wss[(patch != 2) & (patch != 3)].any()
    for q, sign in ((0, 1.0), (1, -1.0)):
        row = s.wall_load_rows(q)[1][0]
        np.testing.assert_allclose(row[3], sign * rho * tau * area, rtol=1e-12)
        np.testing.assert_allclose(row[4:6], 0.0, atol=1e-12 * rho * tau * area)
    s.close()


def test_hydrostatic_column(product):
    """the bed box at rest under g, no particles, all six sides in one forces object: the pressure force is the fluid's weight rho g V (along g: Sf points out of the
    fluid, so this is what the fluid does to the box -- the box pushes back upwards with the same), and the pressure moment about an offset CofR is (r_centroid - CofR) x F;
    the tolerance of test_monitors.py::test_hydrostatic_column for the same solve (1e-5 relative)"""
    nx, ny, nz, dx, rho = 12, 12, 24, 0.005, 1000.0
    s = product.Solver(product.make_case(1, nx, ny, nz, dx, 1e-3, 1e-6, g=(0, 0, -G), p_bc=[2] * 6, p_tol=1e-10, p_final_tol=1e-10, p_rel_tol=0.0))
    cofr = np.array([0.1, -0.05, 0.02])
    s.set_wall_loads([dict(name="box", patches=63, rho=rho, cofr=tuple(cofr))])
    for _ in range(3):
        s.step()
    row = s.wall_load_rows(0)[1][-1]
    V = nx * ny * nz * dx ** 3
    F = np.array([0.0, 0.0, -rho * G * V])
    W = rho * G * V
    assert np.all(np.abs(row[0:3] - F) <= 1e-5 * W), (row[0:3], F)
    r = np.array([nx, ny, nz]) * dx / 2 - cofr
    M = np.cross(r, F)
    assert np.all(np.abs(row[6:9] - M) <= 1e-5 * W * np.linalg.norm(r)), (row[6:9], M)
    assert np.all(np.abs(row[3:6]) <= 1e-5 * W)                                         # at rest: no viscous force
    s.close()


# ------------------------------------------------------------------------------------------------ 5. determinism and non-interference
def test_determinism_and_non_interference(product):
    """as test_monitors.py's: two particles whose stencils share no cell, so that coupled runs can be compared bit for bit"""
    nx, ny, nz, dx = 6, 6, 16, 0.01
    rec = np.zeros((2, 10))
    rec[:, 0:3] = [(0.031, 0.029, 0.032), (0.028, 0.033, 0.124)]
    rec[:, 3:6] = [(0.01, 0.0, -0.05), (0.0, 0.02, -0.03)]
    rec[:, 9] = 0.002
    out = []
    for on in (True, True, False):
        s = product.Solver(product.make_case(1, nx, ny, nz, dx, 2e-4, 1e-5, g=(0, 0, -G), p_bc=[2] * 6))
        s.enable_kernel_timing(True)
        if on:
            s.set_wall_loads([dict(name="f", patches=63, rho=1000.0, cofr=(0.1, 0.2, 0.3))], wall_shear_stress=0b001111, y_plus=63)
        forces, iters = [], []
        for step in range(3):
            s.set_particles(rec); s.step(); forces.append(s.forces())
            st = s.stats(); iters.append((st["p_iters_total"], st["u_iters_total"]))
        res = {nm: s.get(nm) for nm in ("U", "p", "phi_x", "phi_y", "phi_z")}
        res["forces"], res["iters"] = np.array(forces), np.array(iters)
        if on:
            res["rows"] = [np.column_stack(s.wall_load_rows(q)) for q in range(3)]
            res["faces"] = [s.get("wallShearStress_boundary"), s.get("yPlus_boundary")]
            ms, launches = s.kernel_timing("wall_loads")
            assert launches > 0 and ms > 0, (ms, launches)
        else:
            with pytest.raises(product.FoamYadeError):
                s.kernel_timing("wall_loads")                                            # off: no such entry
            with pytest.raises(product.FoamYadeError):
                s.get("yPlus_boundary")
        out.append(res)
        s.close()
    for nm in ("U", "p", "phi_x", "phi_y", "phi_z", "forces", "iters"):
        assert np.array_equal(out[0][nm], out[2][nm]), nm
    for a, b in zip(out[0]["rows"] + out[0]["faces"], out[1]["rows"] + out[1]["faces"]):
        assert np.array_equal(a, b), (a, b)
    assert out[0]["rows"][0].shape == (3, 13) and np.abs(out[0]["faces"][0]).max() > 0


# ------------------------------------------------------------------------------------------------ 6. ring wrap, interval, reconfigure
def test_ring_wrap_interval_reconfigure(product):
    objs = dict(forces=[dict(name="a", patches=63, rho=1.0, interval=2)], wall_shear_stress=dict(patches=0b1010, interval=1))
    rows = []
    for ring in (4, 0):
        s = product.Solver(block_case(product, 0, 6, 5, 4))
        s.set_wall_loads(ring_rows=ring, **objs)
        for _ in range(11):
            s.step()
        rows.append([s.wall_load_rows(q) for q in range(2)])
        if ring:
            t, v = rows[0][0]
            assert v.shape == (5, 12) and rows[0][1][1].shape == (11, 12)
            np.testing.assert_allclose(t, 2e-4 * np.array([2, 4, 6, 8, 10]), rtol=1e-14)
            t3, v3 = s.wall_load_rows(1, first_row=7)
            assert np.array_equal(t3, rows[0][1][0][7:]) and np.array_equal(v3, rows[0][1][1][7:])
            s.set_wall_loads(ring_rows=ring, **objs)                                     # a second call restarts the history
            assert s.wall_load_rows(0)[1].shape == (0, 12)
            s.step(); s.step()
            assert s.wall_load_rows(0)[1].shape == (1, 12)
            s.set_wall_loads(None)                                                       # NULL frees it
            with pytest.raises(product.FoamYadeError):
                s.wall_load_rows(0)
            with pytest.raises(product.FoamYadeError):
                s.get("wallShearStress_boundary")
            s.step()
        s.close()
    for (ta, va), (tb, vb) in zip(*rows):
        assert np.array_equal(ta, tb) and np.array_equal(va, vb)                         # the wrapped ring lost nothing


# ------------------------------------------------------------------------------------------------ 7. refusals, symbols, sizes
BAD = [
    (dict(forces=[dict(name="o1", patches=0, rho=1.0)]), "o1", "empty"),
    (dict(forces=[dict(name="o2", patches=64, rho=1.0)]), "o2", "sides 64"),
    (dict(forces=[dict(name="o3", patches=1, rho=0.0)]), "o3", "rho"),
    (dict(forces=[dict(name="o4", patches=1, rho=-2.0)]), "o4", "rho"),
    (dict(forces=[dict(name="o5", patches=1, rho=1.0, interval=-1)]), "o5", "interval"),
    (dict(forces=[dict(name=f"f{q}", patches=1, rho=1.0) for q in range(5)]), "fy_solver_set_wall_loads", "5 forces objects"),
    (dict(wall_shear_stress=0), "wallShearStress", "empty"),
    (dict(y_plus=dict(patches=128)), "yPlus", "sides 128"),
    (dict(forces=[dict(name="fine", patches=1, rho=1.0)], ring_rows=-1), "fy_solver_set_wall_loads", "ring_rows"),
]


@pytest.mark.parametrize("kw,name,word", BAD, ids=[b[1] + "-" + b[2].split()[0] for b in BAD])
def test_refusals(product, kw, name, word):
    s = product.Solver(product.make_case(1, 6, 6, 6, 0.01, 2e-4, 1e-5, p_bc=[2] * 6))
    with pytest.raises(product.FoamYadeError) as e:
        s.set_wall_loads(**kw)
    assert "error 1" in str(e.value) and word in str(e.value) and name in str(e.value), str(e.value)      # FY_ERR_INVALID, naming the object and the word
    with pytest.raises(product.FoamYadeError):
        s.wall_load_rows(0)                                                                               # a refused call leaves wall loads off
    s.close()


def test_refusals_of_slabs_patch_lists_and_the_case_descriptor(product):
    case = product.make_case(0, 8, 8, 16, 0.1 / 8, 0.005, 0.01, p_bc=[0] * 6)
    slabs = product.VirtualSlabs(case, 2)
    for sl in slabs.solvers:
        with pytest.raises(product.FoamYadeError) as e:
            sl.set_wall_loads([dict(name="f", patches=63, rho=1.0)])
        assert "error 5" in str(e.value) and "slab" in str(e.value)                                         # FY_ERR_UNSUPPORTED
    slabs.close()
    case.wall_loads = product.wall_loads_desc([dict(name="late", patches=0, rho=1.0)])                      # the descriptor of a case applies at create
    with pytest.raises(product.FoamYadeError) as e:
        product.Solver(case)
    assert "late" in str(e.value) and "empty" in str(e.value)
    case.wall_loads = product.wall_loads_desc([dict(name="early", patches=1 << 3, rho=1.0)])
    s = product.Solver(case)
    s.step()
    assert s.wall_load_rows(0)[1].shape == (1, 12)
    s.close()
    mesh = pm.hex_block(4, 3, 5, (0.04, 0.03, 0.05))
    s = product.LduSolver(mesh, 2e-4, 1e-5, [0] * 6, [(0, 0, 0)] * 5 + [(0.1, 0, 0)], [0] * 6, n_non_orth=0)
    for patches, word in (([], "empty"), (list(range(6)) + [0, 1, 2], "9 patches"), ([1, 1], "twice"), ([-1], "does not exist")):
        with pytest.raises(product.FoamYadeError) as e:
            s.set_wall_loads(y_plus=dict(patches=patches))
        assert "error 1" in str(e.value) and "yPlus" in str(e.value) and word in str(e.value), str(e.value)
    s.close()


def test_yplus_without_viscosity_and_writes_to_the_read_outs_are_refused(product):
    """yPlus divides by nu: a laminar case with nu = 0 (which both solvers accept) is refused by name, on both solvers; forces and wallShearStress are not.  The per-face
    fields and the block's new read-outs cannot be written"""
    s = product.Solver(product.make_case(1, 6, 6, 6, 0.01, 2e-4, 0.0, p_bc=[2] * 6))
    with pytest.raises(product.FoamYadeError) as e:
        s.set_wall_loads([dict(name="f", patches=1, rho=1.0)], y_plus=1)
    assert "error 1" in str(e.value) and "yPlus" in str(e.value) and "nu > 0" in str(e.value), str(e.value)
    with pytest.raises(product.FoamYadeError):
        s.wall_load_rows(0)
    s.set_wall_loads([dict(name="f", patches=1, rho=1.0)], wall_shear_stress=1)
    s.close()
    mesh = pm.hex_block(4, 3, 5, (0.04, 0.03, 0.05))
    s = product.LduSolver(mesh, 2e-4, 0.0, [0] * 6, [(0, 0, 0)] * 5 + [(0.1, 0, 0)], [0] * 6, n_non_orth=0)
    with pytest.raises(product.FoamYadeError) as e:
        s.set_wall_loads(y_plus=[5])
    assert "error 1" in str(e.value) and "yPlus" in str(e.value) and "nu > 0" in str(e.value), str(e.value)
    s.close()
    s = product.Solver(product.make_case(1, 6, 6, 6, 0.01, 2e-4, 1e-5, p_bc=[2] * 6))
    s.set_wall_loads(wall_shear_stress=63, y_plus=63)
    for name in ("wallShearStress_boundary", "yPlus_boundary", "nut_boundary", "nearWallDist"):
        with pytest.raises(product.FoamYadeError) as e:
            s.set(name, np.zeros(s.get(name).size))
        assert "read-only" in str(e.value), (name, str(e.value))
    s.close()
    s = product.LduSolver(mesh, 2e-4, 1e-5, [0] * 6, [(0, 0, 0)] * 5 + [(0.1, 0, 0)], [0] * 6, n_non_orth=0)
    before = s.get("nearWallDist").copy()
    s.set_wall_loads(y_plus=[5, 2])
    assert np.count_nonzero(s.get("nearWallDist")) == 4 * 3 + 4 * 5 and not before.any()
    for name in ("wallShearStress_boundary", "yPlus_boundary", "nearWallDist"):
        if name != "wallShearStress_boundary":
            with pytest.raises(product.FoamYadeError):
                s.set(name, np.zeros(s.get(name).size))
    s.enable_kernel_timing(True)
    with pytest.raises(product.FoamYadeError) as e:
        s.kernel_timing("nothing")
    assert "wall_loads" in str(e.value)
    s.set_wall_loads(None)                                            # nearWallDist follows from the current configuration, not from its history
    assert np.array_equal(s.get("nearWallDist"), before)
    s.close()


def test_symbols_sizes_and_abi_version(product):
    L = product.lib()
    for pre in ("fy_solver", "fy_ldu_solver"):
        for fn in ("set_wall_loads", "wall_loads_layout", "get_wall_load_rows"):
            assert hasattr(L, f"{pre}_{fn}")
    assert C.sizeof(product.WallPatchSet) == 8 + 4 * 8 and C.sizeof(product.ForcesObject) == 32 + 40 + 5 * 8 + 8 and C.sizeof(product.WallFieldObject) == 48
    assert C.sizeof(product.WallLoadsDesc) == 8 + 4 * 120 + 2 * 48 + 8 + 8 == 600          # (wall_loads.hpp asserts the same number of the C struct)
    assert product.WALL_LOADS_MAX_FORCES == 4 and product.WALL_LOADS_MAX_PATCHES == 8
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "foamyade_hip.h")).read()
    assert L.fy_abi_version() == int(re.search(r"#define FY_ABI_VERSION (\d+)", hdr).group(1)) >= 25
    for struct in ("fy_case_desc", "fy_ldu_case"):                                        # appended at the END of both descriptors
        body = hdr.split("} %s;" % struct)[0].rstrip()
        assert re.search(r"fy_wall_loads_desc wall_loads;\s*(/\*.*\*/)?$", body), struct
