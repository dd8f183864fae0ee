"""Run-time monitors (fy_solver_set_monitors, fy_ldu_solver_set_monitors): every row a solver keeps equals tests/monitors_ref.py fed the fields read back after the
same step (hold_sources(True): what stood where the sample was taken), within the summation bound derived there -- 4 n 2^-53 S|term| / |den|, min and max bit for
bit.  The boundary values the surface objects reduce are the read-outs "p_boundary" / "U_boundary" / "T_boundary", which test_boundary_readouts holds to the patch
conditions.  Shapes: blocks 5 x 6 x 7 (under one block), 5 x 6 x 1 (sides of 5 and 6 faces), 12 x 12 x 24 (13.5 blocks of 256 cells, 3.375 of the cell sweep's 1024-cell
tiles: a partial last block and padding partials either way; `walls` = four sides), a graded 6 x 5 x 7; general meshes: sheared hexahedra 4 x 3 x 5, prisms, tetrahedra, a 2:1 refined box, a cyclic pair."""
import ctypes as C
import math

import numpy as np
import pytest

import monitors_ref as mr
import poly_meshes as pm

pytestmark = pytest.mark.gpu
COMPS = {"U": 3, "uParticle": 3, "uSource": 3}
G = 9.81


# ------------------------------------------------------------------------------------------------ views of a solver: fields, measures, patch members
class BlockView:
    def __init__(self, s, nx, ny, nz, dx=None, grading=None):
        self.s, self.n = s, (nx, ny, nz)
        h = [np.full(nx, dx), np.full(ny, dx), np.full(nz, dx)] if grading is None else [np.asarray(a, float) for a in grading]
        self.V = ((h[0][None, None, :] * h[1][None, :, None]) * h[2][:, None, None]).ravel() if grading is not None else np.full(nx * ny * nz, dx * dx * dx)
        ax = (h[1][None, :] * h[2][:, None]).ravel(); ay = (h[0][None, :] * h[2][:, None]).ravel(); az = (h[0][None, :] * h[1][:, None]).ravel()
        self.A = np.concatenate([ax, ax, ay, ay, az, az])
        sizes = [ny * nz, ny * nz, nx * nz, nx * nz, nx * ny, nx * ny]
        self.off = np.concatenate([[0], np.cumsum(sizes)])
        self.nb = int(self.off[-1])
        c = np.arange(nx * ny * nz).reshape(nz, ny, nx)
        self.owner = np.concatenate([c[:, :, 0].ravel(), c[:, :, -1].ravel(), c[:, 0, :].ravel(), c[:, -1, :].ravel(), c[0].ravel(), c[-1].ravel()])
        nrm = np.zeros((6, 3))
        for q in range(6):
            nrm[q, q // 2] = 1.0 if q % 2 else -1.0
        self.normal = np.concatenate([np.tile(nrm[q], (sizes[q], 1)) for q in range(6)])
        self.side = np.concatenate([np.full(sizes[q], q) for q in range(6)])

    def members(self, mask):
        return np.flatnonzero((mask >> self.side) & 1)

    def cell(self, name):
        a = self.s.get(name)
        return a.reshape(-1, 3) if COMPS.get(name) == 3 else a

    def phi_out(self):
        nx, ny, nz = self.n
        fx, fy, fz = self.s.get("phi_x").reshape(nz, ny, nx + 1), self.s.get("phi_y").reshape(nz, ny + 1, nx), self.s.get("phi_z").reshape(nz + 1, ny, nx)
        return np.concatenate([-fx[:, :, 0].ravel(), fx[:, :, -1].ravel(), -fy[:, 0, :].ravel(), fy[:, -1, :].ravel(), -fz[0].ravel(), fz[-1].ravel()])

    def face(self, name):
        if name == "phi":
            return self.phi_out()
        a = self.s.get(name + "_boundary")
        return a.reshape(-1, 3) if name == "U" else a


class LduView:
    def __init__(self, s, mesh):
        self.s, self.mesh = s, mesh
        self.V = s.get("V")
        nf = s.get("magSf").size
        self.nb = s.get("p_boundary").size
        self.ni = nf - self.nb
        self.A = s.get("magSf")[self.ni:]
        Sf = s.get("Sf")[self.ni:]
        self.normal = Sf / self.A[:, None]
        if "patch_neighbour" not in mesh:
            self.owner = np.asarray(mesh["owner"])[self.ni:]
            self.side = np.concatenate([np.full(z, q) for q, z in enumerate(mesh["patch_size"])])

    def members(self, patch):
        return np.flatnonzero(self.side == patch)

    def cell(self, name):
        a = self.s.get("uSourceCoupling" if name == "uSource" else name)
        return a.reshape(-1, 3) if COMPS.get(name) == 3 else a

    def face(self, name):
        if name == "phi":
            return self.s.get("phi")[self.ni:]
        a = self.s.get(name + "_boundary")
        return a.reshape(-1, 3) if name == "U" else a


def expected_row(view, obj):
    """the restatement's values and bounds for one object from the fields as they stand now"""
    vals, bnds = [], []
    vol = obj["kind"] == "vol"
    idx = None if vol else view.members(obj["patch"])
    m = view.V if vol else view.A[idx]
    w = None
    if obj.get("weight_field"):
        w = view.cell("alpha") if vol else view.face("phi")[idx]
    for f in obj["fields"]:
        x = view.cell(f) if vol else view.face(f)[idx]
        v, b = mr.reduce(obj["operation"], x, m, w)
        vals += list(v); bnds += list(b)
    return np.array(vals), np.array(bnds)


def assert_row(got, want, bound, op, what):
    print(what, "got", got, "want", want, "bound", bound)
    if op in ("min", "max"):
        assert np.array_equal(got, want), (what, got, want)
    else:
        assert np.all(np.abs(got - want) <= bound), (what, got, want, np.abs(got - want), bound)


def run_against_restatement(s, view, objects, steps, cloud=None, ring_rows=0):
    """set the objects, step, and hold every sampled row to the restatement; returns the rows per object"""
    s.set_monitors(objects, ring_rows=ring_rows)
    s.hold_sources(True)
    want = [[] for _ in objects]
    t, times = getattr(view, "t", 0.0), [[] for _ in objects]              # a row's time counts from the solver's creation, not from set_monitors
    for step in range(1, steps + 1):
        if cloud is not None:
            s.set_particles(cloud(step))
        s.step()
        t += s.stats()["delta_t"]
        for q, o in enumerate(objects):
            if step % o.get("interval", 1) == 0:
                want[q].append(expected_row(view, o)); times[q].append(t)
    view.t = t
    rows = []
    for q, o in enumerate(objects):
        tt, v = s.monitor_rows(q)
        assert len(tt) == len(want[q]) and v.shape == (len(want[q]), len(s.monitor_layout(q))), (o["name"], tt, len(want[q]))
        np.testing.assert_allclose(tt, times[q], rtol=1e-14)
        for r, (val, bnd) in enumerate(want[q]):
            assert_row(v[r], val, bnd, o["operation"], f"{o['name']} row {r}")
        rows.append(v)
    return rows


def cloud_in(lo, hi, count, radius, seed):
    rs = np.random.RandomState(seed)
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    base = np.zeros((count, 10))
    base[:, 0:3] = lo + (hi - lo) * rs.random_sample((count, 3))
    base[:, 3:6] = 0.05 * rs.standard_normal((count, 3))
    base[:, 9] = radius

    def at(step):
        rec = base.copy()
        rec[:, 2] -= 1e-4 * step
        return rec
    return at


def object_sets(pimple, thermal, inlet, walls):
    """two sets of at most 8 objects that together carry every operation, scalar and vector fields, shared fields, and one object with interval 2"""
    sc = ["p"] + (["alpha"] if pimple else []) + (["T"] if thermal else [])
    vol_ops = [op for op in mr.VOLUME_OPS if pimple or op != "weightedVolAverage"]
    a = []
    for q, op in enumerate(vol_ops):
        o = dict(name=f"v_{op}", kind="vol", operation=op, fields=(["U"] + sc) if q % 2 == 0 else (sc + ["U"] + (["uParticle"] if pimple else ["uSource"])))
        if op == "weightedVolAverage":
            o["weight_field"] = "alpha"
        if op == "max":
            o["interval"] = 2
        a.append(o)
    a.append(dict(name="s_flow", kind="surface", patch=inlet, operation="sum", fields=["phi"]))
    b = []
    for q, op in enumerate(mr.SURFACE_OPS):
        o = dict(name=f"s_{op}", kind="surface", patch=walls if q % 2 else inlet, operation=op, fields=["phi", "p", "U"] + (["T"] if thermal else []))
        if op == "weightedAverage":
            o["weight_field"] = "phi"
        if op == "min":
            o["interval"] = 2
        b.append(o)
    b.append(dict(name="v_mean", kind="vol", operation="volAverage", fields=["p", "U"]))
    return a, b


def block_solver(product, solver, nx, ny, nz, dx=0.01, thermal=True, grading=None, **kw):
    """a channel along z: fixedValue inflow at z-, fixed pressure and zeroGradient U at z+, a slip side at x-, a wall at x+, zeroGradient U at y-, a wall at y+"""
    pim = solver == 1
    th = product.thermal_desc(4000.0, 0.6, T_initial=300.0, T_bc=(0, 0, 0, 1, 1, 0), T_value=(0, 0, 0, 320.0, 350.0, 0), particle_temperature=400.0) if thermal else None
    extra = dict(thermal=th) if thermal else {}
    extra.update(kw)
    c = product.make_case(solver, nx, ny, nz, dx, 2e-4, 1e-5, g=(0, 0, -G) if pim else (0, 0, 0), u_bc=[2, 0, 1, 0, 0, 1],
                          u_val=[(0, 0, 0)] * 4 + [(0.01, 0.0, 0.1), (0, 0, 0)], p_bc=[2 if pim else 0] * 5 + [1], p_val=[0, 0, 0, 0, 0, 2.5], grading=grading, **extra)
    return product.Solver(c)


def ldu_solver(product, solver, mesh, thermal=True, **kw):
    """the same channel on a general mesh whose patches are the six sides (poly_meshes.SIDES)"""
    pim = solver == 1
    th = dict(thermal=product.thermal_desc(4000.0, 0.6, T_initial=300.0, particle_temperature=400.0), T_bc=[0, 0, 0, 1, 1, 0], T_val=[0, 0, 0, 320.0, 350.0, 0]) if thermal else {}
    ctl = dict(solver=solver, n_non_orth=1, p_max_iter=5000)
    if pim:
        ctl.update(g=(0, 0, -G), n_outer_correctors=1, n_correctors=2)
    ctl.update(kw)
    return product.LduSolver(mesh, 2e-4, 1e-5, [2, 0, 1, 0, 0, 1], [(0, 0, 0)] * 4 + [(0.01, 0.0, 0.1), (0, 0, 0)], [2 if pim else 0] * 5 + [1], [0, 0, 0, 0, 0, 2.5], **th, **ctl)


# ------------------------------------------------------------------------------------------------ 1. every operation against the restatement
@pytest.mark.parametrize("solver", [0, 1])
def test_block_every_operation(product, solver):
    nx, ny, nz, dx = 5, 6, 7, 0.01
    s = block_solver(product, solver, nx, ny, nz, dx)
    view = BlockView(s, nx, ny, nz, dx)
    cloud = cloud_in((0.005, 0.005, 0.01), (0.045, 0.055, 0.06), 60, 0.15 * dx, 4)
    for objs in object_sets(solver == 1, True, inlet=1 << 4, walls=0b001111):
        rows = run_against_restatement(s, view, objs, 3, cloud)
        assert rows[0].shape[0] == 3 and any(len(r) == 1 for r in rows)             # the interval-2 object sampled once in three steps
    if solver == 1:
        assert view.cell("alpha").min() < 1.0                                       # particles were there
    assert s.monitor_layout(7) == ["volAverage(p)", "volAverage(U)_x", "volAverage(U)_y", "volAverage(U)_z"] and s.monitor_layout(0)[0] == "sum(phi)"
    s.close()


def test_graded_and_flat_blocks(product):
    """a graded 6 x 5 x 7 block (cell volumes and face areas differ), and 5 x 6 x 1: sides of 5 and 6 faces"""
    hx, hy, hz = 0.01 * 1.15 ** np.arange(6), 0.012 * 0.9 ** np.arange(5), 0.008 * 1.1 ** np.arange(7)
    s = block_solver(product, 1, 6, 5, 7, thermal=False, grading=(hx, hy, hz))
    view = BlockView(s, 6, 5, 7, grading=(hx, hy, hz))
    assert abs(view.V.sum() - hx.sum() * hy.sum() * hz.sum()) < 1e-12 * view.V.sum()
    for objs in object_sets(True, False, inlet=1 << 4, walls=0b001111):
        run_against_restatement(s, view, objs, 2, cloud_in((0.005, 0.005, 0.01), (0.05, 0.04, 0.06), 40, 0.002, 9))
    s.close()
    s = block_solver(product, 0, 5, 6, 1, thermal=False)
    view = BlockView(s, 5, 6, 1, 0.01)
    objs = [dict(name="x", kind="surface", patch=0b000011, operation="areaAverage", fields=["p", "U"]),
            dict(name="y", kind="surface", patch=0b001000, operation="sum", fields=["phi"]),
            dict(name="all", kind="surface", patch=63, operation="sum", fields=["phi"])]
    assert len(view.members(3)) == 12 and len(view.members(8)) == 5
    run_against_restatement(s, view, objs, 2)
    s.close()


MESHES = {"hex": lambda: pm.hex_block(4, 3, 5, (0.04, 0.03, 0.05), pm.shear(0.2, 0.1, 0.1)), "prism": lambda: pm.prism_block(4, 3, 4, (0.04, 0.03, 0.04)),
          "tet": lambda: pm.tet_block(3, 3, 3, (0.03, 0.03, 0.03)), "refined": lambda: pm.refined_block(4, 4, 4, 2, (0.04, 0.04, 0.04))}


@pytest.mark.parametrize("solver,kind", [(0, "hex"), (1, "hex"), (1, "prism"), (0, "tet"), (1, "refined")])
def test_general_mesh_every_operation(product, solver, kind):
    mesh = MESHES[kind]()
    s = ldu_solver(product, solver, mesh)
    view = LduView(s, mesh)
    hi = np.asarray(mesh["points"]).max(axis=0)
    cloud = cloud_in(0.2 * hi, 0.7 * hi, 30, 0.001, 6)
    for objs in object_sets(solver == 1, True, inlet=4, walls=1):
        run_against_restatement(s, view, objs, 3, cloud)
    s.close()


# ------------------------------------------------------------------------------------------------ 2. neutral padding
def test_neutral_padding(product):
    """max of an all-negative field and min of an all-positive one, where the reduction has a partial last block and padding partials (3456 cells: 3.375 tiles of the
    cell sweep, padded to 8 partials; 864 wall faces: 3.375 blocks) and on a general mesh of 162 cells: a padding partial of 0 would win both.  The written field is T (a closed box at rest only diffuses it: it
    keeps its sign through the step, which U and p, being solved for, would not); the all-positive one is alpha = 1"""
    nx, ny, nz = 12, 12, 24
    rs = np.random.RandomState(1)
    th = product.thermal_desc(4000.0, 0.6, T_initial=-1.0)
    s = product.Solver(product.make_case(1, nx, ny, nz, 0.005, 2e-4, 1e-5, p_bc=[2] * 6, thermal=th))
    objs = [dict(name="hi", kind="vol", operation="max", fields=["T"]), dict(name="lo", kind="vol", operation="min", fields=["alpha", "T"]),
            dict(name="bhi", kind="surface", patch=0b001111, operation="max", fields=["T"]), dict(name="blo", kind="surface", patch=0b110000, operation="min", fields=["T"])]
    s.set_monitors(objs)
    s.set("T", -1.0 - rs.random_sample(nx * ny * nz))
    s.hold_sources(True)
    s.step()
    view = BlockView(s, nx, ny, nz, 0.005)
    assert view.cell("T").max() < 0 and view.cell("alpha").min() > 0
    for q, o in enumerate(objs):
        want, _ = expected_row(view, o)
        _, v = s.monitor_rows(q)
        assert np.array_equal(v[0], want), (o["name"], v[0], want)
    assert s.monitor_rows(0)[1][0, 0] < 0 and s.monitor_rows(1)[1][0, 0] == 1.0 and s.monitor_rows(2)[1][0, 0] < 0
    s.set_monitors([dict(name="lo", kind="vol", operation="min", fields=["T"]), dict(name="blo", kind="surface", patch=63, operation="min", fields=["T"])])
    s.set("T", 1.0 + rs.random_sample(nx * ny * nz))
    s.step()
    assert s.monitor_rows(0)[1][0, 0] == view.cell("T").min() > 0 and s.monitor_rows(1)[1][0, 0] == view.face("T").min() > 0
    s.close()
    mesh = pm.tet_block(3, 3, 3, (0.03, 0.03, 0.03))
    n = mesh["n_cells"]
    assert n % 256 != 0
    s = product.LduSolver(mesh, 2e-4, 1e-5, [0] * 6, [(0, 0, 0)] * 6, [0] * 6, n_non_orth=1, thermal=product.thermal_desc(4000.0, 0.6, T_initial=-1.0))
    view = LduView(s, mesh)
    for sign, op in ((-1.0, "max"), (1.0, "min")):
        s.set_monitors([dict(name="c", kind="vol", operation=op, fields=["T"]), dict(name="f", kind="surface", patch=2, operation=op, fields=["T"])])
        s.set("T", sign * (1.0 + rs.random_sample(n)))
        s.step()
        T, Tb = view.cell("T"), view.face("T")[view.members(2)]
        assert np.all(sign * T > 0)
        assert s.monitor_rows(0)[1][0, 0] == (T.max() if op == "max" else T.min()) and s.monitor_rows(1)[1][0, 0] == (Tb.max() if op == "max" else Tb.min())
    s.close()


# ------------------------------------------------------------------------------------------------ 3. the boundary read-outs
def check_readouts(view, u_bc, u_val, p_bc, p_val, T_bc, T_val):
    pb, Ub, Tb = view.face("p"), view.face("U"), view.face("T")
    p, Uc, T = view.cell("p"), view.cell("U"), view.cell("T")
    for q in range(6):
        idx = view.members(1 << q if isinstance(view, BlockView) else q)
        own = view.owner[idx]
        if u_bc[q] == 0:
            assert np.array_equal(Ub[idx], np.tile(u_val[q], (len(idx), 1)))
        elif u_bc[q] == 1:
            assert np.array_equal(Ub[idx], Uc[own])
        else:
            un = np.einsum("ij,ij->i", Ub[idx], view.normal[idx])
            # n = Sf / |Sf| carries ~3 roundings per component, u_n five, the subtraction one per component, this check's own dot three: 32 u |U| covers them
            assert np.all(np.abs(un) <= 32 * 2.0 ** -53 * np.abs(Uc[own]).sum(axis=1) + 1e-300), un
            tang = Uc[own] - np.einsum("ij,ij->i", Uc[own], view.normal[idx])[:, None] * view.normal[idx]
            assert np.allclose(Ub[idx], tang, rtol=1e-12, atol=1e-300)
        if p_bc[q] == 1:
            assert np.array_equal(pb[idx], np.full(len(idx), p_val[q]))
        elif p_bc[q] == 0:
            assert np.array_equal(pb[idx], p[own])
        elif q == 4:
            assert np.all(pb[idx] > p[own])                  # fixedFluxPressure on the bottom under gravity: p_P + snGrad / deltaCoeff lies above the cell's value
        want = np.full(len(idx), T_val[q]) if T_bc[q] == 1 else T[own]
        assert np.array_equal(Tb[idx], want)


@pytest.mark.parametrize("solver", [0, 1])
def test_boundary_readouts(product, solver):
    pbc = [2 if solver else 0] * 5 + [1]
    args = ([2, 0, 1, 0, 0, 1], [(0, 0, 0)] * 4 + [(0.01, 0.0, 0.1), (0, 0, 0)], pbc, [0, 0, 0, 0, 0, 2.5], [0, 0, 0, 1, 1, 0], [0, 0, 0, 320.0, 350.0, 0])
    s = block_solver(product, solver, 5, 6, 7)
    view = BlockView(s, 5, 6, 7, 0.01)
    assert s.get("p_boundary").size == view.nb == 2 * (42 + 35 + 30) and s.get("U_boundary").size == 3 * view.nb
    for _ in range(2):
        s.step()
    check_readouts(view, *args)
    with pytest.raises(product.FoamYadeError):
        s.set("p_boundary", np.zeros(view.nb))               # read-outs only
    s.close()
    cold = product.Solver(product.make_case(0, 4, 4, 4, 0.01, 1e-3, 1e-3))
    with pytest.raises(product.FoamYadeError) as e:
        cold.get("T_boundary")
    assert "thermal" in str(e.value)
    cold.close()
    mesh = MESHES["hex"]()
    s = ldu_solver(product, solver, mesh)
    for _ in range(2):
        s.step()
    view = LduView(s, mesh)
    check_readouts(view, *args)
    with pytest.raises(product.FoamYadeError):
        s.set("U_boundary", np.zeros(3 * view.nb))
    s.close()
    slabs = product.VirtualSlabs(product.make_case(0, 8, 8, 16, 0.1 / 8, 0.005, 0.01, p_bc=[0] * 6), 2)
    for sl in slabs.solvers:
        with pytest.raises(product.FoamYadeError) as e:
            sl.get("p_boundary")
        assert "error 5" in str(e.value)
    slabs.close()


def test_readouts_share_nut_boundary_face_order(product):
    """kEqn with nutkWallFunction on two patches of a sheared general mesh: "nearWallDist" and "nut_boundary" are non-zero exactly on those patches' faces, and on the
    same indices U_boundary is the wall's value and p_boundary the owner cell's -- one boundary-face order for all four arrays"""
    mesh = MESHES["hex"]()
    wall = [0, 3]
    u_val = [(0, 0, 0)] * 6
    u_val[5] = (0.3, 0, 0.1)
    turb = dict(turbulence_model=2, nut_initial=3e-5, les_delta_coeff=0.8, k_initial=5e-3, k_tol=1e-13, k_convection_scheme=1, k_relax=0.8, wf_kappa=0.4, wf_E=9.0)
    s = product.LduSolver(mesh, 2e-4, 1e-5, [0] * 6, u_val, [0, 0, 0, 0, 0, 1], solver=1, n_outer_correctors=1, n_correctors=2, p_max_iter=5000, n_non_orth=1,
                          nut_bc=[2 if q in wall else 0 for q in range(6)], nut_val=[1e-5 if q in wall else 0.0 for q in range(6)], **turb)
    for _ in range(2):
        s.step()
    view = LduView(s, mesh)
    idx = np.concatenate([view.members(q) for q in wall])
    y, nutb = s.get("nearWallDist"), s.get("nut_boundary")
    assert y.size == nutb.size == view.nb and np.array_equal(np.flatnonzero(y > 0), np.sort(idx))
    nut = s.get("nut")
    others = np.setdiff1d(np.arange(view.nb), idx)
    assert np.array_equal(nutb[others], nut[view.owner[others]])                      # zeroGradient nut: the owner's value, in this order
    assert not view.face("U")[idx].any() and np.array_equal(view.face("p")[idx], view.cell("p")[view.owner[idx]])
    lid = view.members(5)
    assert np.array_equal(view.face("U")[lid], np.tile(u_val[5], (len(lid), 1))) and not view.face("p")[lid].any()
    s.close()


# ------------------------------------------------------------------------------------------------ 4. known answers
def test_through_flow(product):
    """a channel with a uniform fixedValue inlet and a fixed-pressure outlet: sum(phi) on the inlet is -U_in A within the summation bound, and the sums over all
    sides add up to the volume-integrated divergence the step reports as its global continuity error"""
    nx, ny, nz, dx, uin = 5, 6, 7, 0.01, 0.1
    c = product.make_case(0, nx, ny, nz, dx, 2e-4, 1e-5, u_bc=[2, 2, 2, 2, 0, 1], u_val=[(0, 0, 0)] * 4 + [(0, 0, uin), (0, 0, 0)], p_bc=[0] * 5 + [1])
    s = product.Solver(c)
    objs = [dict(name=f"side{q}", kind="surface", patch=1 << q, operation="sum", fields=["phi"]) for q in range(6)]
    s.set_monitors(objs)
    for _ in range(3):
        s.step()
    flows = np.array([s.monitor_rows(q)[1][-1, 0] for q in range(6)])
    n_in, area = nx * ny, nx * ny * dx * dx
    assert abs(flows[4] + uin * area) <= 4 * n_in * mr.U * uin * area, (flows[4], uin * area)
    assert flows[5] > 0.9 * uin * area and np.all(flows[:4] == 0.0)                # slip sides carry no flux at all; what comes in leaves through the outlet
    st = s.stats()
    total_div = st["cont_err_global"] * (nx * ny * nz * dx ** 3) / st["delta_t"]
    nfaces = 3 * nx * ny * nz + nx * ny + ny * nz + nx * nz
    bound = 4 * nfaces * mr.U * 2 * sum(np.abs(s.get(f)).sum() for f in ("phi_x", "phi_y", "phi_z"))       # every face's flux enters two cells' sums
    assert abs(math.fsum(flows) - total_div) <= bound, (math.fsum(flows), total_div, bound)
    s.close()


def test_hydrostatic_column(product):
    """the bed box at rest under g, no particles: areaAverage(p) on the bottom (fixedFluxPressure) minus that on the top is |g| H, to the tolerance of
    test_fv_parity.py::test_hydrostatic_fixed_flux for p at a tight solver tolerance (1e-5 relative)"""
    nx, ny, nz, dx = 12, 12, 24, 0.005
    s = product.Solver(product.make_case(1, nx, ny, nz, dx, 1e-3, 1e-6, g=(0, 0, -G), p_bc=[2] * 6, p_tol=1e-10, p_final_tol=1e-10, p_rel_tol=0.0))
    s.set_monitors([dict(name="bottom", kind="surface", patch=1 << 4, operation="areaAverage", fields=["p"]),
                    dict(name="top", kind="surface", patch=1 << 5, operation="areaAverage", fields=["p"]),
                    dict(name="walls", kind="surface", patch=0b001111, operation="areaAverage", fields=["p"])])
    for _ in range(3):
        s.step()
    pb, pt, pw = (s.monitor_rows(q)[1][-1, 0] for q in range(3))
    H = nz * dx
    assert abs((pb - pt) - G * H) <= 1e-5 * G * H, (pb - pt, G * H)
    assert abs(pw - 0.5 * (pb + pt)) <= 1e-5 * G * H                                  # the four walls see the column's mean
    s.close()


def test_static_bed(product):
    """a resting cloud in the bed box: volIntegrate(alpha) + the particles' volume is the box volume (the deposit's tolerance, 1e-10 relative);
    weightedVolAverage(U) and volAverage(alpha) equal the restatement"""
    nx, ny, nz, dx = 12, 12, 24, 0.005
    s = product.Solver(product.make_case(1, nx, ny, nz, dx, 2e-4, 1e-5, g=(0, 0, -G), p_bc=[2] * 6))
    view = BlockView(s, nx, ny, nz, dx)
    rs = np.random.RandomState(2)
    rec = np.zeros((200, 10))
    rec[:, 0:3] = np.array([0.01, 0.01, 0.01]) + np.array([0.04, 0.04, 0.05]) * rs.random_sample((200, 3))
    rec[:, 9] = 0.0008
    objs = [dict(name="void", kind="vol", operation="volIntegrate", fields=["alpha"]), dict(name="mean", kind="vol", operation="volAverage", fields=["alpha"]),
            dict(name="uw", kind="vol", operation="weightedVolAverage", weight_field="alpha", fields=["U"])]
    rows = run_against_restatement(s, view, objs, 2, lambda step: rec)
    box = nx * ny * nz * dx ** 3
    solids = 200 * 4.0 / 3.0 * math.pi * 0.0008 ** 3
    assert abs(rows[0][-1, 0] + solids - box) <= 1e-10 * box, (rows[0][-1, 0], solids, box)
    assert rows[1][-1, 0] < 1.0
    s.close()


# ------------------------------------------------------------------------------------------------ 5. determinism and non-interference
def test_determinism_and_non_interference(product):
    """two runs of the same 5 coupled steps give bit-identical rows; a run with monitors and one without give bit-identical U, p, phi and forces; without monitors
    the "monitors" clock sees no launch.  The two particles sit nine cells apart: their stencils share no cell, so the scatter's atomic sums -- whose order is the
    one thing in a coupled step that varies from run to run -- have one term each, and the runs themselves can be compared bit for bit"""
    nx, ny, nz, dx = 6, 6, 16, 0.01
    rec = np.zeros((2, 10))
    rec[:, 0:3] = [(0.031, 0.029, 0.032), (0.028, 0.033, 0.124)]
    rec[:, 3:6] = [(0.01, 0.0, -0.05), (0.0, 0.02, -0.03)]
    rec[:, 9] = 0.002
    objs = [dict(name="v", kind="vol", operation="volAverage", fields=["p", "U", "alpha"]), dict(name="s", kind="surface", patch=1 << 4, operation="areaAverage", fields=["p", "phi"]),
            dict(name="m", kind="vol", operation="max", fields=["U"])]
    out = []
    for on in (True, True, False):
        s = product.Solver(product.make_case(1, nx, ny, nz, dx, 2e-4, 1e-5, g=(0, 0, -G), p_bc=[2] * 6))
        s.enable_kernel_timing(True)
        if on:
            s.set_monitors(objs)
        forces = []
        for step in range(5):
            s.set_particles(rec); s.step(); forces.append(s.forces())
        res = {nm: s.get(nm) for nm in ("U", "p", "phi_x", "phi_y", "phi_z")}
        res["forces"] = np.array(forces)
        res["rows"] = [np.column_stack(s.monitor_rows(q)) for q in range(3)] if on else None
        ms, launches = s.kernel_timing("monitors")
        assert (launches > 0) == on and (ms > 0) == on, (on, ms, launches)
        out.append(res)
        s.close()
    for nm in ("U", "p", "phi_x", "phi_y", "phi_z", "forces"):
        assert np.array_equal(out[0][nm], out[2][nm]), nm                          # monitors on or off: the same run
    for a, b in zip(out[0]["rows"], out[1]["rows"]):
        assert a.shape[0] == 5 and np.array_equal(a, b), (a, b)                    # bit-identical rows from run to run
    assert np.abs(out[0]["forces"]).max() > 0 and out[0]["rows"][0][-1, -1] < 1.0


# ------------------------------------------------------------------------------------------------ 6. ring wrap
def test_ring_wrap(product):
    """a ring of 3 rows and 10 samples (an object with interval 3 beside it): the history is complete and in order, and rows can be fetched from any start"""
    s = block_solver(product, 0, 5, 6, 7, thermal=False)
    view = BlockView(s, 5, 6, 7, 0.01)
    objs = [dict(name="a", kind="vol", operation="volAverage", fields=["p", "U"]), dict(name="b", kind="surface", patch=1 << 5, operation="sum", fields=["phi"], interval=3)]
    rows = run_against_restatement(s, view, objs, 10, ring_rows=3)
    assert rows[0].shape == (10, 4) and rows[1].shape == (3, 1)
    t, v = s.monitor_rows(0)
    assert np.all(np.diff(t) > 0)
    t7, v7 = s.monitor_rows(0, first_row=7)
    assert np.array_equal(t7, t[7:]) and np.array_equal(v7, v[7:])
    s.set_monitors(None)
    with pytest.raises(product.FoamYadeError):
        s.monitor_rows(0)
    s.close()


# ------------------------------------------------------------------------------------------------ 7. refusals through the ABI
BAD = [
    (dict(name="o1", kind="vol", operation="volAverage", fields=["vorticity"]), "'vorticity'"),
    (dict(name="o2", kind="vol", operation="volAverage", fields=["k"]), "'k'"),                                 # laminar: the case has no k
    (dict(name="o3", kind="vol", operation="areaAverage", fields=["p"]), "areaAverage"),
    (dict(name="o4", kind="surface", patch=1, operation="volIntegrate", fields=["p"]), "volIntegrate"),
    (dict(name="o5", kind="vol", operation=99, fields=["p"]), "operation 99"),
    (dict(name="o6", kind="vol", operation="weightedVolAverage", fields=["U"]), "weight field"),
    (dict(name="o7", kind="surface", patch=1, operation="weightedAverage", fields=["U"]), "weight field"),
    (dict(name="o8", kind="surface", patch=0, operation="sum", fields=["phi"]), "empty"),
    (dict(name="o9", kind="surface", patch=1, operation="sum", fields=["alpha"]), "'alpha'"),
    (dict(name="o10", kind="surface", patch=1, operation="sum", fields=["T"]), "'T'"),                           # thermal is off
    (dict(name="o11", kind="vol", operation="sum", fields=["p"] * 9), "9 fields"),
    (dict(name="o12", kind="vol", operation="sum", fields=["p", "p"]), "twice"),
]


@pytest.mark.parametrize("obj,word", BAD, ids=[b[0]["name"] for b in BAD])
def test_refusals(product, obj, word):
    s = product.Solver(product.make_case(1, 6, 6, 6, 0.01, 2e-4, 1e-5, p_bc=[2] * 6))
    with pytest.raises(product.FoamYadeError) as e:
        s.set_monitors([dict(name="fine", kind="vol", operation="sum", fields=["p"]), obj])
    assert "error 1" in str(e.value) and word in str(e.value) and obj["name"] in str(e.value), str(e.value)      # FY_ERR_INVALID, naming the object and the word
    with pytest.raises(product.FoamYadeError):
        s.monitor_rows(0)                                                                                       # a refused call leaves the monitors off
    s.close()


def test_refusals_of_counts_slabs_and_cyclic_patches(product):
    s = product.Solver(product.make_case(1, 6, 6, 6, 0.01, 2e-4, 1e-5, p_bc=[2] * 6))
    with pytest.raises(product.FoamYadeError) as e:
        s.set_monitors([dict(name=f"o{q}", kind="vol", operation="sum", fields=["p"]) for q in range(9)])
    assert "error 1" in str(e.value) and "9 objects" in str(e.value)
    s.close()
    case = product.make_case(0, 8, 8, 16, 0.1 / 8, 0.005, 0.01, p_bc=[0] * 6)
    slabs = product.VirtualSlabs(case, 2)
    for sl in slabs.solvers:
        with pytest.raises(product.FoamYadeError) as e:
            sl.set_monitors([dict(name="v", kind="vol", operation="sum", fields=["p"])])
        assert "error 5" in str(e.value) and "slab" in str(e.value)                                             # FY_ERR_UNSUPPORTED
    slabs.close()
    case.monitors = product.monitor_desc([dict(name="late", kind="vol", operation="sum", fields=["nut"])])     # the descriptor of a case applies at create
    with pytest.raises(product.FoamYadeError) as e:
        product.Solver(case)
    assert "'nut'" in str(e.value) and "late" in str(e.value)
    mesh = pm.make_cyclic(pm.hex_block(4, 3, 5, (0.04, 0.03, 0.05)), [(0, 1)])
    s = product.LduSolver(mesh, 2e-4, 1e-5, [1, 1, 0, 0, 0, 0], [(0, 0, 0)] * 5 + [(0.1, 0, 0)], [0] * 6, n_non_orth=0)
    for patch, word in ((0, "cyclic"), (1, "cyclic"), (6, "does not exist")):
        with pytest.raises(product.FoamYadeError) as e:
            s.set_monitors([dict(name="wrap", kind="surface", patch=patch, operation="sum", fields=["phi"])])
        assert "error 1" in str(e.value) and "wrap" in str(e.value) and word in str(e.value), str(e.value)
    s.set_monitors([dict(name="lid", kind="surface", patch=5, operation="areaAverage", fields=["U"])])
    s.step()
    assert np.array_equal(s.monitor_rows(0)[1][0], [0.1, 0.0, 0.0])
    s.close()


# ------------------------------------------------------------------------------------------------ 9. the ABI
def test_symbols_are_exported(product):
    L = product.lib()
    for pre in ("fy_solver", "fy_ldu_solver"):
        for fn in ("set_monitors", "monitor_layout", "get_monitor_rows"):
            assert hasattr(L, f"{pre}_{fn}")
    assert C.sizeof(product.MonitorObject) == 32 + 12 + 32 + 8 + 8 * 32 and product.MONITOR_MAX_OBJECTS == 8
