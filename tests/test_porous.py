"""Porous zones (fy_solver_set_porous_zones, fy_ldu_solver_set_porous_zones): the Darcy-Forchheimer resistance on the momentum matrix's per-component diagonal, in both
solvers, against tests/porous_ref.py fed the fields read back from the device.

1. rows: the matrix of one step with and without zones, entry by entry (7 x 6 x 5 block, uniform and graded, and poly_meshes' wavy renumbered block)
2. lattice: fy_solver on a 10^3 block against fy_ldu_solver on the same block written as a renumbered polyhedral mesh
3. the known answer: the z-momentum balance of a duct with a zone, with F_z formed in numpy from the read U
4. off is off, and a zone set can be removed; 5. the setter's refusals"""
import numpy as np
import pytest

import poly_meshes as pm
import porous_ref as pr

pytestmark = pytest.mark.gpu
EPS = pr.EPS
TIGHT = dict(p_tol=1e-11, p_rel_tol=0.0, p_final_tol=1e-11, u_tol=1e-11, p_max_iter=5000)


def box(nx, ny, i, j, k):
    """lattice labels i + nx (j + ny k) of the cells with indices in the three ranges"""
    I, J, K = np.meshgrid(np.arange(*i), np.arange(*j), np.arange(*k), indexing="ij")
    return np.sort((I + nx * (J + ny * K)).ravel()).astype(np.int32)


def two_zones(nx, ny, relabel=None):
    """d and f different in every component; 'corner' touches the x- side (slip in the row tests), an edge and a corner of the block"""
    z = [dict(name="corner", cells=box(nx, ny, (0, 2), (0, 3), (0, 2)), d=(3e4, 7e3, 1.1e5), f=(40.0, 15.0, 90.0)),
         dict(name="inner", cells=box(nx, ny, (3, 6), (2, 5), (2, 5)), d=(2e3, 5e4, 9e3), f=(8.0, 120.0, 33.0))]
    if relabel is not None:
        for o in z:
            o["cells"] = np.sort(relabel[o["cells"]]).astype(np.int32)
    return z


def zeroed(zones):
    return [dict(o, d=(0, 0, 0), f=(0, 0, 0)) for o in zones]


def rel_err(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


# ------------------------------------------------------------------------------------------------ 1. rows
NX, NY, NZ = 7, 6, 5
GRADING = (0.01 * 1.15 ** np.arange(NX), 0.012 * 0.9 ** np.arange(NY), 0.008 * 1.1 ** np.arange(NZ))


def block_rows(product, solver, graded, zones, relax, U0, alpha0):
    pim = solver == 1
    case = product.make_case(solver, NX, NY, NZ, 0.01, 2e-4, 1e-5, g=(0, 0, -9.81) if pim else (0, 0, 0), u_bc=[2, 0, 1, 0, 0, 1],
                             u_val=[(0, 0, 0)] * 3 + [(0.05, 0, 0.02), (0.01, 0.0, 0.1), (0, 0, 0)], p_bc=[2 if pim else 0] * 5 + [1], p_val=[0, 0, 0, 0, 0, 2.5],
                             grading=GRADING if graded else None, u_relax=relax, u_relax_final=0.0, n_outer_correctors=1)
    s = product.Solver(case)
    s.set("U", U0)
    if pim:
        s.hold_sources(True)
        s.set("alpha", alpha0)
    if zones is not None:
        s.set_porous_zones(zones)
    s.step()
    out = {nm: s.get(nm) for nm in ["mom_diag", "mom_src", "rAU"] + [f"mom_an{q}" for q in range(6)]}
    if pim:
        out["alpha"] = s.get("alpha")
    if zones is not None:
        out["mom_bd"] = s.get("mom_bd").reshape(-1, 3)
        assert np.array_equal(s.get("porousZone"), pr.zone_map(NX * NY * NZ, zones))
    s.close()
    return out


@pytest.mark.parametrize("solver,graded", [(0, False), (0, True), (1, False), (1, True)], ids=["ico-uniform", "ico-graded", "pimple-uniform", "pimple-graded"])
def test_block_rows(product, solver, graded):
    n = NX * NY * NZ
    rs = np.random.RandomState(11)
    U0 = 0.3 * rs.standard_normal((n, 3))
    alpha0 = 0.45 + 0.5 * rs.random_sample(n)
    zones = two_zones(NX, NY)
    if graded:
        k, j, i = np.meshgrid(np.arange(NZ), np.arange(NY), np.arange(NX), indexing="ij")
        V = ((GRADING[0][i] * GRADING[1][j]) * GRADING[2][k]).ravel()
    else:
        V = np.full(n, (0.01 * 0.01) * 0.01)
    run = lambda z, relax=0.0: block_rows(product, solver, graded, z, relax, U0, alpha0)
    none, base, got = run(None), run(zeroed(zones)), run(zones)
    a = got["alpha"] if solver == 1 else np.ones(n)
    if solver == 1:
        assert np.array_equal(a, alpha0) and a.min() < 0.9                               # the hand-set void fraction is what the step saw
    for nm in ["mom_diag", "mom_src"] + [f"mom_an{q}" for q in range(6)]:              # no relaxation: the scalar row has the bits of a solver without zones
        assert np.array_equal(got[nm], none[nm]) and np.array_equal(base[nm], none[nm]), nm
    assert np.array_equal(base["rAU"], none["rAU"])
    pc = pr.diagonal_additions(n, zones, a, V, 1e-5, U0)
    inz = pc.any(axis=1)
    assert inz.sum() == 12 + 27 and base["mom_bd"][inz].any()                          # a zone's cells on the slip side carry both parts
    want = base["mom_bd"] + pc
    e = rel_err(got["mom_bd"][inz], want[inz]).max()
    print("mom_bd: max relative error / eps", e / EPS)
    assert e <= 4 * EPS
    assert np.array_equal(got["mom_bd"][~inz], base["mom_bd"][~inz])
    bd = got["mom_bd"]
    e = rel_err(got["rAU"], V / (got["mom_diag"] + ((bd[:, 0] + bd[:, 1]) + bd[:, 2]) / 3.0)).max()
    print("rAU: max relative error / eps", e / EPS)
    assert e <= 4 * EPS
    assert np.all(got["rAU"][inz] < none["rAU"][inz])
    if solver == 1:                                                                     # UcEqn.relax(0.7): the dominance test with the porous part's component maximum
        rel = run(zones, 0.7)
        off = np.zeros(n)
        for q in range(6):
            off = off + np.abs(got[f"mom_an{q}"])
        bb = base["mom_bd"]
        dn, src = pr.relaxed(got["mom_diag"], got["mom_src"].reshape(-1, 3), U0, off, (bb[:, 0] + bb[:, 1]) + bb[:, 2], 0.0, pc, 0.7)
        e = rel_err(rel["mom_diag"], dn).max()
        es = (np.abs(rel["mom_src"].reshape(-1, 3) - src) / (np.abs(got["mom_src"].reshape(-1, 3)) + (np.abs(dn) + np.abs(got["mom_diag"]))[:, None] * np.abs(U0))).max()
        print("relaxed diag / src: max relative error / eps", e / EPS, es / EPS)
        assert e <= 4 * EPS and es <= 4 * EPS
        plain = run(None, 0.7)
        assert np.array_equal(plain["mom_diag"][~inz], rel["mom_diag"][~inz]) and np.all(rel["mom_diag"][inz] > plain["mom_diag"][inz])


def ldu_rows(product, mesh, solver, zones, relax, U0, alpha0):
    pim = solver == 1
    kw = dict(solver=1, g=(0, 0, -9.81), n_outer_correctors=1, u_relax=relax, u_relax_final=0.0) if pim else {}
    s = product.LduSolver(mesh, 2e-4, 1e-5, [2, 0, 1, 0, 0, 1], [(0, 0, 0)] * 3 + [(0.05, 0, 0.02), (0.01, 0.0, 0.1), (0, 0, 0)], [2 if pim else 0] * 5 + [1], [0, 0, 0, 0, 0, 2.5], **kw)
    s.set("U", U0)
    if pim:
        s.hold_sources(True)
        s.set("alpha", alpha0)
    if zones is not None:
        s.set_porous_zones(zones)
    s.step()
    out = {nm: s.get(nm) for nm in ["mom_diag", "mom_b", "mom_lower", "mom_upper", "rAU", "V"]}
    if zones is not None:
        out["mom_bd"] = s.get("mom_bd").reshape(-1, 3)
        assert np.array_equal(s.get("porousZone"), pr.zone_map(U0.shape[0], zones))
    s.close()
    return out


@pytest.mark.parametrize("solver", [0, 1], ids=["ico", "pimple"])
def test_general_mesh_rows(product, solver):
    L = (0.07, 0.06, 0.05)
    mesh = pm.hex_block(NX, NY, NZ, L, pm.wavy(0.002, L), renumber_seed=4)
    n = NX * NY * NZ
    rs = np.random.RandomState(12)
    U0 = 0.3 * rs.standard_normal((n, 3))
    alpha0 = 0.45 + 0.5 * rs.random_sample(n)
    zones = two_zones(NX, NY, relabel=mesh["perm"])
    run = lambda z, relax=0.0: ldu_rows(product, mesh, solver, z, relax, U0, alpha0)
    none, base, got = run(None), run(zeroed(zones)), run(zones)
    for nm in ["mom_diag", "mom_b", "mom_lower", "mom_upper"]:
        assert np.array_equal(got[nm], none[nm]) and np.array_equal(base[nm], none[nm]), nm
    a = alpha0 if solver == 1 else np.ones(n)
    V = got["V"]
    pc = pr.diagonal_additions(n, zones, a, V, 1e-5, U0)
    inz = pc.any(axis=1)
    assert inz.sum() == 39 and base["mom_bd"][inz].any()
    e = rel_err(got["mom_bd"][inz], (base["mom_bd"] + pc)[inz]).max()
    print("mom_bd: max relative error / eps", e / EPS)
    assert e <= 4 * EPS
    assert np.array_equal(got["mom_bd"][~inz], base["mom_bd"][~inz])
    bd = got["mom_bd"]
    if solver == 1:                                                                     # (icoFoamYade forms rAU after the predictor, from the same diagonal: k_ldu_HbyA)
        e = rel_err(got["rAU"], V / (got["mom_diag"] + (bd[:, 0] + bd[:, 1] + bd[:, 2]) / 3.0)).max()
        print("rAU: max relative error / eps", e / EPS)
        assert e <= 4 * EPS
    else:
        e = rel_err(got["rAU"], 1.0 / ((got["mom_diag"] + (bd[:, 0] + bd[:, 1] + bd[:, 2]) / 3.0) / V)).max()
        print("rAU: max relative error / eps", e / EPS)
        assert e <= 4 * EPS
    assert np.all(got["rAU"][inz] < none["rAU"][inz])
    if solver == 1:
        rel = run(zones, 0.7)
        own, nei = np.asarray(mesh["owner"]), np.asarray(mesh["neighbour"])
        ni = nei.size
        off = np.zeros(n)
        np.add.at(off, own[:ni], np.abs(got["mom_upper"])); np.add.at(off, nei, np.abs(got["mom_lower"]))
        bb = base["mom_bd"]                                                             # one slip patch: a cell has at most one of its faces, so bmax / bmin are the row's extremes
        dn, src = pr.relaxed(got["mom_diag"], got["mom_b"].reshape(-1, 3), U0, off, bb.max(axis=1), bb.min(axis=1), pc, 0.7)
        # sum |offdiag| is added in another order here (<= 6 terms: 5 eps), then one division and one subtraction
        e = (np.abs(rel["mom_diag"] - dn) / (np.abs(dn) + bb.min(axis=1))).max()
        es = (np.abs(rel["mom_b"].reshape(-1, 3) - src) / (np.abs(got["mom_b"].reshape(-1, 3)) + (np.abs(dn) + np.abs(got["mom_diag"]))[:, None] * np.abs(U0))).max()
        print("relaxed diag / b: max relative error / eps", e / EPS, es / EPS)
        assert e <= 8 * EPS and es <= 8 * EPS
        plain = run(None, 0.7)
        assert np.array_equal(plain["mom_diag"][~inz], rel["mom_diag"][~inz]) and np.all(rel["mom_diag"][inz] > plain["mom_diag"][inz])


# ------------------------------------------------------------------------------------------------ 2. lattice
def close(a, b, rtol, what):
    sc = np.abs(b).max() + 1e-300
    print(what, np.abs(a - b).max() / sc)
    assert np.abs(a - b).max() <= rtol * sc, (what, np.abs(a - b).max() / sc)


@pytest.mark.parametrize("solver", ["ico", "pimple"])
def test_lattice_equals_the_structured_solver(product, solver):
    """tests/test_ldu_parity.py's lattice cavity with two zones (Forchheimer, an anisotropic d) through both solvers, three steps, to that file's tolerances"""
    n = 10
    u_bc = [2, 0, 0, 0, 0, 0]
    u_val = [(0, 0, 0)] * 6
    u_val[3] = (1.0, 0, 0.3)
    mesh = pm.hex_block(n, n, n, renumber_seed=6)
    tol = dict(p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10)
    zf = [dict(name="corner", cells=box(n, n, (0, 3), (0, 4), (6, 10)), d=(4e2, 9e3, 2e1), f=(30.0, 4.0, 70.0)),
          dict(name="inner", cells=box(n, n, (4, 8), (5, 9), (2, 6)), d=(6e3, 1e2, 3e3), f=(5.0, 60.0, 12.0))]
    zg = [dict(o, cells=np.sort(mesh["perm"][o["cells"]]).astype(np.int32)) for o in zf]
    def block():
        if solver == "ico":
            return product.Solver(product.make_case(0, n, n, n, 1.0 / n, 0.4 / n, 0.01, u_bc=u_bc, u_val=u_val, p_solver=0, **tol))
        return product.Solver(product.make_case(1, n, n, n, 1.0 / n, 0.4 / n, 0.01, g=(0, 0, -9.81), u_bc=u_bc, u_val=u_val, p_bc=p_bc, p_solver=0, n_outer_correctors=2, n_correctors=2, p_max_iter=5000, **rel, **tol))

    rel = dict(u_relax=0.7, u_relax_final=1.0, p_relax=0.6, p_relax_final=1.0)
    p_bc = [0, 2, 2, 2, 2, 2]
    if solver == "ico":
        g = product.LduSolver(mesh, 0.4 / n, 0.01, u_bc, u_val, [0] * 6, p_max_iter=5000, **tol)
    else:
        g = product.LduSolver(mesh, 0.4 / n, 0.01, u_bc, u_val, p_bc, solver=1, g=(0, 0, -9.81), n_outer_correctors=2, n_correctors=2, p_max_iter=5000, **rel, **tol)
    f, plain = block(), block()                                                         # plain: the same run without zones
    f.set_porous_zones(zf); g.set_porous_zones(zg)
    U0 = np.random.RandomState(2).rand(n ** 3, 3) * 0.05
    f.set("U", U0); plain.set("U", U0)
    Ug = np.zeros_like(U0); Ug[mesh["perm"]] = U0
    g.set("U", Ug)
    for _ in range(3):
        f.step(); g.step(); plain.step()
    Uf = f.get("U").reshape(-1, 3)
    assert np.abs(Uf).max() > 0.1
    close(pm.to_lattice(mesh, g.get("U").reshape(-1, 3)), Uf, 1e-7, "U")
    # the zones act: the same run without them ends elsewhere, by far more than the tolerance the two solvers are held to
    moved = np.abs(plain.get("U").reshape(-1, 3) - Uf).max() / np.abs(Uf).max()
    print("zones against no zones: max |dU| / max |U|", moved)
    assert moved > 1e-3
    pf, pg = f.get("p"), pm.to_lattice(mesh, g.get("p"))
    close(pg - pg.mean(), pf - pf.mean(), 1e-6, "p")
    sf, sg = f.porous_stats(), g.porous_stats()
    for a, b in zip(sf, sg):
        assert a["cells"] == b["cells"] and abs(a["volume"] - b["volume"]) <= 1e-12 * a["volume"]
        close(b["force"], a["force"], 1e-6, "force")
    f.close(); g.close(); plain.close()


# ------------------------------------------------------------------------------------------------ 3. the known answer
W, NU, H = 0.1, 1e-3, 0.01
DUCT = (4, 4, 24)
# relative imbalance of the z-momentum measured on the MI355X (DESIGN_HISTORY.md "Porous zones"): block BALANCE_MEASURED[0], lattice as a general mesh [1]; the bound
# is ten times the larger, and may not exceed 1e-6 (a missing 1/2, nu or alpha moves the balance at order one)
BALANCE_MEASURED = (3.9e-14, 3.8e-13)
BALANCE_BOUND = min(10 * max(BALANCE_MEASURED), 1e-6)


def duct(product, kind):
    nx, ny, nz = DUCT
    u_bc, p_bc = [2, 2, 2, 2, 0, 1], [0, 0, 0, 0, 0, 1]
    u_val = [(0, 0, 0)] * 4 + [(0, 0, W), (0, 0, 0)]
    tol = dict(p_tol=1e-13, p_rel_tol=0.0, p_final_tol=1e-13, u_tol=1e-13, p_max_iter=5000)
    cells = box(nx, ny, (0, nx), (0, ny), (8, 16))
    if kind == "block":
        s = product.Solver(product.make_case(0, nx, ny, nz, H, 0.02, NU, u_bc=u_bc, u_val=u_val, p_bc=p_bc, p_val=[0, 0, 0, 0, 0, 1.5], p_solver=0, **tol))
        relabel = np.arange(nx * ny * nz)
    else:
        mesh = pm.hex_block(nx, ny, nz, (nx * H, ny * H, nz * H), renumber_seed=3)
        s = product.LduSolver(mesh, 0.02, NU, u_bc, u_val, p_bc, [0, 0, 0, 0, 0, 1.5], **tol)
        relabel = mesh["perm"]
    zone = dict(name="plate", cells=np.sort(relabel[cells]).astype(np.int32), d=(0, 0, 4e4), f=(0, 0, 300.0))
    s.set_porous_zones([zone])
    U = np.zeros((nx * ny * nz, 3)); U[:, 2] = W
    s.set("U", U)
    change = 1.0
    for step in range(600):
        s.step()
        Un = s.get("U").reshape(-1, 3)
        change = np.abs(Un - U).max()
        U = Un
        if change < 1e-10 * W:
            break
    print(kind, "steps", step + 1, "last change / W", change / W)
    assert change < 1e-10 * W
    return s, zone, relabel


@pytest.mark.parametrize("kind", ["block", "general"])
def test_duct_momentum_balance(product, kind):
    """(p_in - p_out) A = F_z + W A (U_P,out - W) - nu A (W - U_P,in) / (h / 2): the discrete operators telescope over the cells of a duct with slip sides; F_z from numpy"""
    nx, ny, nz = DUCT
    s, zone, relabel = duct(product, kind)
    U = s.get("U").reshape(-1, 3)
    pb, Ub = s.get("p_boundary"), s.get("U_boundary").reshape(-1, 3)
    nside = [ny * nz, ny * nz, nx * nz, nx * nz, nx * ny, nx * ny]
    o = np.concatenate([[0], np.cumsum(nside)])
    zin, zout = slice(o[4], o[5]), slice(o[5], o[6])
    A = H * H
    c = zone["cells"]
    V = np.full(c.size, H * H * H)
    F = pr.force(np.ones(c.size), V, NU, zone["d"], zone["f"], U[c])
    cin, cout = relabel[box(nx, ny, (0, nx), (0, ny), (0, 1))], relabel[box(nx, ny, (0, nx), (0, ny), (nz - 1, nz))]
    lhs = (pb[zin] * A).sum() - (pb[zout] * A).sum()
    rhs = F[2] + (W * A * (U[cout, 2] - W)).sum() - (NU * A * (W - U[cin, 2]) / (H / 2)).sum()
    imb = abs(lhs - rhs) / abs(lhs)
    print(kind, "lhs", lhs, "rhs", rhs, "F_z", F[2], "relative imbalance", imb, "bound", BALANCE_BOUND)
    assert np.abs(Ub[zout, 2] - W).max() < 1e-3 * W and F[2] > 0.5 * lhs              # plug flow leaves as it came; the plate carries the pressure drop
    assert imb <= BALANCE_BOUND
    # the statistics: numpy's sums to n_cells eps relative, and the same bits on a repeated call and on a repeated run
    st = s.porous_stats()
    assert len(st) == 1 and st[0]["cells"] == c.size
    terms = pr.row_additions(np.ones(c.size), V, NU, zone["d"], zone["f"], U[c]) * U[c]
    tolF = c.size * EPS * np.abs(terms).sum(axis=0)
    print("stats force", st[0]["force"], "numpy", F, "err", np.abs(st[0]["force"] - F), "tol", tolF)
    assert np.all(np.abs(st[0]["force"] - F) <= tolF)
    assert abs(st[0]["volume"] - V.sum()) <= c.size * EPS * V.sum() and abs(st[0]["void_volume"] - V.sum()) <= c.size * EPS * V.sum()
    again = s.porous_stats()
    assert np.array_equal(again[0]["force"], st[0]["force"]) and again[0]["volume"] == st[0]["volume"] and again[0]["void_volume"] == st[0]["void_volume"]
    s.close()
    s2, _, _ = duct(product, kind)                                                      # the whole run once more, from a new solver
    rerun = s2.porous_stats()
    assert np.array_equal(s2.get("U").reshape(-1, 3), U)
    assert np.array_equal(rerun[0]["force"], st[0]["force"]) and rerun[0]["volume"] == st[0]["volume"] and rerun[0]["void_volume"] == st[0]["void_volume"]
    s2.close()


# ------------------------------------------------------------------------------------------------ 4. off is off, and replaceable
def cavity(product, kind, slip=False):
    n = 6
    u_bc = [2 if slip else 0, 0, 0, 0, 0, 0]
    u_val = [(0, 0, 0)] * 6
    u_val[3] = (1.0, 0, 0.3)
    if kind == "block":
        return product.Solver(product.make_case(0, n, n, n, 1.0 / n, 0.05, 0.01, u_bc=u_bc, u_val=u_val, p_solver=0))
    return product.LduSolver(pm.hex_block(n, n, n, renumber_seed=5), 0.05, 0.01, u_bc, u_val, [0] * 6)


@pytest.mark.parametrize("kind", ["block", "general"])
def test_off_is_off_and_replaceable(product, kind):
    never, was = cavity(product, kind), cavity(product, kind)
    zones = [dict(name="a", cells=[0, 1, 7, 100], d=(1e4, 0, 0), f=(0, 3.0, 0)), dict(name="b", cells=np.arange(150, 180), d=(0, 5e3, 1e3), f=(1.0, 1.0, 1.0))]
    was.enable_kernel_timing(True)
    was.set_porous_zones(zones)
    was.set_porous_zones(zones[::-1])                                                   # a set replaces a set
    assert [z["cells"] for z in was.porous_stats()] == [30, 4]
    assert was.kernel_timing("porous_force")[1] == 1
    was.set_porous_zones(None)
    was.enable_kernel_timing(True)                                                      # (resets the clocks)
    for _ in range(2):
        never.step(); was.step()
    for nm in ("U", "p", "rAU", "mom_diag"):
        assert np.array_equal(never.get(nm), was.get(nm)), nm
    assert was.kernel_timing("porous_force")[1] == 0                                    # no zone: no k_porous_force launch
    slip = cavity(product, kind, slip=True)
    slip.step()
    for s in (was, slip):                                                               # unknown names without a zone, with or without a slip side
        for nm in ("mom_bd", "porousZone"):
            with pytest.raises(product.FoamYadeError) as e:
                s.get(nm)
            assert nm in str(e.value)
        with pytest.raises(product.FoamYadeError) as e:
            s.porous_stats()
        assert "no porous zone" in str(e.value)
    # zones in between: a step with them differs, and after their removal the next step is the plain solver's again from the same state
    was.set_porous_zones(zones); never.set_porous_zones(zones)
    was.step(); never.step()
    was.set_porous_zones([]); never.set_porous_zones(None)
    was.step(); never.step()
    assert np.array_equal(never.get("U"), was.get("U"))
    for s in (never, was, slip):
        s.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
@pytest.mark.parametrize("kind", ["block", "general"])
def test_setter_refusals_by_name(product, kind):
    s = cavity(product, kind)
    ok = dict(name="plate", cells=[3, 4, 5], d=(1, 2, 3), f=(4, 5, 6))
    bad = [([dict(ok, cells=[q]) for q in range(9)], "FY_POROUS_MAX_ZONES"),
           ([dict(ok, cells=[])], "empty"),
           ([dict(ok, cells=[3, 216])], "out of range"),
           ([dict(ok, cells=[3, -1])], "out of range"),
           ([ok, dict(ok, name="sieve", cells=[9, 4])], "two porous zones"),
           ([dict(ok, cells=[3, 4, 3])], "twice"),
           ([dict(ok, d=(1, -2, 3))], "d[1]"),
           ([dict(ok, f=(4, 5, np.inf))], "f[2]"),
           ([dict(ok, d=(np.nan, 2, 3))], "d[0]")]
    for zones, word in bad:
        with pytest.raises(product.FoamYadeError) as e:
            s.set_porous_zones(zones)
        assert "error 1" in str(e.value) and word in str(e.value), (word, str(e.value))     # FY_ERR_INVALID
        if "MAX" not in word:
            assert "plate" in str(e.value) or "sieve" in str(e.value)
        with pytest.raises(product.FoamYadeError):
            s.get("porousZone")                                                             # a refused call sets nothing
    s.set_porous_zones([ok])
    with pytest.raises(product.FoamYadeError):
        s.set_porous_zones([dict(ok, cells=[])])
    assert np.count_nonzero(s.get("porousZone")) == 3                                       # ... and leaves the zones that were set
    for nm in ("porousZone", "mom_bd"):
        with pytest.raises(product.FoamYadeError) as e:
            s.set(nm, s.get(nm))
        assert nm in str(e.value)
    s.close()


def test_slabs_are_refused(product):
    case = product.make_case(0, 8, 8, 16, 0.1 / 8, 0.005, 0.01, p_bc=[0] * 6)
    slabs = product.VirtualSlabs(case, 2)                                                   # fy_solver_create_slab over a local group
    for sl in slabs.solvers:
        with pytest.raises(product.FoamYadeError) as e:
            sl.set_porous_zones([dict(name="plate", cells=[0, 1], d=(1, 1, 1), f=(0, 0, 0))])
        assert "error 5" in str(e.value) and "slab" in str(e.value)                         # FY_ERR_UNSUPPORTED
        sl.set_porous_zones(None)                                                           # nothing to remove: accepted
    slabs.close()
