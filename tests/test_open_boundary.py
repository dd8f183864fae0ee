"""Open boundaries on general meshes on the device (inletOutlet, pressureInletOutletVelocity; include/foamyade_hip.h "Open boundaries").  The CPU oracle does not know
these conditions, so the references are the device code of the conditions a face must EQUAL -- zeroGradient where the flux leaves, fixedValue where it enters, on a mesh
whose open patch is cut into the two halves -- bit for bit, and tests/open_boundary_ref.py (held to its limits in tests/test_open_boundary_ref.py) where no existing
condition is equal.  The open side is zmax of hex_block(18, 15, 4): 270 faces (more than one 256-lane block, no multiple of 64), 1080 cells."""
import numpy as np
import pytest

import open_boundary_ref as ob
import poly_meshes as pm

pytestmark = pytest.mark.gpu

NX, NY, NZ = 18, 15, 4
LEN = (0.18, 0.15, 0.04)                     # 1 cm cubes
ZMIN, ZMAX = 4, 5
NTOP, HALF = NX * NY, NX * NY // 2           # 270, 135
EPS = np.finfo(np.float64).eps
SOLVE = dict(p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10, p_max_iter=5000)
TURB = dict(turbulence_model=3, nut_initial=2e-5, k_initial=2e-4, eps_initial=1.2e-4, k_tol=1e-12, eps_tol=1e-12)
IO, PIO = 3, 4                               # FY_BC_U_INLET_OUTLET, FY_BC_U_PRESSURE_INLET_OUTLET
S_IO, T_IO = 4, 2                            # FY_BC_NUT_INLET_OUTLET, FY_BC_T_INLET_OUTLET


def tilt(P):
    Q = P.copy()
    Q[:, 2] += 0.2 * P[:, 0] + 0.1 * P[:, 1]      # oblique z faces: n = (-0.2, -0.1, 1) / |.|
    return Q


def block(tilted=True):
    return pm.hex_block(NX, NY, NZ, LEN, tilt if tilted else None)


def split(mesh):
    """the same mesh with its zmax patch cut into two patches (faces [0, 135) and [135, 270) of it); the face order is untouched"""
    m = dict(mesh)
    s = int(mesh["patch_start"][ZMAX])
    m["patch_start"] = np.append(mesh["patch_start"], s + HALF).astype(np.int32)
    m["patch_size"] = np.append(mesh["patch_size"][:ZMAX], [HALF, NTOP - HALF]).astype(np.int32)
    m["patch_names"] = list(mesh["patch_names"]) + ["zmax_b"]
    return m


def top_faces(mesh):
    """the top's faces among the boundary faces (the order of "U_boundary"), and their owner cells"""
    b0 = int(mesh["patch_start"][ZMAX]) - len(mesh["neighbour"])
    return slice(b0, b0 + NTOP), np.asarray(mesh["owner"])[int(mesh["patch_start"][ZMAX]):int(mesh["patch_start"][ZMAX]) + NTOP]


def thermal(product):
    return product.thermal_desc(cp=1000.0, kappa=100.0, prt=0.9, T_initial=300.0, T_tol=1e-14, T_rel_tol=0.0, T_max_iter=2000)


def full_model(product, k_bc, k_val, eps_bc, eps_val, T_bc, T_val, nut_bc, nut_val):
    """pimpleFoamYade + RAS kEpsilon + the T equation: what every closure and the T equation read of a patch"""
    return dict(solver=1, nut_bc=nut_bc, nut_val=nut_val, k_bc=k_bc, k_val=k_val, eps_bc=eps_bc, eps_val=eps_val, thermal=thermal(product), T_bc=T_bc, T_val=T_val, **TURB)


def same(a, b, names):
    for nm in names:
        x, y = a.get(nm), b.get(nm)
        assert np.isfinite(x).all(), nm
        np.testing.assert_array_equal(x, y, err_msg=nm)


# ---- 1. all-outflow equals zeroGradient ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ucode", [IO, PIO])
@pytest.mark.parametrize("mode", ["ico", "pimple"])
def test_all_outflow_equals_zeroGradient(product, mode, ucode):
    """through-flow leaves by the top (bottom fixedValue (0 0 w), p fixed at the top): with the open codes on the top every field has the bits of the run whose top is
    zeroGradient, for U and (pimple + kEpsilon + thermal) for k, epsilon and T; the mask stays empty"""
    mesh, w = block(), 0.5
    U0 = np.array([0, 0, w]) + 0.05 * w * np.random.RandomState(11).standard_normal((mesh["n_cells"], 3))

    def make(open_top):
        u_bc = [0, 0, 0, 0, 0, ucode if open_top else 1]
        u_val = [(0, 0, 0)] * 4 + [(0, 0, w), (0.1, 0.2, -0.3)]
        if mode == "ico":
            return product.LduSolver(mesh, 2e-3, 0.01, u_bc, u_val, [0, 0, 0, 0, 0, 1], n_non_orth=1, **SOLVE)
        s = 1 if open_top else 0
        kw = full_model(product, [0, 0, 0, 0, 1, S_IO * s], [0, 0, 0, 0, 2e-4, 5e-4], [0, 0, 0, 0, 1, S_IO * s], [0, 0, 0, 0, 1.2e-4, 3e-4], [0, 0, 0, 0, 1, T_IO * s], [0, 0, 0, 0, 300.0, 320.0],
                        [0] * 5 + [3], [0] * 5 + [2e-5])
        return product.LduSolver(mesh, 2e-3, 1e-5, u_bc, u_val, [0, 0, 0, 0, 0, 1], n_non_orth=1, **kw, **SOLVE)
    a, b = make(True), make(False)
    for s in (a, b):
        s.set("U", U0)
    for _ in range(10):
        a.step(); b.step()
    same(a, b, ("U", "p", "phi") + (("k", "epsilon", "nut", "T") if mode == "pimple" else ()))
    assert np.abs(a.get("U").reshape(-1, 3) - U0).max() > 1e-3                 # (the run moved)
    assert not a.get("U_open_inflow").any()
    assert a.open_boundary_stats()["inflow_faces"] == 0 and a.open_boundary_stats()["outflow_flux"] > 0
    a.close(); b.close()


# ---- 2. scalar split equivalence -------------------------------------------------------------------------------------------------------------------------------------
def test_scalar_inletOutlet_equals_the_split_patch(product):
    """the top is a fixedValue velocity patch that blows in on its first 135 faces and out on its last 135 (the flux sign is fixed by construction): k, epsilon and T
    inletOutlet on it = fixedValue on the inflow half and zeroGradient on the outflow half of the split mesh, every field bit for bit after 5 steps"""
    mesh, w = block(), 0.2
    shape = np.zeros((NTOP, 3)); shape[:HALF, 2] = -w; shape[HALF:, 2] = w
    U0 = 0.02 * np.random.RandomState(12).standard_normal((mesh["n_cells"], 3))
    kv, ev, tv = 5e-4, 3e-4, 320.0
    a = product.LduSolver(mesh, 1e-3, 1e-5, [0, 0, 0, 0, 1, 0], [(0, 0, 0)] * 6, [0, 0, 0, 0, 1, 0], n_non_orth=1, inlets=[dict(patch=ZMAX, terms=[dict(f=1.0, shape=shape)])],
                          **full_model(product, [0] * 5 + [S_IO], [0] * 5 + [kv], [0] * 5 + [S_IO], [0] * 5 + [ev], [0] * 5 + [T_IO], [0] * 5 + [tv], [0] * 5 + [3], [0] * 5 + [2e-5]), **SOLVE)
    b = product.LduSolver(split(mesh), 1e-3, 1e-5, [0, 0, 0, 0, 1, 0, 0], [(0, 0, 0)] * 7, [0, 0, 0, 0, 1, 0, 0], n_non_orth=1,
                          inlets=[dict(patch=ZMAX, terms=[dict(f=1.0, shape=shape[:HALF])]), dict(patch=ZMAX + 1, terms=[dict(f=1.0, shape=shape[HALF:])])],
                          **full_model(product, [0] * 5 + [1, 0], [0] * 5 + [kv, 0], [0] * 5 + [1, 0], [0] * 5 + [ev, 0], [0] * 5 + [1, 0], [0] * 5 + [tv, 0], [0] * 5 + [3, 3], [0] * 5 + [2e-5, 2e-5]),
                          **SOLVE)
    for s in (a, b):
        s.set("U", U0)
    top, _ = top_faces(mesh)
    pattern = np.r_[np.ones(HALF), np.zeros(NTOP - HALF)]
    np.testing.assert_array_equal(a.get("U_open_inflow")[top], pattern)
    for _ in range(5):
        a.step(); b.step()
    same(a, b, ("U", "p", "phi", "k", "epsilon", "nut", "T", "T_boundary", "nut_boundary"))
    m = a.get("U_open_inflow")
    np.testing.assert_array_equal(m[top], pattern)
    assert m.sum() == HALF                                                     # 0 off the open patch
    T = a.get("T_boundary")[top]
    assert (T[:HALF] == tv).all() and (T[HALF:] != tv).all()
    assert a.open_boundary_stats()["inflow_faces"] == HALF
    with pytest.raises(product.FoamYadeError, match="open"):
        b.get("U_open_inflow")
    a.close(); b.close()


# ---- 3. / 4. the momentum matrix --------------------------------------------------------------------------------------------------------------------------------------
V_IN = (0.3, 0.0, -1.0)


def momentum_state(mesh):
    """a random U whose cells under the last 135 top faces hold exactly V_IN (the flux enters there, and a zeroGradient evaluation of the face gives the inlet value)
    and whose cells under the first 135 have w > 0 (it leaves)"""
    _, own = top_faces(mesh)
    U = 0.1 * np.random.RandomState(13).standard_normal((mesh["n_cells"], 3))
    U[own[:HALF], 2] = np.abs(U[own[:HALF], 2]) + 0.2
    U[own[HALF:]] = V_IN
    return U


def momentum_solver(product, mesh, mode, u_top, u_top_val=((0, 0, 0),)):
    n = len(mesh["patch_start"])
    u_bc = [0] * 5 + list(u_top)
    u_val = [(0, 0, 0)] * 5 + list(u_top_val)
    p_bc = [0] * 5 + [1] * (n - 5)
    kw = dict(n_correctors=1, n_non_orth=1, **SOLVE)
    if mode == "pimple":
        kw["solver"] = 1
    return product.LduSolver(mesh, 1e-3, 0.01 if mode == "ico" else 1e-5, u_bc, u_val, p_bc, **kw)


@pytest.mark.parametrize("mode", ["ico", "pimple"])
def test_momentum_inletOutlet_equals_the_split_patch(product, mode):
    """one step with one corrector: the top inletOutlet with inletValue V_IN = the split mesh with zeroGradient on the outflow half and fixedValue V_IN on the inflow
    half -- phi after the write, rAU and HbyA after the step, bit for bit (later fields differ by design: the open patch does not fix the flux)"""
    mesh = block()
    U0 = momentum_state(mesh)
    a = momentum_solver(product, mesh, mode, [IO], [V_IN])
    b = momentum_solver(product, split(mesh), mode, [1, 0], [(0, 0, 0), V_IN])
    a.set("U", U0); b.set("U", U0)
    top, _ = top_faces(mesh)
    same(a, b, ("phi",))
    np.testing.assert_array_equal(a.get("U_open_inflow")[top], np.r_[np.zeros(HALF), np.ones(NTOP - HALF)])
    ubA, ubB = a.get("U_boundary"), b.get("U_boundary")
    np.testing.assert_array_equal(ubA, ubB)
    a.step(); b.step()
    same(a, b, ("rAU", "HbyA", "mom_diag", "mom_b"))
    assert np.abs(a.get("HbyA")).max() > 0.1
    a.close(); b.close()


@pytest.mark.parametrize("mode", ["ico", "pimple"])
def test_pressureInletOutletVelocity_coefficients_on_a_tilted_top(product, mode):
    """the same state against the run whose top is zeroGradient: per cell under an inflow face V / rAU rises by the component mean of (gm - phi) diag_q
    (tests/open_boundary_ref.py) within 64 eps V / rAU_zg -- a difference of two sums of about ten terms of that size; U_boundary = n (n . U_P) on the inflow faces
    within 8 eps |U_P| (five roundings), and the cell's value exactly on the outflow faces"""
    mesh = block()
    U0 = momentum_state(mesh)
    a = momentum_solver(product, mesh, mode, [PIO])
    z = momentum_solver(product, mesh, mode, [1])
    a.set("U", U0); z.set("U", U0)
    top, own = top_faces(mesh)
    same(a, z, ("phi",))                                                       # createPhi evaluates the open faces as zeroGradient
    phi0 = a.get("phi")[int(mesh["patch_start"][ZMAX]):][:NTOP]
    mask0 = a.get("U_open_inflow")[top].astype(bool)
    np.testing.assert_array_equal(mask0, np.r_[np.zeros(HALF, bool), np.ones(NTOP - HALF, bool)])
    fs = slice(int(mesh["patch_start"][ZMAX]), int(mesh["patch_start"][ZMAX]) + NTOP)
    Sf, magSf, dc, V = a.get("Sf")[fs], a.get("magSf")[fs], a.get("dcNO")[fs], a.get("V")
    n = Sf * (1.0 / magSf)[:, None]                                            # (the unit normal as the kernels form it)
    np.testing.assert_allclose(n, ob.unit_normal(Sf), rtol=4 * EPS, atol=0)
    a.step(); z.step()
    nu = 0.01 if mode == "ico" else 1e-5
    want = ob.pio_rAU_shift(nu * magSf * dc, phi0, n)
    got = V[own] / a.get("rAU")[own] - V[own] / z.get("rAU")[own]
    scale = V[own] / z.get("rAU")[own]
    err = np.abs(got - want)[mask0] / scale[mask0]
    print(f"{mode}: V/rAU shift, max |device - restatement| / (V / rAU_zg) = {err.max():.3e} (bound {64 * EPS:.3e}); shift / scale = {(want / scale)[mask0].min():.3e} .. {(want / scale)[mask0].max():.3e}")
    assert (want[mask0] > 1e-3 * scale[mask0]).all()                            # (the shift is no rounding matter)
    assert err.max() <= 64 * EPS
    np.testing.assert_array_equal(got[~mask0], 0.0)                            # an outflow face is a zeroGradient face
    # the boundary value as the step left it: the mask of the corrector's flux, U after it
    m1 = a.get("U_open_inflow")[top].astype(bool)
    np.testing.assert_array_equal(m1, a.get("phi")[fs] < 0)
    assert m1.any() and (~m1).any()
    U1, ub = a.get("U").reshape(-1, 3)[own], a.get("U_boundary")[top]
    dev = np.abs(ub - ob.pio_value(n, U1)).max(axis=1)[m1] / np.abs(U1).max(axis=1)[m1]
    print(f"{mode}: U_boundary on inflow faces, max |device - n (n . U_P)| / |U_P| = {dev.max():.3e} (bound {8 * EPS:.3e})")
    assert dev.max() <= 8 * EPS
    np.testing.assert_array_equal(ub[~m1], U1[~m1])
    a.close(); z.close()


# ---- 5. plug flow ------------------------------------------------------------------------------------------------------------------------------------------------------
def plug_run(product, mode, u_top, w):
    mesh = block(tilted=False)
    kw = dict(solver=1) if mode == "pimple" else {}
    s = product.LduSolver(mesh, 2e-3, 0.01 if mode == "ico" else 1e-5, [2, 2, 2, 2, 1, u_top], [(0, 0, 0)] * 5 + [(0, 0, -w)], [0, 0, 0, 0, 1, 0], **kw, **SOLVE)
    U0 = np.tile([0.0, 0.0, -w], (mesh["n_cells"], 1))
    s.set("U", U0)
    for _ in range(20):
        s.step()
    dev = np.abs(s.get("U").reshape(-1, 3) - U0).max()
    top, _ = top_faces(mesh)
    mask = s.get("U_open_inflow")[top] if u_top >= IO else None
    s.close()
    return dev, mask


@pytest.mark.parametrize("ucode", [IO, PIO])
@pytest.mark.parametrize("mode", ["ico", "pimple"])
def test_plug_flow_stays_plug_flow(product, mode, ucode):
    """U = (0 0 -w) entering through the open top between slip sides and leaving through a zeroGradient bottom with fixed p is an exact discrete solution, as it is
    with the top fixedValue (0 0 -w): after 20 steps max |U - U0| is within 10 times the larger of that run's deviation and 1e-14 w -- both are rounding noise of
    different operation orders, a wrong coefficient is orders above"""
    w = 0.5
    ref, _ = plug_run(product, mode, 0, w)
    dev, mask = plug_run(product, mode, ucode, w)
    print(f"{mode}, code {ucode}: max |U - U0| = {dev:.3e} (fixedValue top: {ref:.3e}; bound {10 * max(ref, 1e-14 * w):.3e})")
    assert mask.all()                                                          # the whole top is an inflow
    assert dev <= 10 * max(ref, 1e-14 * w)


# ---- 6. a sign that changes --------------------------------------------------------------------------------------------------------------------------------------------
SIGN_A, SIGN_DT, SIGN_NU = 40.0, 2e-3, 1e-5      # chosen on the CPU oracle with a zeroGradient top (DESIGN_HISTORY.md "Open boundaries"): both signs hold > 25 % from step 10 on, the pattern moves


SIGN_VIN = (0.002, 0.0, -0.01)                   # inletOutlet's inlet value: of the size of the flow the force drives


def sign_source(mesh):
    """uSource_z = A sin(2 pi x / L) in the two top cell layers (the lattice numbering: layer = cell // (NX NY)), antisymmetric about the mid-plane"""
    nc = mesh["n_cells"]
    i = np.arange(nc) % NX
    src = np.zeros((nc, 3))
    src[:, 2] = SIGN_A * np.sin(2 * np.pi * (i + 0.5) / NX)
    src[np.arange(nc) // (NX * NY) < NZ - 2] = 0.0
    return src


def sign_run(product, ucode):
    mesh = block()
    s = product.LduSolver(mesh, SIGN_DT, SIGN_NU, [0, 0, 0, 0, 0, ucode], [(0, 0, 0)] * 5 + [SIGN_VIN], [0, 0, 0, 0, 0, 1], solver=1, n_non_orth=1, **SOLVE)
    top, own = top_faces(mesh)
    fs = slice(int(mesh["patch_start"][ZMAX]), int(mesh["patch_start"][ZMAX]) + NTOP)
    n = s.get("Sf")[fs] * (1.0 / s.get("magSf")[fs])[:, None]
    src = sign_source(mesh)
    masks, fields = [], None
    for step in range(30):
        s.step(src if step == 0 else None)
        phi, m = s.get("phi"), s.get("U_open_inflow")
        mt = m[top].astype(bool)
        np.testing.assert_array_equal(mt, phi[fs] < 0, err_msg="step %d" % step)
        assert m.sum() == mt.sum()
        U, ub = s.get("U").reshape(-1, 3)[own], s.get("U_boundary")[top]
        if ucode == PIO:
            if mt.any():
                assert (np.abs(ub - ob.pio_value(n, U)).max(axis=1)[mt] <= 8 * EPS * np.abs(U).max(axis=1)[mt]).all(), step
        else:
            np.testing.assert_array_equal(ub[mt], np.tile(SIGN_VIN, (int(mt.sum()), 1)))
        np.testing.assert_array_equal(ub[~mt], U[~mt])
        st = s.open_boundary_stats()
        cnt, fin, fout = ob.stats(phi[fs], np.ones(NTOP, bool))
        tol = NTOP * EPS * np.abs(phi[fs]).sum()
        assert st["inflow_faces"] == cnt and abs(st["inflow_flux"] - fin) <= tol and abs(st["outflow_flux"] - fout) <= tol, (step, st, cnt, fin, fout)
        masks.append(mt.copy())
    fields = {nm: s.get(nm) for nm in ("U", "p", "phi", "U_open_inflow")}
    fields["stats"] = s.open_boundary_stats()
    s.close()
    return masks, fields


@pytest.mark.parametrize("ucode", [IO, PIO])
def test_a_flux_sign_that_changes(product, ucode):
    """fluid at rest under a tilted open top with fixed p, walls elsewhere, driven by a body force in the two top cell layers that blows in on one half and out on the
    other: after every one of 30 steps the mask is (phi < 0) exactly, U_boundary is the condition's value on the inflow faces and the cell's on the others, the stats
    are numpy's sums over phi (the count exactly, the fluxes within 270 eps sum |phi|); both signs hold a quarter of the faces from step 10 on and the pattern moves;
    the run repeated gives the same bits"""
    masks, f1 = sign_run(product, ucode)
    frac = [m.mean() for m in masks]
    print("inflow fraction per step:", " ".join("%.3f" % x for x in frac), "| faces that differ between step 10 and step 30:", int((masks[9] != masks[29]).sum()))
    assert all(0.25 <= x <= 0.75 for x in frac[9:]), frac
    assert (masks[9] != masks[29]).any()
    _, f2 = sign_run(product, ucode)
    for nm in ("U", "p", "phi", "U_open_inflow"):
        np.testing.assert_array_equal(f1[nm], f2[nm], err_msg=nm)
    assert f1["stats"] == f2["stats"]


# ---- 7. off is off -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_off_is_off(product):
    """no open code: no mask (the field and the stats are refused by name), and the "open_boundary" clock counts no launch"""
    mesh = block()
    s = product.LduSolver(mesh, 1e-3, 0.01, [0, 0, 0, 0, 0, 1], [(0, 0, 0)] * 4 + [(0, 0, 0.1), (0, 0, 0)], [0, 0, 0, 0, 0, 1], **SOLVE)
    s.enable_kernel_timing(True)
    for _ in range(2):
        s.step()
    assert s.kernel_timing("open_boundary") == (0.0, 0)
    with pytest.raises(product.FoamYadeError, match="U_open_inflow"):
        s.get("U_open_inflow")
    with pytest.raises(product.FoamYadeError, match="fy_ldu_solver_get_open_boundary_stats"):
        s.open_boundary_stats()
    s.close()
    o = product.LduSolver(mesh, 1e-3, 0.01, [0, 0, 0, 0, 0, IO], [(0, 0, 0)] * 4 + [(0, 0, 0.1), (0, 0, 0)], [0, 0, 0, 0, 0, 1], n_correctors=2, **SOLVE)
    o.enable_kernel_timing(True)
    for _ in range(2):
        o.step()
    assert o.kernel_timing("open_boundary")[1] == 2 * 2 * (1 + 2)              # per step: the start and each of two correctors, a kernel and the fold each
    o.close()


# ---- codes ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_codes_are_refused_where_they_do_not_belong(product):
    """the block solver refuses the new velocity codes as unknown; nut refuses inletOutlet; an unknown code's refusal lists the new words.  On the device although
    nothing is computed: fy_solver_create and fy_ldu_solver_create ask for a HIP device before they look at the codes (the library has no CPU path), so without one
    the refusal would be FY_ERR_NO_DEVICE's, not the one under test"""
    for code in (IO, PIO):
        u_bc = [0, 0, 0, 0, 0, code]
        with pytest.raises(product.FoamYadeError, match="fy_solver_create: unknown velocity boundary type %d on side 5" % code):
            product.Solver(product.make_case(0, 8, 8, 8, 0.0125, 1e-3, 0.01, u_bc=u_bc))
    mesh = block()
    with pytest.raises(product.FoamYadeError, match="nut patch type 4"):
        product.LduSolver(mesh, 1e-3, 1e-5, [0] * 6, [(0, 0, 0)] * 6, [0] * 5 + [1], solver=1, nut_bc=[0] * 5 + [S_IO], nut_val=[0] * 6, **TURB)
    with pytest.raises(product.FoamYadeError, match="velocity patch type 7 .*inletOutlet, pressureInletOutletVelocity"):
        product.LduSolver(mesh, 1e-3, 0.01, [0] * 5 + [7], [(0, 0, 0)] * 6, [0] * 5 + [1])
    assert (product.FY_BC_U_INLET_OUTLET, product.FY_BC_U_PRESSURE_INLET_OUTLET, product.FY_BC_NUT_INLET_OUTLET, product.FY_BC_T_INLET_OUTLET) == (3, 4, 4, 2)
