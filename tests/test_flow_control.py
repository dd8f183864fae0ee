"""Flow-rate control on the general-mesh solver (fy_flow_control_desc: the role of OpenFOAM's meanVelocityForce) on the GPU, against the long-double restatement
flow_control_ref.py.  Meshes of a few hundred cells: A = one ragged block of lanes, B = two blocks with a ragged tail (the fold crosses blocks), C = B's lattice
displaced periodically (non-orthogonal), x and z cyclic."""
import hashlib

import numpy as np
import pytest

import flow_control_ref as fr
import poly_meshes as pm

pytestmark = pytest.mark.gpu

LD = fr.LD
BOX = (0.1, 0.06, 0.1)
UBAR = (0.1, 0.0, 0.0)
TIGHT = dict(p_tol=1e-11, p_rel_tol=0.0, p_final_tol=1e-11, u_tol=1e-11, p_max_iter=5000, u_max_iter=5000)


def mesh_of(which, box=BOX):
    if which == "A":
        return pm.make_cyclic(pm.hex_block(4, 6, 4, box), [(0, 1)]), 0
    if which == "B":
        return pm.make_cyclic(pm.hex_block(7, 6, 7, box), [(0, 1)]), 0
    return pm.make_cyclic(pm.hex_block(7, 6, 7, box, pm.wavy_periodic(0.002, box)), [(0, 1), (4, 5)]), 1


def make(product, which, pimple, flow=None, dt=1e-3, nu=1e-4, box=BOX, mesh=None, **kw):
    """x cyclic, y walls (noSlip), z symmetry (A, B) or cyclic (C)"""
    m, non_orth = mesh_of(which, box) if mesh is None else mesh
    ctl = dict(TIGHT); ctl.update(kw)
    s = product.LduSolver(m, dt, nu, [1, 1, 0, 0, 2, 2], [(0, 0, 0)] * 6, [0] * 6, solver=1 if pimple else 0, n_non_orth=non_orth, flow_control=flow, **ctl)
    return s, m


def shear_flow(s, amp=0.05, box=BOX):
    """a start that moves: a parabola in y along x with a ripple, so that particles at rest feel a drag"""
    C = s.get("C")
    y = C[:, 1] / box[1]
    U = np.zeros((s.n_cells, 3))
    U[:, 0] = amp * 6 * y * (1 - y) * (1 + 0.1 * np.sin(2 * np.pi * C[:, 0] / box[0]))
    s.set("U", U)


def cloud(n, seed, box=BOX, radius=0.002, sigma=None):
    """particles at rest, spread over the box; sigma: Gaussian in y about the mid-plane (a band of lowered void fraction) instead of uniform"""
    rs = np.random.RandomState(seed)
    rec = np.zeros((n, 10))
    rec[:, 0:3] = (0.15 + 0.7 * rs.rand(n, 3)) * np.array(box)
    if sigma is not None:
        rec[:, 1] = np.clip(0.5 + sigma * rs.standard_normal(n), 0.2, 0.8) * box[1]
    rec[:, 9] = radius
    return rec


def bulk_tol(U, V, d, w=None):
    """the bulk velocity of a field in long double and the bound 8 n 2^-53 S |flowDir . U_i| (w_i) V_i / V on what the device's rounding may have left of it"""
    b, scale = fr.bulk(U, V, d, w)
    return b, 8 * len(V) * fr.U53 * float(scale)


# ------------------------------------------------------------------------------------------------ 1. the bulk velocity is held
@pytest.mark.parametrize("pimple", [False, True])
@pytest.mark.parametrize("which", ["A", "B", "C"])
def test_bulk_velocity_is_held(product, which, pimple):
    ubar = (0.06, 0.0, 0.08) if which == "C" else UBAR                  # (C is periodic in x and z: a direction with two components)
    d, mag = fr.direction(ubar)
    s, _ = make(product, which, pimple, product.flow_control_desc(ubar))
    V = s.get("V")
    for step in range(5):
        s.step()
        b, tol = bulk_tol(s.get("U"), V, d)
        print(f"{which} pimple={pimple} step {step}: bulk - |Ubar| = {float(b - LD(mag)):.3e}, tol {tol:.3e}")
        assert abs(b - LD(mag)) <= tol, (step, float(b), mag, tol)
    assert s.flow_control()["corrections"] == 5 * 2
    s.close()
    s, _ = make(product, which, pimple, product.flow_control_desc(ubar, relaxation=0.5))
    s.step()
    f = s.flow_control()
    b, tol = bulk_tol(s.get("U"), V, d)
    want = LD(f["ubar"]) + LD(0.5) * (LD(mag) - LD(f["ubar"]))
    print(f"{which} pimple={pimple} r=0.5: bulk - want = {float(b - want):.3e}, tol {tol:.3e}")
    assert abs(b - want) <= tol
    s.close()


# ------------------------------------------------------------------------------------------------ 2. the correction is the formula
@pytest.mark.parametrize("pimple", [False, True])
@pytest.mark.parametrize("which", ["B", "C"])
def test_correction_is_the_formula(product, which, pimple):
    G0, r = 0.5, 0.7
    d, mag = fr.direction(UBAR)
    s1, m = make(product, which, pimple, product.flow_control_desc(UBAR, relaxation=r, gradient0=G0), n_correctors=1)
    s2, _ = make(product, which, pimple, None, n_correctors=1)
    rec = cloud(20, 7)
    for s in (s1, s2):
        shear_flow(s)
        s.hold_sources(True)
        s.set_particles(rec)
    s2.set("uSource", np.tile(np.asarray(d) * G0, (s2.n_cells, 1)))
    s1.step(); s2.step()
    assert np.abs(s2.get("uSourceCoupling")).max() > 0                   # the particles did leave a source
    assert np.array_equal(s1.get("uSource"), np.zeros(3 * s1.n_cells))  # reading "uSource" still returns what was written: nothing
    V, U2, rAU2 = s2.get("V"), s2.get("U"), s2.get("rAU")
    assert np.array_equal(s1.get("rAU"), rAU2)
    ref = fr.correction(U2, rAU2, V, UBAR, r)
    dG = float(ref["dGradP"])
    rel = 16 * s2.n_cells * fr.U53 * ref["kappa"]
    tolU = np.abs(rAU2).max() * abs(dG) * rel + 2 * np.spacing(np.abs(np.asarray(ref["U"], float)))
    diff = np.abs(np.asarray(s1.get("U").reshape(-1, 3), LD) - ref["U"]).astype(float)
    print(f"{which} pimple={pimple}: max |U1 - expected| = {diff.max():.3e}, smallest tolerance {tolU.min():.3e}, dGradP {dG:.6e}, kappa {ref['kappa']:.3f}")
    assert np.abs(U2 - s1.get("U")).max() > 1e3 * tolU.max()             # (the correction is not a no-op)
    assert np.all(diff <= tolU), (diff.max(), tolU.min())
    f = s1.flow_control()
    for key, want in (("ubar", ref["ubar"]), ("rAU_ave", ref["rAU_ave"]), ("dGradP", ref["dGradP"]), ("gradient", LD(G0) + ref["dGradP"])):
        scale = abs(float(want)) if key != "gradient" else abs(G0) + abs(dG)
        print(f"    {key}: device {f[key]!r}, reference {float(want)!r}")
        assert abs(LD(f[key]) - want) <= rel * scale + 2 * np.spacing(scale), key
    assert f["corrections"] == 1
    s1.close(); s2.close()


# ------------------------------------------------------------------------------------------------ 3. two correctors and two outer iterations
def test_two_correctors_two_outer_iterations(product):
    """corrections grow by 4 per step.  The gradient is gradP0 + dGradP with gradP0 += (the last dGradP) at each assembly.  After a step the getter shows the dGradP of
    the step's LAST correction only, so the replay needs the one the first outer iteration ended with: in step 1 a twin with ONE outer iteration (the same first
    iteration, bit for bit: no relaxation factors, p_final_tol = p_tol) supplies it.  With one outer iteration the getter's history replays exactly over 3 steps"""
    d, mag = fr.direction(UBAR)
    G0 = 0.25
    fl = lambda: product.flow_control_desc(UBAR, relaxation=0.7, gradient0=G0)
    s, _ = make(product, "B", True, fl(), n_outer_correctors=2, n_correctors=2)
    twin, _ = make(product, "B", True, fl(), n_outer_correctors=1, n_correctors=2)
    for q in (s, twin):
        shear_flow(q)
        q.hold_sources(True)                                              # (the step's momentum source stays readable after it)
    twin.step()
    mid = twin.flow_control()
    assert mid["corrections"] == 2
    st = fr.State(G0)
    for step in range(3):
        s.step()
        f = s.flow_control()
        assert f["corrections"] == 4 * (step + 1)
        if step == 0:
            st.assemble(); st.correct(mid["dGradP"])                      # outer iteration 1 (its first corrector's dGradP was overwritten by its second's)
            st.assemble(); st.correct(f["dGradP"])                        # outer iteration 2
            assert st.gradP0 == G0 + mid["dGradP"] and f["gradient"] == st.gradient
            # ... and the second assembly's momentum source carried that gradP0: without particles pimpleFoamYade's source field is the effective external source
            src = s.get("uSourceCoupling").reshape(-1, 3)
            assert np.array_equal(src[:, 0], np.full(s.n_cells, st.gradP0)) and not src[:, 1:].any()
    s.close(); twin.close()
    one, _ = make(product, "B", True, fl(), n_outer_correctors=1, n_correctors=2)
    shear_flow(one)
    st = fr.State(G0)
    for step in range(3):
        one.step()
        f = one.flow_control()
        st.assemble(); st.correct(f["dGradP"])
        assert f["corrections"] == 2 * (step + 1) and f["gradient"] == st.gradient, (step, f, st.gradP0)
    assert st.gradP0 != G0
    one.close()


# ------------------------------------------------------------------------------------------------ 4. known answer
def test_known_answer_plane_channel(product):
    """uniform hexahedra between two no-slip walls, periodic in x and z, icoFoamYade, r = 1: once the slowest viscous mode has decayed below 1e-10 the reported gradient
    is the discrete closed form |Ubar| / c (flow_control_ref.channel_gradient) to 100 max(u_tol, p_tol, decay) relative.
    Observed on an MI355X: gradient 1.1368421052631579 against the closed form 1.1368421052631579 after 234 steps -- relative distance 0 (bound 9.3e-9)."""
    H, nu, dt, tol = 1.0, 1.0, 0.01, 1e-11
    box = (1.0, H, 1.0)
    mesh = pm.make_cyclic(pm.hex_block(4, 6, 4, box), [(0, 1), (4, 5)])
    s, _ = make(product, "A", False, product.flow_control_desc(UBAR), dt=dt, nu=nu, box=box, mesh=(mesh, 0), p_tol=tol, p_final_tol=tol, u_tol=tol)
    steps, decay = fr.viscous_steps(H, nu, dt)
    assert steps <= 300
    for _ in range(steps):
        s.step()
    want = float(fr.channel_gradient(6, H, nu, UBAR[0]))
    got = s.flow_control()["gradient"]
    bound = 100 * max(tol, decay)
    print(f"known answer: gradient {got!r}, closed form {want!r}, relative distance {abs(got - want) / want:.3e}, bound {bound:.3e}, {steps} steps")
    assert abs(got - want) <= bound * want
    u = s.get("U").reshape(-1, 3)[:, 0].reshape(4, 6, 4)[0, :, 0]            # (lattice numbering: i + nx (j + ny k) -> [k][j][i])
    prof = np.asarray(fr.channel_profile(6, H, nu, want), float)
    assert np.allclose(u, prof, rtol=1e-6)
    s.close()


# ------------------------------------------------------------------------------------------------ 5. superficial
def test_superficial_weighs_with_the_void_fraction(product):
    d, mag = fr.direction(UBAR)
    rec = cloud(60, 11, radius=0.0035, sigma=0.1)
    out = {}
    for sup in (True, False):
        s, _ = make(product, "B", True, product.flow_control_desc(UBAR, superficial=sup))
        s.hold_sources(True)                                              # (alpha stays readable after the step)
        shear_flow(s)
        s.set_particles(rec)
        V = s.get("V")
        for step in range(3):
            s.step()
        alpha, U = s.get("alpha"), s.get("U")
        assert alpha.min() < 0.99 and alpha.max() <= 1.0
        (bw, tw), (bp, tp) = bulk_tol(U, V, d, alpha), bulk_tol(U, V, d)
        print(f"superficial={sup}: weighted - |Ubar| = {float(bw - LD(mag)):.3e} (tol {tw:.3e}), plain - |Ubar| = {float(bp - LD(mag)):.3e} (tol {tp:.3e}), min alpha {alpha.min():.4f}")
        out[sup] = (abs(bw - LD(mag)), tw, abs(bp - LD(mag)), tp)
        s.close()
    assert out[True][0] <= out[True][1] and out[True][2] > 1e3 * out[True][3]
    assert out[False][2] <= out[False][3] and out[False][0] > 1e3 * out[False][1]


# ------------------------------------------------------------------------------------------------ 6. off is off
@pytest.mark.parametrize("pimple", [False, True])
def test_off_is_off(product, pimple):
    off, _ = make(product, "B", pimple)
    off.enable_kernel_timing(True)
    with pytest.raises(product.FoamYadeError, match="unknown kernel clock 'flow_control'"):
        off.kernel_timing("flow_control")
    off.enable_kernel_timing(False)
    with pytest.raises(product.FoamYadeError) as e:
        off.flow_control()
    assert "error 1" in str(e.value) and "flow control is off" in str(e.value)
    idle, _ = make(product, "B", pimple, product.flow_control_desc(UBAR, relaxation=0.0, gradient0=0.0))
    rec = cloud(20, 5)
    for s in (off, idle):
        shear_flow(s)
        s.set_particles(rec)
    for _ in range(3):
        off.step(); idle.step()
    for nm in ("U", "p", "phi"):
        assert np.array_equal(off.get(nm), idle.get(nm)), nm
    assert np.abs(off.get("U")).max() > 0 and idle.flow_control()["gradient"] == 0.0
    off.close(); idle.close()
    # switching off mid-run: the next step is that of a solver whose external source is what "uSource" holds, no more
    x = np.zeros((off.n_cells, 3)); x[:, 1] = 0.01
    a, _ = make(product, "B", pimple, product.flow_control_desc(UBAR, relaxation=0.7, gradient0=0.5))
    b, _ = make(product, "B", pimple, product.flow_control_desc(UBAR, relaxation=0.7, gradient0=0.5))
    for s in (a, b):
        shear_flow(s)
        s.set("uSource", x)
        s.step(); s.step()
    assert np.array_equal(a.get("U"), b.get("U"))
    a.set_flow_control(None)
    b.set_flow_control(product.flow_control_desc(UBAR, relaxation=0.0, gradient0=0.0))      # (equal to off, by the first half of this test)
    a.step(); b.step()
    for nm in ("U", "p", "phi", "uSource"):
        assert np.array_equal(a.get(nm), b.get(nm)), nm
    assert np.array_equal(a.get("uSource").reshape(-1, 3), x)
    with pytest.raises(product.FoamYadeError, match="flow control is off"):
        a.flow_control()
    a.set_flow_control(product.flow_control_desc(UBAR, gradient0=0.125))                       # a new call restarts the state from gradient0
    assert a.flow_control() == dict(gradient=0.125, ubar=0.0, rAU_ave=0.0, dGradP=0.0, corrections=0)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 7. the same bits from run to run
def test_same_bits_run_to_run(product):
    """two fresh solvers, 5 steps, with particles (four, far apart: no cell takes more than two of the scatter's atomic additions, whose order is then immaterial)"""
    rec = np.zeros((4, 10))
    rec[:, 0:3] = np.array([[0.2, 0.3, 0.2], [0.8, 0.3, 0.2], [0.2, 0.7, 0.8], [0.8, 0.7, 0.8]]) * np.array(BOX)
    rec[:, 9] = 0.002
    digests = []
    for _ in range(2):
        s, _ = make(product, "B", True, product.flow_control_desc(UBAR, relaxation=0.9, gradient0=0.1))
        shear_flow(s)
        s.set_particles(rec)
        h = hashlib.sha256()
        for _ in range(5):
            s.step()
            f = s.flow_control()
            h.update(s.get("U").tobytes()); h.update(s.get("p").tobytes())
            h.update(np.array([f["gradient"], f["ubar"], f["rAU_ave"], f["dGradP"], f["corrections"]], np.float64).tobytes())
        digests.append(h.hexdigest())
        s.close()
    assert digests[0] == digests[1]


# ------------------------------------------------------------------------------------------------ 8. the launch budget
@pytest.mark.parametrize("pimple,n_outer,n_corr", [(False, 1, 2), (True, 2, 2), (True, 1, 1)])
def test_launch_budget(product, pimple, n_outer, n_corr):
    kw = dict(n_outer_correctors=n_outer) if pimple else {}
    s, _ = make(product, "B", pimple, product.flow_control_desc(UBAR), n_correctors=n_corr, **kw)
    s.enable_kernel_timing(True)
    steps = 2
    for _ in range(steps):
        s.step()
    ms, launches = s.kernel_timing("flow_control")
    assemblies, correctors = n_outer, n_outer * n_corr
    print(f"pimple={pimple} {n_outer} x {n_corr}: {launches / steps:g} launches per step, {1e3 * ms / launches:.2f} us per launch")
    assert 0 < launches <= steps * (assemblies + 3 * correctors)
    assert s.flow_control()["corrections"] == steps * correctors
    s.close()


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals(product):
    fd = product.flow_control_desc
    for pimple, desc, word in ((False, fd((0, 0, 0)), "ubar"), (True, fd((0, 0, 0)), "ubar"), (False, fd((float("nan"), 0, 0)), "ubar"), (True, fd(UBAR, relaxation=1.5), "relaxation"),
                               (False, fd(UBAR, relaxation=-0.1), "relaxation"), (False, fd(UBAR, superficial=True), "superficial")):
        with pytest.raises(product.FoamYadeError) as e:
            make(product, "A", pimple, desc)
        assert "error 1" in str(e.value) and "fy_ldu_solver_create" in str(e.value) and "flow_control." + word in str(e.value), str(e.value)
    s, _ = make(product, "A", False)
    for desc, word in ((fd((0, 0, 0)), "ubar"), (fd(UBAR, relaxation=1.5), "relaxation"), (fd(UBAR, superficial=True), "superficial")):
        with pytest.raises(product.FoamYadeError) as e:
            s.set_flow_control(desc)
        assert "error 1" in str(e.value) and "fy_ldu_solver_set_flow_control" in str(e.value) and "flow_control." + word in str(e.value), str(e.value)
    with pytest.raises(product.FoamYadeError) as e:
        s.flow_control()
    assert "error 1" in str(e.value) and "fy_ldu_solver_get_flow_control" in str(e.value)
    s.step()                                                              # a refused descriptor left the solver as it was
    s.close()
    p, _ = make(product, "A", True, fd(UBAR, superficial=True))           # pimpleFoamYade takes it
    p.close()
