"""The thermal loop on the device (fy_thermal_desc.particle_cp, beta, T_ref): particle temperatures the library integrates, and Boussinesq buoyancy -- against closed
forms and against tests/thermal_loop_ref.py, the numpy restatement written from the formulas (itself held to closed forms in tests/test_thermal_loop_ref.py).  Bars: 1e-10 of
the compared field's range against the restatement (tests/test_heat_transfer.py's BAR), 1e-12 against a closed form, bit for bit where the statement is about bits."""
import numpy as np
import pytest

import heat_transfer_ref as ht
import thermal_loop_ref as tl
from test_heat_transfer import BAR, BOX, WATER, assert_field, bed_case, bed_cloud, cloud, one_per_cell, thermal

pytestmark = pytest.mark.gpu

RHO_P = 2650.0                                           # make_case's rho_p
# The moving bed's particles (r ~ 2 mm in water, dt 2e-4) have dt hA / (m c_pp) ~ 0.07 / c_pp: a physical c_pp leaves r_p ~ 1e-4, at which Tp moves by 1e-4 of the
# temperature difference per step and a comparison at 1e-10 of Tp's range would hardly see the update.  The comparisons with the restatement use c_pp = 0.05 J/kg/K:
# r_p of order one, so that hA' differs from hA by its half and Tp crosses a good part of the difference in a step.
CPP_BED = 0.05


# ---- 1. two bodies, point mode --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r_p", [0.1, 5.0])
def test_two_body_closed_form_in_point_mode(product, r_p):
    """one particle at rest in every cell centre, fluid at 0, particles at 50: every cell and its particle are the closed recurrence.  At r_p = 5 an explicit update of Tp
    would overshoot the fluid temperature and oscillate; the pair's backward Euler step approaches the equilibrium monotonically"""
    n, dx, dt = 4, 0.01, 0.02
    nu, rho, cp, kappa, Tp0 = 1e-2, 1.0, 1000.0, 0.6, 50.0
    N = n ** 3
    c = np.arange(N)
    rec = np.zeros((N, 10))
    rec[:, 0:3] = (np.stack([c % n, (c // n) % n, c // (n * n)], axis=1) + 0.5) * dx
    rec[:, 9] = 0.1 * dx
    hA = float(ht.nusselt(ht.RANZ_MARSHALL, 1.0, ht.SMALL, ht.prandtl(nu, rho, cp, kappa)) * kappa * np.pi * 0.2 * dx)
    vol_p = (4.0 / 3.0) * np.pi * (0.1 * dx) ** 3
    cpp = dt * hA / (r_p * RHO_P * vol_p)
    mc = RHO_P * vol_p * cpp
    assert abs(dt * hA / mc / r_p - 1.0) < 1e-12
    Cf = rho * cp * dx ** 3
    th = thermal(product, 200, cp=cp, kappa=kappa, T_initial=0.0, particle_temperature=Tp0, particle_cp=cpp)
    s = product.Solver(product.make_case(0, n, n, n, dx, dt, nu, rho_f=rho, thermal=th))
    Ts, Tps, qs = tl.two_body(0.0, Tp0, hA, dt, Cf, mc, 6)
    total, prev = mc * Tp0, Tp0
    for step in range(6):
        s.set_particles(rec)
        s.step()
        T, Tp, q = s.get("T"), s.particle_temperatures(), s.particle_heat()
        eT, eTp, eq = np.abs(T - Ts[step]).max(), np.abs(Tp - Tps[step]).max(), np.abs(q - qs[step]).max()
        heat = Cf * T + mc * Tp
        print(f"r_p {r_p} step {step}: |T - cf| {eT:.3e}, |Tp - cf| {eTp:.3e} of {Tp0}; |q - cf| {eq:.3e} of {hA * Tp0:.3e}; heat content off by {np.abs(heat / total - 1).max():.3e}")
        assert eT <= 1e-12 * Tp0 and eTp <= 1e-12 * Tp0 and eq <= 1e-12 * hA * Tp0
        assert np.abs(heat - total).max() <= 1e-13 * total
        assert (Tp < prev).all() and (Tp > T).all()          # monotone: down towards the equilibrium, never past the fluid
        prev = Tp
    assert np.abs(s.get("U")).max() == 0.0
    s.close()


# ---- 2. Gaussian passes against the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", ["RanzMarshall", "Gunn"])
def test_gaussian_passes_match_the_restatement(product, law):
    lawc = product.NUSSELT_GUNN if law == "Gunn" else product.NUSSELT_RANZ_MARSHALL
    nu, rho = 1e-5, 1000.0
    s = product.Solver(bed_case(product, thermal(product, 40, T_initial=300.0, nusselt_law=lawc, particle_temperature=111.0, particle_cp=CPP_BED, **WATER)))
    Nc = BOX[0] * BOX[1] * BOX[2]
    rs = np.random.RandomState(19)
    s.set("U", 0.05 * rs.standard_normal((Nc, 3)))
    s.set("T", 300.0 + 50.0 * rs.random_sample(Nc))
    rec = bed_cloud(3000, outside=5)
    assert np.ptp(rec[:, 9]) > 0
    mc = tl.heat_capacity(rec, RHO_P, CPP_BED)
    Pr = ht.prandtl(nu, rho, WATER["cp"], WATER["kappa"])
    s.hold_sources(True)
    s.set_particles(rec)
    s.set_particle_temperatures(280.0 + 90.0 * rs.random_sample(rec.shape[0]))
    for step in range(3):
        s.set_particles(rec)
        Tp = s.particle_temperatures()
        U = s.get("U").reshape(Nc, 3)
        s.step()
        dt = s.stats()["delta_t"]
        k, ids, w, chain = s.stencils()
        assert (k[:5] == 0).all() and (k[5:] > 0).mean() > 0.9
        hAp, Sp, Su = tl.pass_a(lawc, rec, ids, w, U, s.get("alpha"), Tp, nu, WATER["kappa"], Pr, Nc, dt, mc)
        q_ref, Tp_ref = tl.pass_b(hAp, ids, w, s.get("T"), Tp, dt, mc)
        r_p = dt * hAp / (mc - dt * hAp)                       # hA' = hA / (1 + r_p)  =>  r_p = dt hA' / (m c - dt hA')
        assert 0.3 < np.median(r_p[k > 0]) < 30.0, np.median(r_p[k > 0])
        q, Tp_new = s.particle_heat(), s.particle_temperatures()
        assert_field(s.get("heatSp"), Sp, f"{law} heatSp, step {step}")
        assert_field(s.get("heatSu"), Su, f"{law} heatSu, step {step}")
        assert_field(q, q_ref, f"{law} q, step {step}")
        assert_field(Tp_new, Tp_ref, f"{law} Tp, step {step}")
        assert (Tp_new[:5] == Tp[:5]).all() and (q[:5] == 0.0).all()      # nobody located them: bit for bit
        assert np.abs(Tp_new - Tp)[k > 0].min() > 0
    s.close()


# ---- 3. energy balance ---------------------------------------------------------------------------------------------------------------------------------------
def test_energy_balance_in_a_closed_box_at_rest(product):
    """zeroGradient walls, g = 0, particles and fluid at rest: what the fluid's heat content gains the particles' loses"""
    nx, ny, nz, dx, dt = 8, 6, 5, 0.01, 0.05
    rho, cp, cpp = 1000.0, 4180.0, 800.0
    th = thermal(product, 100, T_initial=0.0, particle_temperature=50.0, nusselt_law=product.NUSSELT_GUNN, particle_cp=cpp, **WATER)
    s = product.Solver(product.make_case(1, nx, ny, nz, dx, dt, 1e-6, rho_f=rho, p_bc=[2] * 6, thermal=th))
    rec = cloud(300, (0.01, 0.01, 0.01), (0.07, 0.05, 0.04), 0.002, 23, speed=0.0)
    mc = tl.heat_capacity(rec, RHO_P, cpp)
    s.hold_sources(True)
    Told, Tpold = s.get("T"), np.full(300, 50.0)
    for step in range(3):
        s.set_particles(rec)
        s.step()
        T, alpha, q, Tp = s.get("T"), s.get("alpha"), s.particle_heat(), s.particle_temperatures()
        fluid, part, exchanged = rho * cp * (alpha * dx ** 3 * (T - Told)).sum(), (mc * (Tp - Tpold)).sum(), abs(dt * q.sum())
        print(f"step {step}: fluid gains {fluid:.12e} J, particles gain {part:.12e} J, exchanged {exchanged:.12e} J, imbalance {abs(fluid + part) / exchanged:.2e}")
        assert abs(fluid + part) <= BAR * exchanged
        assert fluid > 0 > part and alpha.min() < 1.0
        Told, Tpold = T, Tp
    assert Tp.max() < 50.0
    s.close()


# ---- 4. equilibrium is a fixed point ---------------------------------------------------------------------------------------------------------------------------
def test_equilibrium_is_a_fixed_point_in_a_moving_bed(product):
    T0 = 300.0
    s = product.Solver(bed_case(product, thermal(product, 60, T_initial=T0, particle_temperature=T0, nusselt_law=product.NUSSELT_GUNN, particle_cp=CPP_BED, **WATER)))
    rec = bed_cloud()
    for step in range(4):
        s.set_particles(rec)
        s.step()
        T, Tp = s.get("T"), s.particle_temperatures()
        print(f"step {step}: max |T / T0 - 1| = {np.abs(T / T0 - 1).max():.3e}, max |Tp / T0 - 1| = {np.abs(Tp / T0 - 1).max():.3e}")
        assert np.abs(T - T0).max() <= 1e-12 * T0 and np.abs(Tp - T0).max() <= 1e-12 * T0
    assert np.abs(s.get("U")).max() > 0 and s.get("heatSp").max() > 0
    s.close()


# ---- 5. adjustable time step ------------------------------------------------------------------------------------------------------------------------------------
def test_the_update_uses_the_steps_own_delta_t(product):
    """adjustTimeStep: the bed starts at rest, so setDeltaT.H stretches deltaT by its factor 1.2 from step to step; the particles' heat content must change by exactly the
    step's own deltaT times what they received.  All particles are hotter than the fluid (one sign, no cancellation in the sums), r_p is of order one (Tp moves by kelvins,
    so Tp' - Tp loses nothing to Tp's own rounding): both sums are then good to ~1e-15"""
    th = thermal(product, 40, T_initial=300.0, particle_temperature=350.0, particle_cp=CPP_BED, **WATER)
    s = product.Solver(bed_case(product, th, adjust_time_step=1, max_co=0.5, max_delta_t=1e-3))
    rec = bed_cloud()
    mc = tl.heat_capacity(rec, RHO_P, CPP_BED)
    dts, Tpold = [], np.full(rec.shape[0], 350.0)
    for step in range(4):
        s.set_particles(rec)
        s.step()
        dt, q, Tp = s.stats()["delta_t"], s.particle_heat(), s.particle_temperatures()
        lhs, rhs = (mc * (Tp - Tpold)).sum(), dt * q.sum()
        print(f"step {step}: deltaT {dt:.6e}, sum m c dTp = {lhs:.15e}, deltaT sum q = {rhs:.15e}, relative difference {abs(lhs / rhs - 1):.2e}")
        assert abs(lhs - rhs) <= 1e-12 * abs(rhs) and rhs < 0
        dts.append(dt); Tpold = Tp
    assert len(set(dts)) == 4 and dts[0] != 2e-4, dts
    s.close()


# ---- 6. who owns Tp --------------------------------------------------------------------------------------------------------------------------------------------
def test_ownership_of_the_particle_temperatures(product):
    import torch
    rec = bed_cloud(200, 7)
    rs = np.random.RandomState(3)
    s = product.Solver(bed_case(product, thermal(product, 40, T_initial=300.0, particle_temperature=222.0, particle_cp=CPP_BED, **WATER)))
    s.set_particles(rec)
    assert (s.particle_temperatures() == 222.0).all() and s.particle_temperature_resets() == 0
    a = 280.0 + 90.0 * rs.random_sample(200)
    s.set_particle_temperatures(a)
    np.testing.assert_array_equal(s.particle_temperatures(), a)
    b = 280.0 + 90.0 * rs.random_sample(200)
    s.set_particle_temperatures(torch.from_numpy(b).to("cuda"))
    np.testing.assert_array_equal(s.particle_temperatures(), b)
    s.step()
    after = s.particle_temperatures()
    k = s.stencils()[0]
    assert (k > 0).all() and (after != b).all()              # integration continued from what was set
    s.set_particles(rec)                                     # the same count: the array stands
    np.testing.assert_array_equal(s.particle_temperatures(), after)
    s.step()
    assert (s.particle_temperatures() != after).all() and s.particle_temperature_resets() == 0
    s.set_particles(rec[:-1])                                # another count: the uniform value again, counted
    s.step()
    Tp = s.particle_temperatures()
    assert Tp.size == 199 and s.particle_temperature_resets() == 1
    assert np.abs(Tp - 222.0).max() > 0 and Tp.min() >= 222.0 and Tp.max() < 300.0       # one step from 222 towards the fluid's 300
    s.set_particle_temperatures(None)                        # re-initialised, not counted
    assert (s.particle_temperatures() == 222.0).all() and s.particle_temperature_resets() == 1
    s.close()
    # particle_cp == 0: the caller owns Tp; the getter returns what was set, and a step leaves it alone
    s = product.Solver(bed_case(product, thermal(product, 40, T_initial=300.0, particle_temperature=222.0, **WATER)))
    s.set_particles(rec)
    assert (s.particle_temperatures() == 222.0).all()
    s.set_particle_temperatures(a)
    s.step()
    np.testing.assert_array_equal(s.particle_temperatures(), a)
    assert np.abs(s.particle_heat()).max() > 0 and s.particle_temperature_resets() == 0
    s.close()
    cold = product.Solver(bed_case(product))
    cold.set_particles(rec)
    with pytest.raises(product.FoamYadeError) as e:
        cold.particle_temperatures()                         # no heat transfer
    assert "error 1" in str(e.value) and "heat transfer" in str(e.value)
    cold.close()


# ---- 7. the buoyancy field -------------------------------------------------------------------------------------------------------------------------------------
def separate_particles():
    """four particles of the bed box, any two of them five or more cells apart along some axis (a stencil reaches two cells): no cell receives from two of them, so the
    Gaussian scatter's sums have one term each and uSource is reproducible bit for bit"""
    rec = np.zeros((4, 10))
    rec[:, 0:3] = [(0.025, 0.025, 0.025), (0.095, 0.075, 0.025), (0.025, 0.075, 0.065), (0.095, 0.025, 0.065)]
    rec[:, 3:6] = [(0.05, 0, 0), (0, -0.05, 0), (0, 0, 0.05), (-0.03, 0.03, 0)]
    rec[:, 9] = 0.002
    return rec


@pytest.mark.parametrize("solver", ["ico", "pimple"])
def test_buoyancy_field_is_exact(product, solver):
    beta, T_ref = 2.1e-4, 293.0
    out = {}
    for b in (beta, 0.0):
        th = thermal(product, 50, T_initial=300.0, particle_temperature=350.0, beta=b, T_ref=T_ref, **WATER)
        if solver == "ico":
            nx, ny, nz, dx = 6, 5, 4, 0.1 / 6
            g = (0.7, -1.3, -9.81)
            u_val = [(0, 0, 0)] * 6
            u_val[3] = (1.0, 0, 0)
            s = product.Solver(product.make_case(0, nx, ny, nz, dx, 1e-3, 1e-2, g=g, u_val=u_val, thermal=th))
            rec = one_per_cell(nx, ny, nz, dx, 40, 11)
        else:
            nx, ny, nz = BOX
            g = (0, 0, -9.81)
            s = product.Solver(bed_case(product, th))
            rec = separate_particles()
        Nc = nx * ny * nz
        T0 = 280.0 + 40.0 * np.random.RandomState(5).random_sample(Nc)
        s.set("T", T0)
        s.hold_sources(True)
        s.enable_kernel_timing(True)
        s.set_particles(rec)
        s.step()
        if solver == "pimple":
            ids = s.stencils()[1]
            assert np.unique(ids[ids >= 0]).size == (ids >= 0).sum()      # no shared cell
        out[b] = (s.get("uSource"), s.get("U"))
        if b:
            a = s.get("buoyancy").reshape(Nc, 3)
            assert np.array_equal(a, tl.buoyancy(T0, beta, T_ref, g))
            assert (np.abs(a).max(axis=0) > 0).tolist() == [gq != 0 for gq in g]
            assert s.kernel_timing("buoyancy")[1] == 1
        else:
            with pytest.raises(product.FoamYadeError):
                s._size("buoyancy")                          # beta == 0: nothing allocated
            assert s.kernel_timing("buoyancy") == (0.0, 0)
        s.close()
    assert np.array_equal(out[beta][0], out[0.0][0]) and np.abs(out[0.0][0]).max() > 0      # uSource stays what the coupling left
    assert np.abs(out[beta][1] - out[0.0][1]).max() > 0                                     # and the flow feels the difference


# ---- 8. T == T_ref --------------------------------------------------------------------------------------------------------------------------------------------
def test_reference_temperature_is_a_bitwise_no_op(product):
    """T0 = Tp = T_ref = 0: every term of the heat exchange is an exact zero, T stays exactly T_ref, the buoyant acceleration is (-beta * 0) * g = -0.0 * g, and adding a
    signed zero changes no bit of uSource's sum.  The particles sit more than four cells apart (separate_particles) so that two runs of the SAME code agree bit for bit:
    a crowded bed's scatter adds through atomics in an order that differs from run to run (tests/test_heat_transfer.py::test_pimple_box_is_unchanged_by_thermal)"""
    out = []
    for beta in (3e-4, 0.0):
        s = product.Solver(bed_case(product, thermal(product, 40, T_initial=0.0, particle_temperature=0.0, particle_cp=CPP_BED, beta=beta, T_ref=0.0, **WATER)))
        rec = separate_particles()
        for step in range(4):
            rec[:, 0:3] += 2e-4 * rec[:, 3:6]
            s.set_particles(rec)
            s.step()
        out.append((s.get("U"), s.get("p"), s.get("T")))
        if beta:
            assert (s.get("buoyancy") == 0.0).all()
        s.close()
    for a, b, nm in zip(out[0], out[1], ("U", "p", "T")):
        assert np.array_equal(a, b), nm
    assert np.abs(out[0][0]).max() > 0 and (out[0][2] == 0.0).all()


# ---- 9. stratified rest state ----------------------------------------------------------------------------------------------------------------------------------
def test_stratified_rest_state(product):
    """a closed box of fluid whose temperature rises linearly with height is at rest under dp/dz = (1 - beta (T - T_ref)) g_z: fixedFluxPressure walls balance the
    buoyancy that travels through phicForces.  Bounds: tests/test_fv_parity.py::test_hydrostatic_fixed_flux's, which are solver-tolerance bounds"""
    nx, ny, nz, dx = 6, 6, 12, 0.01
    beta, T_ref, gz, dTdz = 2e-4, 300.0, -9.81, 200.0
    z = (np.arange(nz) + 0.5) * dx
    prof = T_ref + dTdz * (z - 0.5 * nz * dx)
    T0 = np.repeat(prof, nx * ny)
    th = thermal(product, 200, T_initial=T_ref, T_bc=[0, 0, 0, 0, 1, 1], T_value=[0, 0, 0, 0, T_ref - dTdz * 0.5 * nz * dx, T_ref + dTdz * 0.5 * nz * dx], beta=beta, T_ref=T_ref, **WATER)
    s = product.Solver(product.make_case(1, nx, ny, nz, dx, 1e-3, 1e-6, g=(0, 0, gz), p_bc=[2] * 6, p_tol=1e-12, p_final_tol=1e-12, p_rel_tol=0.0, thermal=th))
    s.set("T", T0)
    for _ in range(5):
        s.step()
    umax = np.abs(s.get("U")).max()
    p = s.get("p").reshape(nz, ny, nx)
    d2 = (p[2:] - 2.0 * p[1:-1] + p[:-2]) / dx ** 2
    want = -beta * gz * dTdz
    print(f"max|U| = {umax:.3e}; d2p/dz2 in [{d2.min():.9e}, {d2.max():.9e}], expected {want:.9e}: relative error {np.abs(d2 / want - 1).max():.2e}")
    assert umax < 1e-8
    np.testing.assert_allclose(d2, want, rtol=1e-5)
    assert_field(s.get("T"), T0, "stratified T")
    a = s.get("buoyancy").reshape(-1, 3)
    assert np.abs(a[:, 2]).max() > 1e-3 and (a[:, :2] == 0).all()
    s.close()


# ---- 11. refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_create_refuses_what_it_cannot_run(product):
    mk = lambda rho_p=2650.0, **kw: product.Solver(product.make_case(1, 4, 4, 4, 0.01, 1e-3, 1e-2, rho_p=rho_p, thermal=thermal(product, 10, **kw, **WATER)))
    with pytest.raises(product.FoamYadeError) as e:
        mk(particle_cp=-1.0)
    assert "error 1" in str(e.value) and "particle_cp" in str(e.value)
    with pytest.raises(product.FoamYadeError) as e:
        mk(rho_p=0.0, particle_cp=800.0)
    assert "error 1" in str(e.value) and "rho_particle" in str(e.value) and "particle_cp" in str(e.value)
    for kw, name in ((dict(beta=float("nan")), "beta"), (dict(beta=float("inf")), "beta"), (dict(T_ref=float("nan")), "T_ref"), (dict(beta=1e-4, T_ref=float("-inf")), "T_ref")):
        with pytest.raises(product.FoamYadeError) as e:
            mk(**kw)
        assert "error 1" in str(e.value) and name in str(e.value)
    mk(particle_cp=800.0, beta=2e-4, T_ref=300.0).close()


def test_executable_prints_the_three_entries(product, tmp_path):
    import os
    import subprocess
    from test_heat_transfer_case import heat_case
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yade-openfoam-coupling_amd", "bin", "foamYadeHip")
    if not os.path.exists(exe):
        pytest.fail("foamYadeHip has not been built: run __graft_entry__.build()")
    dst = heat_case(tmp_path, "bed_pimple", coupling="heatTransfer { active on; Cp 1000; kappa 50; particleTemperature 350; particleCp 840; beta 2e-4; TRef 300; }\n",
                    entries={"bottom": "type fixedValue; value uniform 320;", "top": "type fixedValue; value uniform 290;"})
    out = subprocess.run([exe, "-solver", "pimple", "-case", str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("Heat transfer:")]
    assert len(lines) == 1 and "particleCp 840" in lines[0] and "beta 0.0002" in lines[0] and "TRef 300" in lines[0], out.stdout
    assert "Particle temperatures:" not in out.stdout        # no batch, no reset
    assert os.path.exists(dst / "0.002" / "T.water")         # the run went to its end with the loop on


# ---- 10. differentially heated cavity ---------------------------------------------------------------------------------------------------------------------------
# de Vahl Davis (1983), Ra = 1e3, Pr = 0.71: wall-averaged Nusselt number 1.118.  Measured on an MI355X (DESIGN_HISTORY.md "Heat exchange"): Nu = 1.122708 at 16^2 after
# 118 steps, 1.119062 at 32^2 after 310 steps; the hot and the cold wall differ by 1.9e-9 and 1.4e-12 (what is left of the transient where the run stops).  The bounds
# are twice the measured 32^2 deviation and twice the larger hot / cold difference: headroom for another machine's iteration counts, and no more.
NU_BENCHMARK = 1.118
CAVITY_DEVIATION_32 = 1.0622e-3                              # |Nu(32^2) - 1.118| as measured (0.095 %)
CAVITY_HOT_COLD = 1.87e-9                                    # |Nu_hot - Nu_cold| as measured (the larger of the two grids: 16^2)
CAVITY_NZ = 1                                                # the block takes one layer of cells


def cavity_nusselt(product, n, nz=CAVITY_NZ, dt=4e-3, **kw):
    """unit square, hot wall x = 0 (T = 1), cold wall x = 1 (T = 0), adiabatic y walls, g along -y, slip z sides; alpha_T = 1, nu = 0.71, g beta = 710: Ra = 1e3.
    Returns (Nu_hot, Nu_cold, steps, max|U|) at the steady state: the wall cells' one-sided difference (T_wall - T_cell) / (dx / 2), averaged over the wall.
    Three outer correctors: with one, the PIMPLE loop's pressure-velocity splitting leaves a transient at 32^2 that decays by a fixed factor per STEP whatever the time step
    (measured: 0.987 per step at dt 2e-3, 4e-3 and 8e-3 alike, 1e-6 per step still left after 600), i.e. an iteration error, not physics; with three it is gone in 310 steps"""
    dx, nu = 1.0 / n, 0.71
    th = thermal(product, 2000, cp=1.0, kappa=1.0, T_initial=0.5, T_bc=[1, 1, 0, 0, 0, 0], T_value=[1.0, 0.0, 0, 0, 0, 0], T_tol=1e-12, beta=71.0, T_ref=0.5)
    u_bc = [0, 0, 0, 0, 2, 2]
    s = product.Solver(product.make_case(1, n, n, nz, dx, dt, nu, rho_f=1.0, g=(0, -10.0, 0), u_bc=u_bc, p_bc=[2] * 6, u_tol=1e-11, p_tol=1e-11, p_final_tol=1e-11,
                                         p_rel_tol=0.0, n_outer_correctors=3, thermal=th, **kw))
    last, steps, trace = None, 0, []
    for steps in range(1, 601):
        s.step()
        T = s.get("T").reshape(nz, n, n)
        hot, cold = ((1.0 - T[:, :, 0]) / (0.5 * dx)).mean(), ((T[:, :, -1] - 0.0) / (0.5 * dx)).mean()
        if last is not None and steps % 50 == 0:
            trace.append(f"{steps}: {hot - last:+.2e}")
        if last is not None and abs(hot - last) < 1e-7:
            break
        last = hot
    print(f"{n}^2: change of Nu_hot per step at step " + ", ".join(trace))
    umax = np.abs(s.get("U")).max()
    s.close()
    return hot, cold, steps, umax


def test_differentially_heated_cavity(product):
    res = {n: cavity_nusselt(product, n) for n in (16, 32)}
    for n, (hot, cold, steps, umax) in res.items():
        print(f"{n}^2: Nu_hot {hot:.6f}, Nu_cold {cold:.6f}, |hot - cold| {abs(hot - cold):.3e}, deviation from {NU_BENCHMARK} {abs(hot - NU_BENCHMARK):.3e} "
              f"({abs(hot / NU_BENCHMARK - 1) * 100:.2f} %), {steps} steps, max|U| {umax:.4f}")
    dev = {n: abs(res[n][0] - NU_BENCHMARK) for n in res}
    gap = max(abs(res[n][0] - res[n][1]) for n in res)
    assert all(res[n][2] < 600 for n in res), "no steady state within 600 steps"
    assert dev[32] < dev[16]
    assert dev[32] <= 2.0 * CAVITY_DEVIATION_32 and gap <= 2.0 * CAVITY_HOT_COLD
