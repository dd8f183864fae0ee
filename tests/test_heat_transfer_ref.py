"""tests/heat_transfer_ref.py against closed forms, and the C-ABI of the heat exchange (no GPU): the restatement the device is held to must itself be right."""
import ctypes

import numpy as np
import pytest

import heat_transfer_ref as ht


@pytest.fixture
def prod():
    from conftest import load_product
    return load_product()


ZG = [ht.ZERO_GRADIENT] * 6


def zero_phi(nx, ny, nz):
    return np.zeros((nx + 1) * ny * nz), np.zeros(nx * (ny + 1) * nz), np.zeros(nx * ny * (nz + 1))


def test_cosine_mode_between_adiabatic_walls_decays_by_the_discrete_factor():
    """cos(pi (i + 1/2) / nx) is an eigenvector of the 3-point Laplacian with zero-gradient ends: eigenvalue lambda_h = (2 / dx^2)(1 - cos(pi / nx)), so one implicit
    Euler step multiplies it by exactly 1 / (1 + dt D lambda_h)"""
    nx, ny, nz, dx, dt, D = 16, 4, 4, 0.01, 0.05, 2e-4
    h = ht.block_sizes(nx, ny, nz, dx)
    mode = np.tile(np.cos(np.pi * (np.arange(nx) + 0.5) / nx), ny * nz)
    lam = (2.0 / dx ** 2) * (1.0 - np.cos(np.pi / nx))
    T = 300.0 + 5.0 * mode
    for step in range(1, 4):
        T = ht.solve_T(h, dt, zero_phi(nx, ny, nz), None, None, T, D, 1.0, ZG, [0.0] * 6, ht.LINEAR)
        assert np.abs(T - (300.0 + 5.0 * mode / (1.0 + dt * D * lam) ** step)).max() <= 1e-12 * 5.0


def test_one_particle_per_cell_at_rest_relaxes_geometrically():
    """uniform T0, a particle at rest in every cell of a fluid at rest: T1 = (T0 + beta Tp) / (1 + beta), beta = dt hA / (rho cp V), and Nu = 2 up to the `small` in Re"""
    n, dx, dt = 4, 0.01, 0.02
    nu, rho, cp, kappa, Tp, T0 = 1e-6, 1000.0, 4180.0, 0.6, 350.0, 300.0
    Pr = ht.prandtl(nu, rho, cp, kappa)
    N = n ** 3
    rec = np.zeros((N, 10)); rec[:, 9] = 0.1 * dx
    ids, w = ht.point_stencils(np.arange(N))
    hA, Sp, Su = ht.pass_a(ht.RANZ_MARSHALL, rec, ids, w, np.zeros((N, 3)), None, Tp, nu, kappa, Pr, N)
    Nu = hA / (kappa * np.pi * 0.2 * dx)
    assert np.abs(Nu - 2.0).max() < 1e-4
    h = ht.block_sizes(n, n, n, dx)
    T = np.full(N, T0)
    beta = dt * hA[0] / (rho * cp * dx ** 3)
    for step in range(1, 6):
        Tn = ht.solve_T(h, dt, zero_phi(n, n, n), None, None, T, kappa / (rho * cp), 1.0, ZG, [0.0] * 6, ht.LINEAR, Sp, Su, rho * cp)
        q = ht.pass_b(hA, ids, w, Tn, Tp)
        assert np.abs(Tn - (Tp + (T0 - Tp) / (1.0 + beta) ** step)).max() <= 1e-12 * Tp
        # what the particles received left the fluid: rho cp V (T - T_old) = -dt q per cell.  T - T_old cancels: each T carries half an ulp of 300, so the
        # bound is a few ulps of the cell's heat content rho cp V T, not of the exchanged heat
        assert np.abs(rho * cp * dx ** 3 * (Tn - T) + dt * q).max() <= 16 * np.finfo(float).eps * rho * cp * dx ** 3 * Tn.max()
        T = Tn


def test_both_laws_give_two_in_a_fluid_at_rest():
    for law in (ht.RANZ_MARSHALL, ht.GUNN):
        assert ht.nusselt(law, 1.0, 0.0, 6.9) == 2.0
    # and grow with Re; Gunn's grows as the bed gets denser
    assert ht.nusselt(ht.RANZ_MARSHALL, 1.0, 100.0, 0.7) == pytest.approx(2.0 + 6.0 * 0.7 ** (1 / 3))
    assert ht.nusselt(ht.GUNN, 0.4, 50.0, 0.7) > ht.nusselt(ht.GUNN, 0.9, 50.0, 0.7) > 2.0


@pytest.mark.parametrize("law", [ht.RANZ_MARSHALL, ht.GUNN])
def test_the_exchange_is_conservative_on_random_stencils(law):
    """sum_p q_p = sum_c (Sp_c T_c - Su_c) for ANY T, because each particle's weights sum to one"""
    rs = np.random.RandomState(5)
    n, Nc, K = 400, 90, 16
    k = rs.randint(0, 13, n)                                # some particles without a stencil
    ids = np.full((n, K), -1, np.int32); w = np.zeros((n, K))
    for p in range(n):
        ids[p, :k[p]] = rs.choice(Nc, k[p], replace=False)
        ww = rs.random_sample(k[p]) + 0.01
        w[p, :k[p]] = ww / ww.sum()
    rec = np.zeros((n, 10)); rec[:, 3:6] = rs.standard_normal((n, 3)); rec[:, 9] = 1e-3 * (0.5 + rs.random_sample(n))
    U, alpha, T, Tp = rs.standard_normal((Nc, 3)), 0.4 + 0.6 * rs.random_sample(Nc), 300 + 50 * rs.random_sample(Nc), 280 + 90 * rs.random_sample(n)
    hA, Sp, Su = ht.pass_a(law, rec, ids, w, U, alpha, Tp, 1e-6, 0.6, 6.9, Nc)
    q = ht.pass_b(hA, ids, w, T, Tp)
    assert (hA[k == 0] == 0).all() and (q[k == 0] == 0).all() and (hA[k > 0] > 0).all()
    assert abs(q.sum() - (Sp * T - Su).sum()) <= 1e-12 * np.abs(q).sum()


def test_graded_fixed_value_walls_hold_a_linear_profile():
    """steady conduction between two fixedValue walls is linear in x on ANY grading: the half-cell boundary distance and the face weights must agree with it"""
    hx = 0.01 * 1.3 ** np.arange(6); hy = np.full(5, 0.02); hz = 0.015 * 0.8 ** np.arange(4)
    h = [hx, hy, hz]
    xc = np.cumsum(hx) - 0.5 * hx
    bc = [ht.FIXED_VALUE, ht.FIXED_VALUE] + [ht.ZERO_GRADIENT] * 4
    val = [300.0, 400.0, 0, 0, 0, 0]
    exact = np.tile(300.0 + 100.0 * xc / hx.sum(), 20)
    T = ht.solve_T(h, 1e30, zero_phi(6, 5, 4), None, None, exact * 0, 1e-4, 1.0, bc, val, ht.LINEAR)
    assert np.abs(T - exact).max() <= 1e-10 * 100.0


def test_abi_carries_the_thermal_descriptor_and_entry_points(prod):
    L = ctypes.CDLL(prod.LIB_PATH)
    assert L.fy_abi_version() >= 18
    for name in ("fy_solver_set_particle_temperatures_host", "fy_solver_set_particle_temperatures_device", "fy_solver_get_particle_heat_host", "fy_solver_get_thermal_stats"):
        assert hasattr(L, name), name
    c = prod.case_defaults(prod.FY_SOLVER_PIMPLE)
    t = c.thermal
    assert (t.on, t.cp, t.kappa, t.prt, t.nusselt_law, t.T_initial, t.T_max_iter, t.particle_temperature) == (0, 0, 0, 0, 0, 0, 0, 0)      # all zero: off
    assert list(t.T_bc) == [0] * 6 and list(t.T_value) == [0.0] * 6
    # the descriptor is the LAST member: fy_case_defaults clears exactly the bytes the mirror describes (a poisoned tail would survive a shorter C struct)
    poisoned = prod.CaseDesc()
    ctypes.memset(ctypes.byref(poisoned), 0xff, ctypes.sizeof(poisoned))
    prod.lib().fy_case_defaults(ctypes.byref(poisoned), 1)
    assert poisoned.thermal.on == 0 and poisoned.thermal.particle_temperature == 0.0 and poisoned.average.n_items == 0
    d = prod.thermal_desc(4180.0, 0.6, T_initial=300.0, T_bc=[1, 1, 0, 0, 0, 0], T_value=[300, 350, 0, 0, 0, 0], nusselt_law=prod.NUSSELT_GUNN, particle_temperature=320.0)
    assert (d.on, d.nusselt_law, d.T_bc[1], d.T_value[1], d.particle_temperature) == (1, 1, 1, 350.0, 320.0)
