"""tests/thermal_loop_ref.py against closed forms, and the C-ABI of the thermal loop (no GPU): the restatement the device is held to must itself be right."""
import ctypes

import numpy as np
import pytest

import heat_transfer_ref as ht
import thermal_loop_ref as tl


@pytest.fixture
def prod():
    from conftest import load_product
    return load_product()


@pytest.mark.parametrize("r_p", [0.1, 5.0])
def test_step_reproduces_the_two_body_recurrence(r_p):
    """one particle in every cell with weight 1: the loop's step is the closed recurrence cell by cell, and the pair is the backward-Euler step
    m c (Tp' - Tp) = dt hA (T' - Tp') = -C (T' - T) with the UNDAMPED hA"""
    N, dt, hA, C = 7, 0.02, 3e-3, 1e-3
    mc = dt * hA / r_p
    ids, w = ht.point_stencils(np.arange(N))
    T, Tp = np.zeros(N), np.full(N, 50.0)
    Ts, Tps, qs = tl.two_body(0.0, 50.0, hA, dt, C, mc, 6)
    for n in range(6):
        Tn, Tpn, q = tl.step_at_rest(np.full(N, hA), ids, w, T, Tp, dt, mc, np.full(N, C))
        np.testing.assert_allclose(Tn, Ts[n], rtol=1e-14)
        np.testing.assert_allclose(Tpn, Tps[n], rtol=1e-14)
        np.testing.assert_allclose(q, qs[n], rtol=1e-13)
        np.testing.assert_allclose(mc * (Tpn - Tp), dt * hA * (Tn - Tpn), rtol=1e-12)      # the elimination: backward Euler in Tp'
        np.testing.assert_allclose(mc * (Tpn - Tp), -C * (Tn - T), rtol=1e-12)
        assert (Tpn < Tp).all() and (Tpn > Tn).all()                                        # monotone, no overshoot, for any r_p
        T, Tp = Tn, Tpn
    # the exact solution of the pair's backward-Euler step, solved as a 2 x 2 system
    A = np.array([[C + dt * hA, -dt * hA], [-dt * hA, mc + dt * hA]])
    x = np.linalg.solve(A, np.array([C * 0.0, mc * 50.0]))
    np.testing.assert_allclose([Ts[0], Tps[0]], x, rtol=1e-13)


def test_random_stencils_conserve_the_total_heat_content():
    rs = np.random.RandomState(5)
    n, K, Nc, dt = 400, 6, 60, 0.03
    ids = rs.randint(0, Nc, (n, K))
    w = rs.random_sample((n, K))
    short = rs.randint(1, K + 1, n)                      # 1 .. K entries per particle, five particles with none
    short[:5] = 0
    for p in range(n):
        ids[p, short[p]:] = -1
        w[p, short[p]:] = 0.0
    w[5:] /= w[5:].sum(axis=1, keepdims=True)
    hA = 1e-3 * (0.5 + rs.random_sample(n))
    hA[:5] = 0.0
    mc = 2e-4 * (0.2 + rs.random_sample(n))
    C = 5e-3 * (0.5 + rs.random_sample(Nc))
    T, Tp = 300.0 + 40.0 * rs.random_sample(Nc), 280.0 + 90.0 * rs.random_sample(n)
    total = (C * T).sum() + (mc * Tp).sum()
    for _ in range(4):
        Tn, Tpn, q = tl.step_at_rest(hA, ids, w, T, Tp, dt, mc, C)
        assert (Tpn[:5] == Tp[:5]).all() and (q[:5] == 0.0).all()
        exchanged = dt * np.abs(q).sum()
        assert abs((mc * (Tpn - Tp)).sum() - dt * q.sum()) <= 1e-10 * exchanged
        assert abs((C * (Tn - T)).sum() + dt * q.sum()) <= 1e-10 * exchanged
        T, Tp = Tn, Tpn
    assert abs((C * T).sum() + (mc * Tp).sum() - total) <= 1e-13 * total
    assert Tp.min() >= 280.0 and Tp.max() <= 370.0 and T.min() >= 280.0 and T.max() <= 370.0      # monotone: nothing leaves the initial range


def test_buoyancy_keeps_its_operation_order():
    T = np.array([300.0, 310.5, 289.25])
    a = tl.buoyancy(T, 2e-4, 300.0, (0.0, 0.0, -9.81))
    assert a.shape == (3, 3) and (a[:, :2] == 0.0).all()
    assert a[1, 2] == (-2e-4 * (310.5 - 300.0)) * -9.81 and a[2, 2] < 0 < a[1, 2]


def test_descriptor_mirror_and_symbol(prod):
    """the three new fields close fy_thermal_desc, and the getter is exported with its argument types declared"""
    names = [f[0] for f in prod.ThermalDesc._fields_]
    assert names[-3:] == ["particle_cp", "beta", "T_ref"] and names[-4] == "particle_temperature"
    d = prod.thermal_desc(cp=4180.0, kappa=0.6)
    assert (d.particle_cp, d.beta, d.T_ref) == (0.0, 0.0, 0.0)
    d = prod.thermal_desc(cp=4180.0, kappa=0.6, particle_cp=800.0, beta=2e-4, T_ref=300.0)
    assert (d.particle_cp, d.beta, d.T_ref) == (800.0, 2e-4, 300.0)
    L = prod.lib()
    assert L.fy_solver_get_particle_thermal_state.argtypes[1] is ctypes.c_int
    assert L.fy_solver_get_particle_thermal_state(None, 0, None, None) != 0                 # a null solver is refused, not dereferenced
