"""tests/porous_ref.py against itself (no GPU): the properties the operator has by construction, and the Python mirror's descriptor."""
import ctypes as C

import numpy as np

import porous_ref as pr


def cells(n=40, seed=3):
    rs = np.random.RandomState(seed)
    return 0.4 + 0.6 * rs.random_sample(n), 1e-6 * (0.5 + rs.random_sample(n)), rs.standard_normal((n, 3))


def test_darcy_row_is_linear_in_U():
    a, V, U = cells()
    d, f0 = np.array([3e4, 1e3, 7e5]), np.zeros(3)
    r1 = pr.row_additions(a, V, 1e-5, d, f0, U)
    r2 = pr.row_additions(a, V, 1e-5, d, f0, 3.7 * U)
    assert np.array_equal(r1, r2)                                        # f = 0: the coefficient does not see U, so the row's product with U is linear in it
    F1, F2 = pr.force(a, V, 1e-5, d, f0, U), pr.force(a, V, 1e-5, d, f0, 2.0 * U)
    assert np.array_equal(F2, 2.0 * F1)                                  # (a factor 2 is exact in binary)
    Fa, Fb = pr.force(a, V, 1e-5, d, f0, U), pr.force(a, V, 1e-5, d, f0, U[::-1].copy())
    Fs = pr.force(a, V, 1e-5, d, f0, U + U[::-1])
    assert np.all(np.abs(Fs - (Fa + Fb)) <= 4 * len(a) * pr.EPS * (np.abs(pr.row_additions(a, V, 1e-5, d, f0, U)) * (np.abs(U) + np.abs(U[::-1]))).sum(axis=0))


def test_forchheimer_row_is_quadratic_and_uses_the_half():
    a, V, U = cells()
    f = np.array([20.0, 5.0, 90.0])
    r1 = pr.row_additions(a, V, 1e-5, np.zeros(3), f, U)
    r2 = pr.row_additions(a, V, 1e-5, np.zeros(3), f, 2.0 * U)
    assert np.array_equal(r2, 2.0 * r1)
    one = pr.coeff(0.0, np.zeros(3), np.array([1.0, 1.0, 1.0]), np.array([[3.0, 4.0, 12.0]]))
    assert np.array_equal(one, np.full((1, 3), 6.5))                     # 0.5 |U|, |(3, 4, 12)| = 13


def test_row_restates_the_force():
    a, V, U = cells(300)
    d, f = np.array([3e4, 1e3, 7e5]), np.array([20.0, 5.0, 90.0])
    bd = pr.row_additions(a, V, 1e-5, d, f, U)
    F = pr.force(a, V, 1e-5, d, f, U)
    assert np.array_equal((bd * U).sum(axis=0), F)
    ld = (bd.astype(np.longdouble) * U.astype(np.longdouble)).sum(axis=0)
    assert np.all(np.abs(F - ld.astype(np.float64)) <= 300 * pr.EPS * np.abs(bd * U).sum(axis=0))


def test_scatter_and_relaxation():
    a, V, U = cells(30)
    zones = [dict(cells=[1, 5, 7], d=(1e4, 2e4, 3e4), f=(1.0, 2.0, 3.0)), dict(cells=[0, 29], d=(0, 0, 5e5), f=(0, 0, 40.0))]
    pc = pr.diagonal_additions(30, zones, a, V, 1e-5, U)
    assert np.count_nonzero(pc.any(axis=1)) == 5 and np.array_equal(pr.zone_map(30, zones)[[0, 1, 2, 29]], [2, 1, 0, 2])
    diag0 = np.full(30, 1e-3); src0 = np.zeros((30, 3)); off = np.full(30, 5e-4)
    dn, src = pr.relaxed(diag0, src0, U, off, np.zeros(30), np.zeros(30), pc, 0.7)
    out = ~pc.any(axis=1)
    assert np.array_equal(dn[out], diag0[out] / 0.7)                     # dominant rows outside the zones: D / relax
    assert np.all(dn[~out] > dn[out][0]) and np.array_equal(src, (dn - diag0)[:, None] * U)
    assert np.array_equal(dn[~out], (diag0[~out] + pc[~out].max(axis=1)) / 0.7)


def test_descriptor_mirror(product):
    z = [dict(name="plate", cells=[3, 4, 9], d=(1, 2, 3), f=(4, 5, 6)), dict(name="sieve", cells=np.arange(20, 25), d=(0, 0, 7e5), f=(0, 0, 0))]
    d = product.porous_desc(z)
    assert d.n_zones == 2 and d.zones[0].name == b"plate" and list(d.zones[0].d) == [1, 2, 3] and list(d.zones[1].f) == [0, 0, 0]
    assert d.zones[1].n_cells == 5 and [d.zones[1].cells[q] for q in range(5)] == [20, 21, 22, 23, 24]
    assert C.sizeof(product.PorousZone) == 32 + 48 + 8 + 8 and C.sizeof(product.PorousDesc) == 8 + 8 * C.sizeof(product.PorousZone)
    assert product.porous_desc([dict(cells=[q]) for q in range(9)]).n_zones == 9            # kept for the setter to refuse
    ctr = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5]])
    assert list(product.cells_in_box(ctr, (0.5, 0, 0), (1.5, 1, 1))) == [0, 1]               # the closed box (boxToCell)
    L = product.lib()
    for nm in ("fy_solver_set_porous_zones", "fy_solver_get_porous_stats", "fy_ldu_solver_set_porous_zones", "fy_ldu_solver_get_porous_stats"):
        assert hasattr(L, nm)
    L.fy_solver_set_porous_zones.argtypes = [C.c_void_p, C.c_void_p]
    assert L.fy_solver_set_porous_zones(None, None) != 0                 # a null solver is refused, not dereferenced
