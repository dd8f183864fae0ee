"""The explicit stress term of pimpleFoamYade's momentum equation, div(alpha nuEff dev2(T(grad U))): one LDS-tiled sweep (k_stress_div, the default on one
domain without linearUpwind) against the two sweeps that hand the tensor through memory (k_pre_coupling + k_div_G, FOAMYADE_NO_TILED_STRESS=1).  Both form every
value by the same device functions in the same order and nothing is reduced, so divG -- and with it every field of a fluid-only run and every iteration
count -- is the same BITS.  The shapes are the smallest at which a 16 x 8 x 4 tile can go wrong."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = (16, 8, 4)
SWITCH = "FOAMYADE_NO_TILED_STRESS"
FIELDS = ("U", "p", "phi_x", "phi_y", "phi_z", "mom_src", "mom_diag", "divG")

FV, ZG, SLIP = 0, 1, 2            # FY_BC_U_*
PZG, PFV, PFLUX = 0, 1, 2         # FY_BC_P_*


def closed_box():
    """C3's boundary set: no-slip walls, fixedFluxPressure, gravity"""
    return dict(g=(0, 0, -9.81), u_bc=[FV] * 6, u_val=[(0, 0, 0)] * 6, p_bc=[PFLUX] * 6)


def c5_set(sides=FV):
    """C5's boundary set: z- inlet fixedValue, z+ outlet zeroGradient with p = 0, `sides` on x and y"""
    return dict(g=(0, 0, -9.81), u_bc=[sides] * 4 + [FV, ZG], u_val=[(0, 0, 0)] * 4 + [(0, 0, 0.05), (0, 0, 0)], p_bc=[PFLUX] * 5 + [PFV], p_val=[0.0] * 6)


def sizes(n, ratio):
    """n cell sizes in geometric progression, last / first = ratio, summing to 0.1"""
    h = ratio ** (np.arange(n) / max(n - 1, 1))
    return h * (0.1 / h.sum())


def both_paths(product, monkeypatch, dims, seed, **kw):
    """the same case on the default path and with the switch set: ((fields, iteration counts, stores the tensor?) x 2)"""
    nx, ny, nz = dims
    out = []
    for off in (False, True):
        if off:
            monkeypatch.setenv(SWITCH, "1")
        s = product.Solver(product.make_case(1, nx, ny, nz, 0.1 / max(dims), 2e-4, 1e-5, p_solver=1, **kw))
        s.set("U", np.random.RandomState(seed).rand(nx * ny * nz, 3) * 0.05)
        its = []
        for step in range(3):
            s.step()
            st = s.stats()
            its.append((st["p_iters_total"], st["u_iters_total"]))
        try:
            s.get("stress_G")
            stored = True
        except product.FoamYadeError:
            stored = False
        out.append(({nm: s.get(nm) for nm in FIELDS}, its, stored))
        s.close()
    monkeypatch.delenv(SWITCH)
    product.Solver(product.make_case(0, 8, 8, 8, 0.1, 1e-3, 0.01, p_solver=1)).close()      # (re-reads the switch for the tests that follow)
    return out


def assert_same_bits(a, b):
    (fa, its_a, _), (fb, its_b, _) = a, b
    print("iterations (p, u) per step:", its_a, its_b)
    assert its_a == its_b, (its_a, its_b)
    assert all(p > 0 and u > 0 for p, u in its_a), its_a
    for nm in FIELDS:
        np.testing.assert_array_equal(fa[nm], fb[nm], err_msg=nm)
    assert fa["divG"].size == 3 or np.abs(fa["divG"]).max() > 0        # (one cell: every face takes the cell's own row, the divergence is zero)


CASES = {
    # no extent a multiple of a tile edge: partial tiles on every high side, in z fewer cells than two tiles
    "19x11x7_closed_box": ((19, 11, 7), closed_box()),
    "one_tile": (TILE, closed_box()),
    "one_tile_plus_one_cell": (tuple(t + 1 for t in TILE), closed_box()),
    # a slab cell of one tile that is a boundary cell in another direction takes the patch rules: fixedValue, zeroGradient, slip
    "32x16x8_c5": ((32, 16, 8), c5_set()),
    "32x16x8_c5_slip_sides": ((32, 16, 8), c5_set(SLIP)),
    "19x11x7_graded": ((19, 11, 7), dict(closed_box(), grading=(sizes(19, 3.0), sizes(11, 0.5), sizes(7, 2.0)))),
    "16x16x16_smagorinsky": ((16, 16, 16), dict(closed_box(), turbulence_model=1, nut_initial=1e-5)),
    # the smallest block a case can have: one cell, every face a patch (the C5 set, so that the pressure equation has something to solve)
    "1x1x1": ((1, 1, 1), c5_set()),
}


@pytest.mark.parametrize("name", list(CASES))
def test_tiled_stress_sweep_equals_the_two_sweeps(product, name, monkeypatch):
    dims, kw = CASES[name]
    a, b = both_paths(product, monkeypatch, dims, 11, **kw)
    assert not a[2] and b[2], "the default path must keep the tensor in LDS, the switch must bring the stored tensor back"
    assert_same_bits(a, b)


def test_linear_upwind_keeps_the_two_sweeps(product, monkeypatch):
    """linearUpwind reads grad U stored by the sweep that forms G: the two-sweep path whatever the switch says"""
    a, b = both_paths(product, monkeypatch, (19, 11, 7), 12, convection_scheme=2, **closed_box())
    assert a[2] and b[2]
    assert_same_bits(a, b)
