"""tests/open_boundary_ref.py held to what it must reduce to (no GPU): the restatement the device code of the open boundaries is compared with."""
import numpy as np

import open_boundary_ref as ob


def test_a_normal_along_z_gives_the_diagonal_1_1_0():
    np.testing.assert_array_equal(ob.pio_diag([0.0, 0.0, 1.0]), [1.0, 1.0, 0.0])
    np.testing.assert_array_equal(ob.pio_diag([0.0, 0.0, -1.0]), [1.0, 1.0, 0.0])
    np.testing.assert_array_equal(ob.pio_value([0.0, 0.0, 1.0], [0.3, -0.2, -1.5]), [0.0, 0.0, -1.5])
    # the tangential components are fixed at 0 (a full diagonal), the normal one is zeroGradient (none)
    dg, bd, b = ob.face_contribution(ob.U_PRESSURE_INLET_OUTLET, True, 2.0, -0.5, [0.0, 0.0, 1.0], [0.3, -0.2, -1.5])
    assert dg == -0.5
    np.testing.assert_array_equal(bd, [2.5, 2.5, 0.0])
    np.testing.assert_array_equal(b, [0.0, 0.0, 0.0])              # refValue 0: nothing on the right-hand side of a planar face


def test_with_the_mask_all_zero_every_contribution_is_zero_gradients():
    rs = np.random.RandomState(5)
    for _ in range(20):
        n = ob.unit_normal(rs.standard_normal(3))
        uP, uv = rs.standard_normal(3), rs.standard_normal(3)
        gm, phi = rs.uniform(0.1, 2.0), rs.uniform(0.1, 2.0)
        zg = ob.face_contribution(ob.U_ZERO_GRADIENT, False, gm, phi, n, uP)
        for code in (ob.U_INLET_OUTLET, ob.U_PRESSURE_INLET_OUTLET):
            got = ob.face_contribution(code, False, gm, phi, n, uP, uv)
            assert got[0] == zg[0] == phi
            np.testing.assert_array_equal(got[1], zg[1]); np.testing.assert_array_equal(got[2], zg[2])
            np.testing.assert_array_equal(ob.boundary_value(code, False, n, uP, uv), uP)
        assert not zg[1].any() and not zg[2].any()


def test_an_inflow_face_of_inletOutlet_is_the_fixed_value_face():
    rs = np.random.RandomState(6)
    n = ob.unit_normal(rs.standard_normal(3))
    uP, uv = rs.standard_normal(3), rs.standard_normal(3)
    a = ob.face_contribution(ob.U_INLET_OUTLET, True, 1.3, -0.4, n, uP, uv)
    b = ob.face_contribution(ob.U_FIXED_VALUE, False, 1.3, -0.4, n, uP, uv)
    assert a[0] == b[0] == 1.3
    np.testing.assert_array_equal(a[2], b[2]); np.testing.assert_array_equal(a[2], (1.3 + 0.4) * uv)
    np.testing.assert_array_equal(ob.boundary_value(ob.U_INLET_OUTLET, True, n, uP, uv), uv)


def test_the_transform_form_is_consistent_with_its_boundary_value():
    """with the coefficients of an oblique inflow face the row reproduces the flux terms it restates: (dg + bd_q) U_P,q - b_q = phi U_b,q - gm (U_b,q - U_P,q)"""
    rs = np.random.RandomState(7)
    for _ in range(20):
        n = ob.unit_normal(rs.standard_normal(3))
        uP = rs.standard_normal(3)
        gm, phi = rs.uniform(0.1, 2.0), -rs.uniform(0.1, 2.0)
        dg, bd, b = ob.face_contribution(ob.U_PRESSURE_INLET_OUTLET, True, gm, phi, n, uP)
        ub = ob.pio_value(n, uP)
        np.testing.assert_allclose((dg + bd) * uP - b, phi * ub - gm * (ub - uP), rtol=0, atol=64 * np.finfo(float).eps * (gm - phi) * np.abs(uP).max())
        assert (bd >= 0).all()                                         # gm - phi > 0 on an inflow face: the added diagonal never weakens the row
        np.testing.assert_allclose(ob.pio_rAU_shift([gm], [phi], n[None]), [bd.mean()], rtol=4 * np.finfo(float).eps)


def test_mask_and_stats():
    phi = np.array([-1.0, 2.0, -0.0, 0.0, -3.0, 4.0])
    openf = np.array([1, 1, 1, 1, 0, 0])
    np.testing.assert_array_equal(ob.inflow_mask(phi, openf), [1, 0, 0, 0, 0, 0])     # (-0.0 < 0 is false; a closed face is never flagged)
    assert ob.stats(phi, openf) == (1, -1.0, 2.0)
