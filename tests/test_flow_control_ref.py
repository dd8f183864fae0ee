"""The long-double restatement of flow-rate control (flow_control_ref.py) checked on its own, without a GPU: the closed form of the plane channel against a direct
time march of the same discrete equations under the controller, and the relaxation recurrence of one correction."""
import numpy as np
import pytest

import flow_control_ref as fr

LD = fr.LD


def test_profile_solves_the_discrete_equations_and_tends_to_poiseuille():
    H, nu, G = 0.7, 0.03, 2.5
    err = []
    for ny in (6, 12, 24):
        u = fr.channel_profile(ny, H, nu, G)
        dy = LD(H) / ny
        up = np.concatenate([[-u[0]], u, [-u[-1]]])                # mirror values: the wall face's gradient (0 - u) / (dy / 2) = (u_ghost - u) / dy with u_ghost = -u
        res = LD(nu) * (up[2:] - 2 * up[1:-1] + up[:-2]) / (dy * dy) + LD(G)
        assert np.abs(res).max() < 1e-15 * G
        assert np.allclose(np.asarray(u, float), np.asarray(u[::-1], float), rtol=1e-14) and u.min() > 0
        err.append(abs(float(u.mean()) - G * H * H / (12 * nu)))
    assert err[1] < 0.3 * err[0] and err[2] < 0.3 * err[1]               # second order in dy
    assert float(fr.channel_gradient(6, H, nu, 0.1)) == pytest.approx(0.1 / float(fr.channel_profile(6, H, nu).mean()), rel=1e-15)


def test_controller_on_the_discrete_channel_reaches_the_closed_form():
    """implicit Euler on the 1-D channel with the three events of the control per step (assembly: gradP0 += dGradP; the source; after the solve: dGradP assigned, U
    corrected with rAU = 1 / A): its gradient converges to |Ubar| / c"""
    ny, H, nu, dt, ubar_vec, r = 6, 1.0, 1.0, 0.01, (0.1335, 0, 0), 1.0
    dy = H / ny
    A = np.zeros((ny, ny))
    for j in range(ny):
        for nb in (j - 1, j + 1):
            if 0 <= nb < ny:
                A[j, j] += nu / dy ** 2; A[j, nb] -= nu / dy ** 2
            else:
                A[j, j] += 2 * nu / dy ** 2
    M = np.eye(ny) / dt + A
    rAU = 1.0 / np.diag(M)
    V = np.full(ny, dy)
    st = fr.State(0.0)
    u = np.zeros(ny)
    steps, decay = fr.viscous_steps(H, nu, dt)
    assert steps == 234 and decay < 1e-10
    for _ in range(steps):
        g0 = st.assemble()
        u = np.linalg.solve(M, u / dt + g0)
        U3 = np.stack([u, 0 * u, 0 * u], axis=1)
        c = fr.correction(U3, rAU, V, ubar_vec, r)
        st.correct(c["dGradP"])
        u = np.asarray(c["U"][:, 0], float)
        assert float(fr.bulk(np.stack([u, 0 * u, 0 * u], axis=1), V, (1, 0, 0))[0]) == pytest.approx(0.1335, rel=1e-14)
    assert st.corrections == steps
    assert st.gradient == pytest.approx(float(fr.channel_gradient(ny, H, nu, 0.1335)), rel=100 * decay)


@pytest.mark.parametrize("r", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("weighted", [False, True])
def test_relaxation_recurrence(r, weighted):
    """ubar_after = ubar + r (|Ubar| - ubar), with or without the void-fraction weights, for any direction"""
    rs = np.random.RandomState(3)
    n = 294
    U = rs.standard_normal((n, 3)); rAU = 1e-3 * (1 + rs.rand(n)); V = 1e-6 * (1 + rs.rand(n))
    w = 0.5 + 0.5 * rs.rand(n) if weighted else None
    ubar_vec = (0.06, -0.02, 0.08)
    d, mag = fr.direction(ubar_vec)
    assert abs(np.dot(d, d) - 1) < 4e-16
    c = fr.correction(U, rAU, V, ubar_vec, r, w)
    after, scale = fr.bulk(c["U"], V, d, w)
    want = c["ubar"] + LD(r) * (LD(mag) - c["ubar"])
    assert abs(after - want) < 64 * n * float(np.finfo(LD).eps) * max(float(scale), mag)
    assert c["kappa"] > 1.0                                              # (U has both signs)


def test_state_bookkeeping():
    st = fr.State(0.25)
    assert st.gradient == 0.25 and st.assemble() == 0.25
    st.correct(0.5); st.correct(0.125)                                   # assigned, not accumulated
    assert (st.gradP0, st.dGradP, st.gradient, st.corrections) == (0.25, 0.125, 0.375, 2)
    assert st.assemble() == 0.375 and st.dGradP == 0.0 and st.gradient == 0.375
