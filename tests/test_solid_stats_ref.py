"""tests/solid_stats_ref.py held to its own known answers (CPU): the restatement the device's solid-phase statistics are compared with in tests/test_solid_stats.py."""
import numpy as np

import solid_stats_ref as ss

NC = 60


def stencils(n, seed, kmax=12, unlocated=0):
    """random stencils as stencils_of returns them: k slots of distinct cells with normalised weights, -1 / 0 beyond; the first `unlocated` particles have k = 0"""
    rs = np.random.RandomState(seed)
    k = rs.randint(1, kmax + 1, n).astype(np.int32)
    k[:unlocated] = 0
    ids = np.full((n, 16), -1, np.int32)
    w = np.zeros((n, 16))
    for i in range(n):
        ids[i, :k[i]] = rs.choice(NC, k[i], replace=False)
        x = rs.random_sample(k[i]) + 0.05
        w[i, :k[i]] = x / x.sum()
    return k, ids, w


def cloud(n, seed, radius=None):
    rs = np.random.RandomState(seed)
    rec = np.zeros((n, 10))
    rec[:, 0:3] = rs.random_sample((n, 3))
    rec[:, 3:6] = 0.3 * rs.standard_normal((n, 3))
    rec[:, 9] = radius if radius is not None else 1e-3 * (0.5 + rs.random_sample(n))
    return rec


def volumes(seed=1):
    return 1e-6 * (0.5 + np.random.RandomState(seed).random_sample(NC))


def test_uniform_velocity_has_no_granular_temperature():
    rec = cloud(400, 3)
    rec[:, 3:6] = (0.3, -1.7, 0.9)
    k, ids, w = stencils(400, 4)
    S, m, A = ss.moments([(rec, k, ids, w, None)], NC)
    f = ss.fields(S, volumes())
    bound = ss.theta_bound(S, m, A)
    print(f"granularTemperature max {f['granularTemperature'].max():.3e}, bound min {bound[m > 0].min():.3e} max {bound.max():.3e}")
    assert (m > 0).all() and (f["granularTemperature"] <= bound).all()
    assert np.abs(f["uSolid"] - np.array([0.3, -1.7, 0.9])).max() <= 1e-13


def test_monodisperse_cloud_has_its_diameter_as_dsauter():
    r = 0.7e-3
    rec = cloud(400, 5, radius=r)
    k, ids, w = stencils(400, 6)
    S, m, A = ss.moments([(rec, k, ids, w, None)], NC)
    f = ss.fields(S, volumes())
    d = 2.0 * r
    # s1 / s6 = (pi d^3 / 6) sum w / (d^2 sum w): the two sums carry bound 1 each, the formula four more roundings
    tol = (2.0 * (m + 3.0) + 6.0) * ss.U53 * d
    assert (np.abs(f["dSauter"] - d) <= tol).all() and (m > 0).all()


def test_opposite_pairs_have_no_mean_velocity_and_a_third_of_u_squared():
    n = 300
    k, ids, w = stencils(n, 8)
    rec = cloud(n, 9)
    u = np.array([0.4, -0.25, 1.1])
    a, b = rec.copy(), rec.copy()
    a[:, 3:6], b[:, 3:6] = u, -u
    S, m, A = ss.moments([(a, k, ids, w, None), (b, k, ids, w, None)], NC)
    f = ss.fields(S, volumes())
    touched = m > 0
    assert touched.all()
    # the +u and -u terms are exact negatives of each other, but numpy adds them in two passes: |sum| <= bound 1
    assert (np.abs(S[:, 2:5]) <= ss.sum_bound(m, A)[:, 2:5]).all()
    u2 = (u * u).sum()
    assert (np.abs(f["granularTemperature"] - u2 / 3.0) <= ss.theta_bound(S, m, A) + 4 * ss.U53 * u2).all()
    assert np.abs(f["uSolid"]).max() <= 1e-13


def test_totals_count_the_located_particles_and_their_volume():
    n, out = 500, 37
    rec = cloud(n, 11)
    k, ids, w = stencils(n, 12, unlocated=out)
    ids[:out, :3] = 5; w[:out, :3] = 1.0 / 3.0               # rows of an unlocated particle may hold anything: k == 0 decides
    Tp = 300.0 + np.arange(n)
    S, m, A = ss.moments([(rec[:200], k[:200], ids[:200], w[:200], Tp[:200]), (rec[200:], k[200:], ids[200:], w[200:], Tp[200:])], NC)
    d = 2.0 * rec[out:, 9]
    vp = np.pi * d ** 3 / 6.0
    pairs = m.sum()
    assert abs(S[:, 0].sum() - (n - out)) <= (pairs + 3) * ss.U53 * (n - out)
    assert abs(S[:, 1].sum() - vp.sum()) <= (pairs + 3) * ss.U53 * vp.sum()
    f = ss.fields(S, volumes(), thermal=True)
    assert f["TParticle"].min() >= Tp[out] - 1e-9 and f["TParticle"].max() <= Tp[-1] + 1e-9
    assert "TParticle" not in ss.fields(S, volumes())
    S0 = ss.moments([(rec, k, ids, w, None)], NC)[0]
    assert (S0[:, 7] == 0.0).all()


def test_untouched_cells_are_zero_and_point_stencils_have_weight_one():
    cell = np.array([3, 3, -1, 7, 3])
    k, ids, w = ss.point_stencils(cell)
    rec = cloud(5, 13)
    S, m, A = ss.moments([(rec, k, ids, w, 350.0)], NC)
    assert m[3] == 3 and m[7] == 1 and m.sum() == 4 and S[3, 0] == 3.0 and S[7, 0] == 1.0
    f = ss.fields(S, volumes(), thermal=True)
    for nm, x in f.items():
        assert (x[m == 0] == 0.0).all(), nm
    assert abs(f["TParticle"][7] - 350.0) <= 1e-12 * 350.0 and abs(f["dSauter"][7] - 2.0 * rec[3, 9]) <= 1e-15
