"""numpy restatement of the thermal loop (fy_thermal_desc.particle_cp, beta, T_ref), written from the formulas -- not from the kernels -- on top of
tests/heat_transfer_ref.py (nusselt, pass_a, pass_b):

    m_p c_pp dTp/dt = q_p,   m_p = rho_particle (4/3) pi r^3,   backward Euler for the coupled particle-fluid pair
    r_p = dt hA_p / (m_p c_pp),   hA'_p = hA_p / (1 + r_p)
    pass A: Sp_c += w hA',  Su_c += w hA' Tp^n          pass B: q_p = hA' (sum w T_c^{n+1} - Tp^n),  Tp^{n+1} = Tp^n + dt q_p / (m_p c_pp)
    buoyancy: a_c = (-beta (T_c - T_ref)) g

Eliminating Tp^{n+1}: m c (Tp^{n+1} - Tp^n) = dt hA (T_f^{n+1} - Tp^{n+1}).  Stencil layout as in heat_transfer_ref: rows (n, K), ids -1 / weights 0 beyond a particle's entries."""
import numpy as np

import heat_transfer_ref as ht


def heat_capacity(rec, rho_particle, particle_cp):
    """m_p c_pp [J/K] per particle from the record's radius"""
    return rho_particle * (4.0 / 3.0) * np.pi * rec[:, 9] ** 3 * particle_cp


def damped(hA, dt, mc):
    """hA' = hA / (1 + r_p), r_p = dt hA / (m c)"""
    return hA / (1.0 + dt * hA / mc)


def scatter(hA, ids, w, Tp, Nc):
    """Sp [Nc] = sum w hA, Su [Nc] = sum w hA Tp over the valid stencil entries"""
    Tp = np.broadcast_to(np.asarray(Tp, float), hA.shape)
    Sp, Su = np.zeros(Nc), np.zeros(Nc)
    rows, cols = np.nonzero(ids >= 0)
    np.add.at(Sp, ids[rows, cols], w[rows, cols] * hA[rows])
    np.add.at(Su, ids[rows, cols], w[rows, cols] * hA[rows] * Tp[rows])
    return Sp, Su


def pass_a(law, rec, ids, w, U, alpha, Tp, nu, kappa, Pr, Nc, dt, mc):
    """(hA', Sp, Su): heat_transfer_ref.pass_a's hA damped per particle, and the scatter of the damped coefficient"""
    hA, _, _ = ht.pass_a(law, rec, ids, w, U, alpha, Tp, nu, kappa, Pr, Nc)
    hAp = damped(hA, dt, mc)
    Sp, Su = scatter(hAp, ids, w, Tp, Nc)
    return hAp, Sp, Su


def pass_b(hAp, ids, w, T, Tp, dt, mc):
    """(q, Tp^{n+1}): a particle without a stencil has q = 0 and keeps its Tp"""
    Tp = np.broadcast_to(np.asarray(Tp, float), hAp.shape)
    q = ht.pass_b(hAp, ids, w, T, Tp)
    return q, np.where((ids >= 0).any(axis=1), Tp + dt * q / mc, Tp)


def step_at_rest(hA, ids, w, T, Tp, dt, mc, C):
    """one step of the loop for a fluid at rest whose cells exchange no heat with each other: cell heat capacities C [J/K] (rho cp alpha V), the T equation is then
    C (T' - T) / dt = Su - Sp T' cell by cell.  Returns (T', Tp', q)"""
    hAp = damped(hA, dt, mc)
    Sp, Su = scatter(hAp, ids, w, Tp, T.size)
    Tn = (C * T + dt * Su) / (C + dt * Sp)
    q, Tpn = pass_b(hAp, ids, w, Tn, Tp, dt, mc)
    return Tn, Tpn, q


def two_body(T, Tp, hA, dt, C, mc, steps):
    """the closed recurrence of one particle in one cell: T' = (T + b Tp) / (1 + b), b = dt hA' / C, Tp' = Tp + dt hA' (T' - Tp) / (m c).  Returns the lists of T, Tp, q"""
    hAp = hA / (1.0 + dt * hA / mc)
    b = dt * hAp / C
    Ts, Tps, qs = [], [], []
    for _ in range(steps):
        T = (T + b * Tp) / (1.0 + b)
        q = hAp * (T - Tp)
        Tp = Tp + dt * q / mc
        Ts.append(T); Tps.append(Tp); qs.append(q)
    return Ts, Tps, qs


def buoyancy(T, beta, T_ref, g):
    """a [n][3] = (-beta (T - T_ref)) g, in this operation order"""
    return (-beta * (np.asarray(T, float) - T_ref))[:, None] * np.asarray(g, float)[None, :]
