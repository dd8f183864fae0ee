"""numpy restatement of the selectable drag closures (fy_set_drag_law) and the Saffman-Mei lift (FY_FORCE_SAFFMAN_MEI_LIFT), written from the
formulas of DESIGN.md section 3 "force laws" -- not from the kernels -- plus the bookkeeping around them that FoamYade.C fixes (what is interpolated
with which weights, what is scattered back into which field), so that a test can rebuild forces, uSourceDrag and uSource from the stencils the library
reports.  Notation: eps = interpolated alpha_f, phi = max(1 - eps, 0), m = |u_r|, Re = small + m d / nu."""
import numpy as np

SMALL = 1e-9                                         # FoamYade.H:85
REFERENCE, DI_FELICE, KOCH_HILL, BEETSTRA, SCHILLER_NAUMANN = 0, 1, 2, 3, 4
ADDED_MASS, GAUSSIAN_TORQUE, SAFFMAN_MEI_LIFT = 1, 2, 4


def drag_K(law, eps, m, d, rho, nu):
    """(K, K phi): the coefficient per unit solid volume -- force = pv K u_r -- and what is scattered into uSourceDrag / uSource"""
    phi = np.maximum(1.0 - eps, 0.0)
    Re = SMALL + m * d / nu
    with np.errstate(divide="ignore", invalid="ignore"):
        if law == REFERENCE:                         # FoamYade.C:366-382: Wen-Yu (without its 1/d, as shipped) above alpha_f = 0.8, Ergun below; divides by alpha_p
            ap = 1.0 - eps
            cd = np.where(Re < 1000, 24.0 / Re * (1.0 + 0.15 * Re ** 0.687), 0.44)
            wen_yu = 0.75 * cd * eps * ap * rho * m * eps ** -2.65
            ergun = 150.0 * (ap * ap / eps) * (nu * rho / (d * d)) + 1.75 * ap * rho * (1.0 / d) * m
            beta = np.where(eps > 0.8, wen_yu, ergun)
            return beta / ap, beta
        if law == DI_FELICE:
            Re_e = eps * Re
            Cd = (0.63 + 4.8 / np.sqrt(Re_e)) ** 2
            chi = 3.7 - 0.65 * np.exp(-0.5 * (1.5 - np.log10(Re_e)) ** 2)
            K = 0.75 * Cd * rho * m * eps ** (2.0 - chi) / d
        elif law == KOCH_HILL:
            Re_h = 0.5 * eps * Re
            plnp = np.where(phi > 0, phi * np.log(np.where(phi > 0, phi, 1.0)), 0.0)
            dilute = (1.0 + 3.0 * np.sqrt(phi / 2.0) + (135.0 / 64.0) * plnp + 16.14 * phi) / (1.0 + 0.681 * phi - 8.48 * phi ** 2 + 8.16 * phi ** 3)
            F0 = np.where(phi < 0.4, dilute, 10.0 * phi / eps ** 3)
            F3 = 0.0673 + 0.212 * phi + 0.0232 / eps ** 5
            K = 18.0 * nu * rho * eps ** 2 / d ** 2 * (F0 + 0.5 * F3 * Re_h)
        elif law == BEETSTRA:
            Re_e = eps * Re
            F = (10.0 * phi / eps ** 2 + eps ** 2 * (1.0 + 1.5 * np.sqrt(phi))
                 + (0.413 * Re_e / (24.0 * eps ** 2)) * ((1.0 / eps + 3.0 * eps * phi + 8.4 * Re_e ** -0.343) / (1.0 + 10.0 ** (3.0 * phi) * Re_e ** (-(1.0 + 4.0 * phi) / 2.0))))
            K = 18.0 * nu * rho * eps / d ** 2 * F
        else:
            raise ValueError(law)
    return K, K * phi


def schiller_naumann_factor(Re):
    return np.where(Re < 1000, 1.0 + 0.15 * Re ** 0.687, 0.44 * Re / 24.0)


def saffman_mei(ur, omega, d, pv, rho, nu):
    """F_L = rho pv Cl (u_r x omega) per particle"""
    m = np.linalg.norm(ur, axis=1)
    Re_p = m * d / nu
    Re_w = np.linalg.norm(omega, axis=1) * d * d / nu
    b = 0.5 * Re_w / (Re_p + SMALL)
    a = 0.3314 * np.sqrt(b)
    f = np.where(Re_p < 40, (1.0 - a) * np.exp(-0.1 * Re_p) + a, 0.0524 * np.sqrt(b * Re_p))
    Cl = 3.0 / (2.0 * np.pi * np.sqrt(Re_w + SMALL)) * 6.46 * f
    return (rho * pv * Cl)[:, None] * np.cross(ur, omega)


def curl(vGrad):
    """vorticity from grad U stored xx xy xz yx yy yz zx zy zz with G_ij = d_i U_j (calcHydroTorque, FoamYade.C:472-474)"""
    return np.stack([vGrad[:, 5] - vGrad[:, 7], vGrad[:, 6] - vGrad[:, 2], vGrad[:, 3] - vGrad[:, 1]], axis=1)


def deposit(rec, ids, w, V, alpha, uParticle):
    """setCellVolFraction for one batch (FoamYade.C:318-328): the cells its stencils touch get alpha = max(1 - sum pVol w / V, 0.1) and
    uParticle = sum pVol w v / V; alpha and uParticle are updated in place"""
    valid = ids >= 0
    volp = np.pi * (2.0 * rec[:, 9]) ** 3 / 6.0
    pvol = np.zeros_like(V); up = np.zeros((V.size, 3))
    rows = np.nonzero(valid)[0]
    cells = ids[valid]
    ww = w[valid] * volp[rows]
    np.add.at(pvol, cells, ww)
    np.add.at(up, cells, ww[:, None] * rec[rows, 3:6])
    touched = np.zeros(V.size, bool); touched[cells] = True
    alpha[touched] = np.maximum(1.0 - pvol[touched] / V[touched], 0.10)
    uParticle[touched] = up[touched] / V[touched, None]


def gaussian_batch(law, models, rec, ids, w, fields, alpha, uParticle, V, rhoF, rhoP, nu, dt):
    """hydroDragForce + archimedesForce (+ the opt-in models) and their back-scatter for one batch (FoamYade.C:354-389, 392-435, 465-479) with the drag
    closure `law`.  ids / w: the (n, 16) stencil rows, -1 / 0 beyond each particle's entries.  Returns (force [n, 6], uSourceDrag increment [Nc], uSource
    increment [Nc, 3], diagnostics dict with eps and Re per particle)"""
    n, Nc = rec.shape[0], V.size
    valid = ids >= 0
    k = valid.sum(axis=1)
    loc = k > 0
    idc = np.where(valid, ids, 0)
    wz = np.where(valid, w, 0.0)
    interp = lambda field: np.einsum("nk,nk...->n...", wz, field[idc])
    d = 2.0 * rec[:, 9]
    volp = np.pi * d ** 3 / 6.0
    pv = wz.sum(axis=1) * volp
    uf, eps = interp(fields["U"]), interp(alpha)
    A = 2.0 * nu * fields["divT"] * rhoF - fields["gradP"]                  # archimedesForce FoamYade.C:416-426, both terms share the weights
    ur = uf - rec[:, 3:6]
    m = np.linalg.norm(ur, axis=1)
    safe = lambda x, fill: np.where(loc, x, fill)
    K, Kphi = drag_K(law, safe(eps, 0.5), m, safe(d, 1.0), rhoF, nu)
    F = np.zeros((n, 6))
    b = pv[:, None] * interp(A)
    F[:, :3] = (pv * K)[:, None] * ur + b
    if models & GAUSSIAN_TORQUE:                                             # FoamYade.C:477-478
        F[:, 3:] = (np.pi * d ** 3)[:, None] * (interp(curl(fields["vGrad"])) - rec[:, 6:9]) * nu * rhoF
    if models & ADDED_MASS:                                                  # FoamYade.C:396-404
        am = (pv / np.maximum(k, 1))[:, None] * (interp(fields["ddtU"]) - rec[:, 3:6] / dt) * rhoP
        F[:, :3] += am; b = b + am
    if models & SAFFMAN_MEI_LIFT:
        fl = saffman_mei(ur, interp(curl(fields["vGrad"])), safe(d, 1.0), pv, rhoF, nu)
        F[:, :3] += fl; b = b + fl
    F[~loc] = 0.0
    D = np.zeros(Nc); S = np.zeros((Nc, 3))
    rows, cols = np.nonzero(valid)
    cells = ids[rows, cols]
    np.add.at(D, cells, -Kphi[rows] * w[rows, cols] / rhoF)                  # FoamYade.C:385
    np.add.at(S, cells, -b[rows] * (w[rows, cols] / (V[cells] * rhoF))[:, None])      # FoamYade.C:433, 406-411
    S += uParticle * D[:, None]                                              # FoamYade.C:386
    return F, D, S, dict(eps=eps[loc], Re=(SMALL + m * d / nu)[loc], located=loc)


def point_batch(law, rec, cell, U, V, rhoF, nu):
    """stokesDragForce (FoamYade.C:437-444), with Schiller-Naumann's factor for law 4, for records whose containing cell is `cell` (-1: outside).
    Returns (drag [n, 3], uSource increment [Nc, 3], Re of the located particles)"""
    inside = cell >= 0
    c = np.where(inside, cell, 0)
    d = 2.0 * rec[:, 9]
    ur = U[c] - rec[:, 3:6]
    Re = SMALL + np.linalg.norm(ur, axis=1) * d / nu
    f = schiller_naumann_factor(Re) if law == SCHILLER_NAUMANN else np.ones_like(Re)
    F = (3.0 * np.pi * d * nu * rhoF * f)[:, None] * ur
    F[~inside] = 0.0
    S = np.zeros((V.size, 3))
    np.add.at(S, c[inside], -F[inside] / (V[c[inside]] * rhoF)[:, None])
    return F, S, Re[inside]
