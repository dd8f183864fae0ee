"""numpy restatement of the heat exchange (fy_thermal_desc), written from the formulas of DESIGN.md section 3 "heat exchange" and DESIGN_FV.md "T equation" --
not from the kernels: the two Nusselt laws, pass A (coefficients and the scatter of Sp / Su) and pass B (the particles' fluxes) on given stencils, and the fluid's
temperature equation assembled densely on a uniform or graded block from given phi, alpha, nut and old T, solved with numpy.linalg.solve.

Layouts are the library's: cell c = i + nx (j + ny k); face arrays phi_x [(nx + 1) ny nz], phi_y [nx (ny + 1) nz], phi_z [nx ny (nz + 1)], oriented along +axis;
sides XMIN, XMAX, YMIN, YMAX, ZMIN, ZMAX = 0 .. 5; stencil rows (n, K) with ids -1 / weights 0 beyond a particle's entries."""
import numpy as np

SMALL = 1e-9                                         # FoamYade.H:85, as tests/force_laws_ref.py forms Re
RANZ_MARSHALL, GUNN = 0, 1
ZERO_GRADIENT, FIXED_VALUE = 0, 1
LINEAR, UPWIND = 0, 1


def prandtl(nu, rho, cp, kappa):
    return nu * rho * cp / kappa


def nusselt(law, eps, Re, Pr):
    p3 = Pr ** (1.0 / 3.0)
    if law == RANZ_MARSHALL:
        return 2.0 + 0.6 * np.sqrt(Re) * p3
    if law == GUNN:
        Res = eps * Re
        return (7.0 - 10.0 * eps + 5.0 * eps ** 2) * (1.0 + 0.7 * Res ** 0.2 * p3) + (1.33 - 2.4 * eps + 1.2 * eps ** 2) * Res ** 0.7 * p3
    raise ValueError(law)


def point_stencils(cell):
    """point-force mode: the containing cell (-1: outside) with weight 1"""
    cell = np.asarray(cell)
    return cell.reshape(-1, 1), (cell >= 0).astype(float).reshape(-1, 1)


def pass_a(law, rec, ids, w, U, alpha, Tp, nu, kappa, Pr, Nc):
    """hA [n] (0 for a particle without a stencil), Sp [Nc] = sum w hA, Su [Nc] = sum w hA Tp.  alpha = None: 1 everywhere (point-force mode)"""
    valid = ids >= 0
    loc = valid.any(axis=1)
    idc = np.where(valid, ids, 0)
    wz = np.where(valid, w, 0.0)
    eps = np.ones(rec.shape[0]) if alpha is None else np.einsum("nk,nk->n", wz, alpha[idc])
    uf = np.einsum("nk,nkc->nc", wz, U[idc])
    d = 2.0 * rec[:, 9]
    m = np.linalg.norm(uf - rec[:, 3:6], axis=1)
    Re = SMALL + m * d / nu
    hA = np.where(loc, nusselt(law, np.where(loc, eps, 1.0), Re, Pr) * kappa * np.pi * d, 0.0)
    Tp = np.broadcast_to(np.asarray(Tp, float), (rec.shape[0],))
    Sp, Su = np.zeros(Nc), np.zeros(Nc)
    rows, cols = np.nonzero(valid)
    cells = ids[rows, cols]
    np.add.at(Sp, cells, w[rows, cols] * hA[rows])
    np.add.at(Su, cells, w[rows, cols] * hA[rows] * Tp[rows])
    return hA, Sp, Su


def pass_b(hA, ids, w, T, Tp):
    """q [n] = hA (sum w T - Tp): W into each particle"""
    valid = ids >= 0
    Tf = np.einsum("nk,nk->n", np.where(valid, w, 0.0), T[np.where(valid, ids, 0)])
    return np.where(valid.any(axis=1), hA * (Tf - np.broadcast_to(np.asarray(Tp, float), hA.shape)), 0.0)


def block_sizes(nx, ny, nz, dx=None, grading=None):
    """per-axis cell sizes of a uniform (dx) or graded (hx, hy, hz) block"""
    if grading is not None:
        return [np.asarray(a, float) for a in grading]
    return [np.full(n, float(dx)) for n in (nx, ny, nz)]


def cell_volumes(h):
    return (h[2][:, None, None] * h[1][None, :, None] * h[0][None, None, :]).ravel()


def assemble_T(h, dt, phi, alpha, nut, Told, D, Prt, bc, val, scheme, Sp=None, Su=None, rho_cp=1.0, nut_b=None):
    """dense (A, b) of
        alpha V (T - Told) / dt + sum_f F_f T_f - T sum_f F_f - sum_f alpha_f Deff_f |S_f| / |d_f| (T_N - T) = (Su - Sp T) / rho_cp
    F_f = alpha_f phi_f outward, alpha_f and Deff_f = D + nut / Prt the linear interpolates (alpha_f = 1 on a boundary face, Deff_b = D + nut_b / Prt with nut_b the
    cell's value unless nut_b[side] gives one), T_f linear or upwind; fixedValue side: half-cell distance and F_b T_b; zeroGradient side: T_b = T.
    h = [hx, hy, hz]; phi = (phi_x, phi_y, phi_z); alpha, nut = None: 1 and 0"""
    nx, ny, nz = (a.size for a in h)
    N = nx * ny * nz
    n3 = (nx, ny, nz)
    alpha = np.ones(N) if alpha is None else np.asarray(alpha, float)
    nut = np.zeros(N) if nut is None else np.asarray(nut, float)
    Deff = D + nut / Prt
    fshape = [(nz, ny, nx + 1), (nz, ny + 1, nx), (nz + 1, ny, nx)]
    ph = [np.asarray(phi[d], float).reshape(fshape[d]) for d in range(3)]
    V = cell_volumes(h)
    A = np.zeros((N, N)); b = np.zeros(N)
    stride = (1, nx, nx * ny)
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                c = i + nx * (j + ny * k)
                ijk = (i, j, k)
                A[c, c] += alpha[c] * V[c] / dt
                b[c] += alpha[c] * V[c] * Told[c] / dt
                sumF = 0.0
                for d in range(3):
                    q = ijk[d]
                    area = V[c] / h[d][q]
                    for s in (0, 1):
                        fi = [k, j, i]                       # index into ph[d] (z, y, x order), the face on side s
                        fi[2 - d] += s
                        pv = (1.0 if s else -1.0) * ph[d][tuple(fi)]
                        side = 2 * d + s
                        if (q == 0 and s == 0) or (q == n3[d] - 1 and s == 1):
                            F = pv                           # alpha_f = 1 on the boundary
                            sumF += F
                            if bc[side] == FIXED_VALUE:
                                nb = nut[c] if nut_b is None or nut_b[side] is None else nut_b[side]
                                gam = (D + nb / Prt) * area / (0.5 * h[d][q])
                                A[c, c] += gam
                                b[c] += (gam - F) * val[side]
                            else:
                                A[c, c] += F
                        else:
                            qn = q + (1 if s else -1)
                            cn = c + (stride[d] if s else -stride[d])
                            wP = h[d][qn] / (h[d][q] + h[d][qn])          # the own cell's linear weight: distance face - neighbour centre over centre distance
                            af = wP * alpha[c] + (1.0 - wP) * alpha[cn]
                            df = wP * Deff[c] + (1.0 - wP) * Deff[cn]
                            gam = af * df * area / (0.5 * (h[d][q] + h[d][qn]))
                            F = af * pv
                            sumF += F
                            if scheme == UPWIND:
                                cP, cN = max(F, 0.0), min(F, 0.0)
                            else:
                                cP, cN = wP * F, (1.0 - wP) * F
                            A[c, c] += cP + gam
                            A[c, cn] += cN - gam
                A[c, c] -= sumF
    if Sp is not None:
        A[np.arange(N), np.arange(N)] += np.asarray(Sp) / rho_cp
        b += np.asarray(Su) / rho_cp
    return A, b


def solve_T(*args, **kw):
    A, b = assemble_T(*args, **kw)
    return np.linalg.solve(A, b)


def residual_bound(A, b, T):
    """what the equation's own residual on a given T implies for its distance from the exact solution: |A^-1 (b - A T)|_inf"""
    return np.abs(np.linalg.solve(A, b - A @ T)).max()
