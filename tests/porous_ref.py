"""numpy restatement of the porous zones' operator (DESIGN_FV.md "Porous resistance"; csrc/porous.hpp): per component q of a zone's cell
    C_q = nu d_q + (0.5 |U|) f_q,   |U| = sqrt((u0^2 + u1^2) + u2^2)
the row additions a V C_q on the momentum matrix's per-component diagonal, the resistance force F_q = sum a V C_q U_q, and fvMatrix::relax's dominance test with the
porous part's component maximum.  Every bracket is one IEEE operation, as the kernels form them (-ffp-contract=off)."""
import numpy as np

EPS = np.finfo(np.float64).eps


def coeff(nu, d, f, U):
    """C [n][3] of cells with velocities U [n][3] in a zone with coefficients d [3] (1/m^2) and f [3] (1/m)"""
    U = np.asarray(U, np.float64).reshape(-1, 3)
    d = np.asarray(d, np.float64); f = np.asarray(f, np.float64)
    hm = 0.5 * np.sqrt((U[:, 0] * U[:, 0] + U[:, 1] * U[:, 1]) + U[:, 2] * U[:, 2])
    return nu * d[None, :] + hm[:, None] * f[None, :]


def row_additions(a, V, nu, d, f, U):
    """what the per-component diagonal gains in the zone's cells: (a V) C_q, [n][3]; a = alpha (pimpleFoamYade) or 1 (icoFoamYade), V the cell volumes"""
    aV = np.asarray(a, np.float64) * np.asarray(V, np.float64)
    return aV[:, None] * coeff(nu, d, f, U)


def force(a, V, nu, d, f, U):
    """F [3] = sum over the zone's cells of a V C_q(U) U_q (per unit density)"""
    U = np.asarray(U, np.float64).reshape(-1, 3)
    return (row_additions(a, V, nu, d, f, U) * U).sum(axis=0)


def zone_map(n_cells, zones):
    """zone_of [n_cells]: 0 outside, 1 + index inside (the read-out "porousZone")"""
    z = np.zeros(n_cells)
    for q, o in enumerate(zones):
        z[np.asarray(o["cells"])] = q + 1
    return z


def diagonal_additions(n_cells, zones, a, V, nu, U):
    """the additions of every zone scattered to [n_cells][3] (zeros outside the zones)"""
    out = np.zeros((n_cells, 3))
    a = np.broadcast_to(np.asarray(a, np.float64), (n_cells,)); V = np.broadcast_to(np.asarray(V, np.float64), (n_cells,))
    U = np.asarray(U, np.float64).reshape(-1, 3)
    for o in zones:
        c = np.asarray(o["cells"])
        out[c] = row_additions(a[c], V[c], nu, o["d"], o["f"], U[c])
    return out


def relaxed(diag0, src0, U, offsum, bmax, bmin, pc, relax):
    """fvMatrix::relax as the assembly sweeps apply it: D = max(|(D0 + bmax) + max_q pc_q|, sum |offdiag|) / relax - bmin, source += (D - D0) U.
    diag0 / src0: the unrelaxed row; bmax / bmin: the component maximum / minimum of the boundary part (block: its sum / 0); pc [n][3]: the porous additions"""
    pm = pc.max(axis=1)
    t = diag0 + bmax
    t = np.where(pm > 0, t + pm, t)
    dn = np.maximum(np.abs(t), offsum) / relax - bmin
    return dn, src0 + (dn - diag0)[:, None] * np.asarray(U).reshape(-1, 3)
