"""numpy restatement of the solid-phase statistics (include/foamyade_hip.h, fy_solver_set_solid_statistics), written from the definitions: the eight per-cell sums
from a batch's records and its stencils as stencils_of(batch) returns them, and the fields from sums and cell volumes -- every bracket below is one IEEE double
operation, in the order k_solid_stats_cells performs it.  Nothing here is in the reference or in OpenFOAM: the definitions are this library's own."""
import numpy as np

U53 = 2.0 ** -53


def point_stencils(cell):
    """point-force mode: (k, ids, w) of the containing cell (-1: outside) with weight 1"""
    cell = np.asarray(cell)
    return (cell >= 0).astype(np.int32), cell.reshape(-1, 1), (cell >= 0).astype(float).reshape(-1, 1)


def terms(rec, k, ids, w, Tp=None):
    """the (particle, cell) pairs of one batch: cells [m] and the eight terms [m, 8] each pair adds to its cell.  A particle with k == 0 has no pair; an id < 0 is no
    slot.  Tp: per particle, a number, or None (no heat transfer: the s7 terms are 0)"""
    rec = np.asarray(rec, float).reshape(-1, 10)
    ids, w, k = np.asarray(ids), np.asarray(w, float), np.asarray(k)
    valid = (ids >= 0) & (k > 0)[:, None]
    rows, cols = np.nonzero(valid)
    cells, ww = ids[rows, cols], w[rows, cols]
    d = 2.0 * rec[rows, 9]
    vp = np.pi * ((d * d) * d) / 6.0
    vx, vy, vz = rec[rows, 3], rec[rows, 4], rec[rows, 5]
    tp = np.zeros(rec.shape[0]) if Tp is None else np.broadcast_to(np.asarray(Tp, float), (rec.shape[0],))
    wv = ww * vp
    t = np.stack([ww, wv, wv * vx, wv * vy, wv * vz, wv * ((vx * vx + vy * vy) + vz * vz), ww * (d * d), wv * tp[rows]], axis=1)
    return cells, t


def moments(batches, Nc):
    """batches: [(rec, k, ids, w, Tp)] -> (S [Nc, 8], m [Nc], A [Nc, 8]): the sums over all batches, the number of terms per cell and the sums of the terms' magnitudes"""
    S, A, m = np.zeros((Nc, 8)), np.zeros((Nc, 8)), np.zeros(Nc)
    for rec, k, ids, w, Tp in batches:
        cells, t = terms(rec, k, ids, w, Tp)
        np.add.at(S, cells, t)
        np.add.at(A, cells, np.abs(t))
        np.add.at(m, cells, 1.0)
    return S, m, A


def sum_bound(m, A):
    """a sum of m terms in any order, each formed by at most three roundings, differs from the exact sum by at most (m + 3) 2^-53 sum |term|"""
    return (m[:, None] + 3.0) * U53 * A


def fields(S, V, thermal=False):
    """the fields from the sums S [Nc, 8] and the cell volumes V [Nc], in the specified operation order; zeros where s1 == 0"""
    S, V = np.asarray(S, float).reshape(-1, 8), np.asarray(V, float)
    has = S[:, 1] != 0.0
    s1 = np.where(has, S[:, 1], 1.0)
    z = lambda x: np.where(has, x, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = S[:, 2:5] / s1[:, None]
        ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
        out = dict(nParticle=z(S[:, 0] / V), solidFraction=z(S[:, 1] / V), uSolid=np.where(has[:, None], u, 0.0),
                   granularTemperature=z(np.maximum(0.0, ((S[:, 5] / s1) - ((ux * ux + uy * uy) + uz * uz)) / 3.0)),
                   dSauter=z(((6.0 / np.pi) * S[:, 1]) / np.where(has, S[:, 6], 1.0)))
        if thermal:
            out["TParticle"] = z(S[:, 7] / s1)
    return out


def theta_bound(S, m, A):
    """how far granularTemperature can lie from the exact moments' value through the rounding of s1 .. s5 (bound 1 on each) and of the formula's own operations: with
    e_j the relative bound of s_j's positive-term sums and U_j = sum |terms of s_(2+j)| / s1 >= |u_j|, first order, doubled for the second-order terms left out"""
    with np.errstate(divide="ignore", invalid="ignore"):
        s1 = np.where(S[:, 1] != 0, S[:, 1], 1.0)
        e = (m + 3.0) * U53
        q = S[:, 5] / s1
        U2 = ((A[:, 2:5] / s1[:, None]) ** 2).sum(axis=1)
        return np.where(S[:, 1] != 0, 2.0 * ((2.0 * e + 2.0 * U53) * q + (4.0 * e + 6.0 * U53) * U2) / 3.0, 0.0)
