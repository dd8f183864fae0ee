"""mesh.findCell on a general polyhedral mesh, restated in plain numpy from the mesh dictionary alone (points, face_offsets, face_points, owner, neighbour) -- not
from the solver's geometry and not from the kernel.  OpenFOAM's default decomposition (polyMesh::CELL_TETS) splits every face into triangles that both of its cells
share, so the tetrahedra (cell centre, p0, p_i, p_i+1) tile the mesh without gaps or overlaps, warped faces included.  Here: the fan of each face's point list as
stored, the apex at the cell centre the caller hands in (the restatement's, oracle.LduSolver(...).geometry("C")), barycentric coordinates in np.longdouble.

    cells_of(x, tol) = the cells with a tetrahedron whose four barycentric coordinates are all >= -tol

An empty set: the point is outside the mesh.  More than one cell: the point is on a shared triangle, edge or vertex, and any member is right.  Cyclic halves are
boundary faces, as findCell has them.  Star-shaped cells (every face triangle seen from the centre) are assumed, as by the decomposition itself.

Also here: the meshes and the point sets of tests/test_ldu_find_cell.py, so that tests/test_find_cell_ref.py can hold them to properties without a device."""
import numpy as np

import poly_meshes as pm

LD = np.longdouble
TOL = 1e-9


class FindCellRef:
    def __init__(self, mesh, centres):
        P = np.asarray(mesh["points"], LD)
        off, fp = np.asarray(mesh["face_offsets"]), np.asarray(mesh["face_points"])
        own, nei = np.asarray(mesh["owner"]), np.asarray(mesh["neighbour"])
        self.n_cells = int(mesh["n_cells"])
        self.C = np.asarray(centres, np.float64).reshape(-1, 3)
        assert self.C.shape[0] == self.n_cells
        cell, ia, ib, ic = [], [], [], []
        for f in range(len(own)):
            q = fp[off[f]:off[f + 1]]
            for c in ([own[f], nei[f]] if f < len(nei) else [own[f]]):
                for i in range(1, len(q) - 1):
                    cell.append(c); ia.append(q[0]); ib.append(q[i]); ic.append(q[i + 1])
        cell = np.asarray(cell)
        order = np.argsort(cell, kind="stable")
        self.tet_cell = cell[order]
        self.tet_off = np.searchsorted(self.tet_cell, np.arange(self.n_cells + 1))          # cell -> its tetrahedra [tet_off[c], tet_off[c + 1])
        apex = np.asarray(self.C, LD)[self.tet_cell]
        A, B, Cc = (P[np.asarray(v)[order]] - apex for v in (ia, ib, ic))
        D = np.einsum("tk,tk->t", A, np.cross(B, Cc))
        assert np.all(D != 0), "a flat tetrahedron: a face triangle in a plane through its cell's centre"
        # x = apex + mu_a A + mu_b B + mu_c Cc: the rows of the inverse of [A B Cc]
        self.apex = apex
        self.rows = np.stack([np.cross(B, Cc), np.cross(Cc, A), np.cross(A, B)], axis=1) / D[:, None, None]
        # the ball round each centre that holds the cell's tetrahedra (float64, used to choose candidates only; widened below)
        r2 = np.zeros(self.n_cells)
        for V in (A, B, Cc):
            np.maximum.at(r2, self.tet_cell, np.einsum("tk,tk->t", V, V).astype(np.float64))
        self.r2 = r2

    def pairs(self, X, chunk=512):
        """for points X [n, 3]: (point index, cell, m) for every candidate cell of every point, m = the largest over the cell's tetrahedra of the smallest of the four
        barycentric coordinates (np.longdouble).  A cell that is no candidate (the point outside the ball round its centre) cannot hold the point"""
        X = np.asarray(X, np.float64).reshape(-1, 3)
        out_i, out_c, out_m = [], [], []
        ntet = np.diff(self.tet_off)
        for s in range(0, X.shape[0], chunk):
            x = X[s:s + chunk]
            with np.errstate(invalid="ignore", over="ignore"):
                d2 = ((x[:, None, :] - self.C[None, :, :]) ** 2).sum(axis=2)
                pi, ci = np.nonzero(d2 <= self.r2[None, :] * (1 + 1e-6) + 1e-300)
            if pi.size == 0:
                continue
            rep = ntet[ci]
            seg = np.repeat(np.arange(pi.size), rep)                                         # the (point, cell) pair of each (point, tetrahedron) row
            first = np.concatenate([[0], np.cumsum(rep)[:-1]])
            t = np.repeat(self.tet_off[ci] - first, rep) + np.arange(rep.sum())
            r = np.asarray(x, LD)[pi[seg]] - self.apex[t]
            mu = np.einsum("tjk,tk->tj", self.rows[t], r)
            lam = np.concatenate([mu, (LD(1) - mu.sum(axis=1))[:, None]], axis=1).min(axis=1)
            m = np.full(pi.size, -np.inf, LD)
            np.maximum.at(m, seg, lam)
            out_i.append(pi + s); out_c.append(ci); out_m.append(m)
        if not out_i:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, LD)
        return np.concatenate(out_i), np.concatenate(out_c), np.concatenate(out_m)

    def cells_of(self, X, tol=TOL):
        """one set of cells per point"""
        X = np.asarray(X, np.float64).reshape(-1, 3)
        i, c, m = self.pairs(X)
        out = [set() for _ in range(X.shape[0])]
        for a, b in zip(i[m >= -tol], c[m >= -tol]):
            out[a].add(int(b))
        return out

    def classify(self, X, tol=TOL):
        """(pairs, n_admissible [n], decided_in [n], decided_out [n]): a point is decidedly inside with a cell at tolerance 0 (and so at tol), decidedly outside with
        none at tol, free in between"""
        X = np.asarray(X, np.float64).reshape(-1, 3)
        i, c, m = self.pairs(X)
        n_adm = np.bincount(i[m >= -tol], minlength=X.shape[0])
        n_strict = np.bincount(i[m >= 0], minlength=X.shape[0])
        return (i, c, m), n_adm, n_strict > 0, n_adm == 0

    def admissible(self, pairs, cells, n, tol=TOL):
        """[n] bool: cells[i] is in cells_of(x_i, tol)"""
        i, c, m = pairs
        ok = np.zeros(n, bool)
        hit = (m >= -tol) & (c == np.asarray(cells)[i])
        ok[i[hit]] = True
        return ok

    def nearest_centre(self, X):
        X = np.asarray(X, np.float64).reshape(-1, 3)
        out = np.zeros(X.shape[0], np.int64)
        for s in range(0, X.shape[0], 512):
            out[s:s + 512] = ((X[s:s + 512, None, :] - self.C[None, :, :]) ** 2).sum(axis=2).argmin(axis=1)
        return out


# ---- the meshes of tests/test_ldu_find_cell.py: name -> (mesh, warped)
def _cyclic():
    return pm.make_cyclic(pm.hex_block(8, 8, 8, (1.0, 1.0, 1.0), pm.wavy_periodic(0.025, (1.0, 1.0, 1.0)), renumber_seed=10), [(0, 1), (4, 5)])


MESHES = {
    "hex8_wavy": (lambda: pm.hex_block(8, 8, 8, vertex_map=pm.wavy(0.04), renumber_seed=12), True),
    "hex10_wavy": (lambda: pm.hex_block(10, 10, 10, vertex_map=pm.wavy(0.02), renumber_seed=8), True),
    "prisms_wavy": (lambda: pm.prism_block(6, 6, 4, vertex_map=pm.wavy(0.15 / 6)), True),
    "tets": (lambda: pm.tet_block(4, 4, 4), False),
    "tets_wavy": (lambda: pm.tet_block(4, 4, 4, vertex_map=pm.wavy(0.15 / 4)), True),
    "refined": (lambda: pm.refined_block(4, 4, 4, 2), False),
    "refined_wavy": (lambda: pm.refined_block(4, 4, 4, 2, vertex_map=pm.wavy(0.03)), True),
    "hex_sheared": (lambda: pm.hex_block(6, 5, 4, vertex_map=pm.shear(0.3, 0.2, 0.25)), False),
    "cyclic_wavy": (_cyclic, True),
}
U_BC = {"cyclic_wavy": [1, 1, 0, 0, 1, 1]}                  # (the cyclic halves: FY_BC_U_ZERO_GRADIENT, as test_cyclic_patches_match_the_restatement has them)


def faces_of(mesh):
    off, fp = np.asarray(mesh["face_offsets"]), np.asarray(mesh["face_points"])
    return [fp[off[f]:off[f + 1]] for f in range(len(off) - 1)]


def case_points(mesh, centres=None, seed=1):
    """about 6 000 points that ask findCell everything at once, from the mesh dictionary (and, for the cell-centre records, the centres): (X [n, 3], h).  h = the
    cube root of the bounding box's volume per cell, the unit of the offsets.
      uniform over the bounding box enlarged by 5 % (some outside);
      interior vertices, face centres (the mean of the face's points) and edge midpoints, exact and jittered by +-1e-12 h and +-1e-9 h per component; a few of each
        on the boundary (there the exact and the 1e-12 ones are undecided between the two tolerances: kept few);
      points on interior faces pushed up to 0.05 h off them (on warped cells: in a cell whose centre is not the nearest);
      points 1e-6 h inside and 1e-6 h outside boundary faces (the cyclic halves of a cyclic mesh among them);
      cell centres;
      one NaN record, one record 100 box lengths away"""
    rs = np.random.RandomState(seed)
    P = np.asarray(mesh["points"], np.float64)
    lo, hi = P.min(axis=0), P.max(axis=0)
    h = float(np.prod(hi - lo) / mesh["n_cells"]) ** (1.0 / 3.0)
    faces = faces_of(mesh)
    ni = len(mesh["neighbour"])
    on_boundary = np.zeros(P.shape[0], bool)
    for f in range(ni, len(faces)):
        on_boundary[faces[f]] = True
    fcentre = np.array([P[q].mean(axis=0) for q in faces])
    edges = {}
    for f, q in enumerate(faces):
        for a, b in zip(q, np.roll(q, -1)):
            key = (min(a, b), max(a, b))
            edges[key] = edges.get(key, False) or f >= ni
    ekeys = sorted(edges)
    emid = np.array([0.5 * (P[a] + P[b]) for a, b in ekeys])
    e_bnd = np.array([edges[k] for k in ekeys])

    def pick(A, n):
        return A[rs.choice(A.shape[0], min(n, A.shape[0]), replace=False)]

    groups = []
    for inner, bnd in ((P[~on_boundary], P[on_boundary]), (fcentre[:ni], fcentre[ni:]), (emid[~e_bnd], emid[e_bnd])):
        for A in (pick(inner, 380), pick(bnd, 8)):
            groups.append(A)
            for amp in (1e-12, 1e-9):
                groups.append(A + amp * h * rs.choice([-1.0, 1.0], A.shape))
    near = []                                                       # interior faces: a random point of the face's first triangle, pushed off it
    for f in rs.choice(ni, min(ni, 500), replace=False):
        a, b, c = P[faces[f][0]], P[faces[f][1]], P[faces[f][2]]
        w = rs.dirichlet((1.0, 1.0, 1.0))
        nrm = np.cross(b - a, c - a)
        near.append(w[0] * a + w[1] * b + w[2] * c + rs.uniform(-0.05, 0.05) * h * nrm / np.linalg.norm(nrm))
    groups.append(np.array(near))
    own = np.asarray(mesh["owner"])
    bsel = ni + rs.choice(len(faces) - ni, min(len(faces) - ni, 300), replace=False)
    if "patch_neighbour" in mesh:                                   # every cyclic half takes part
        cyc = [q for q, b in enumerate(mesh["patch_neighbour"]) if b >= 0]
        extra = np.concatenate([mesh["patch_start"][q] + rs.choice(mesh["patch_size"][q], 25, replace=False) for q in cyc])
        bsel = np.unique(np.concatenate([bsel, extra]))
    for sgn in (-1.0, 1.0):
        pts = []
        for f in bsel:                                              # off the centroid of the face's first fan triangle (a warped face's point mean is not on the fan)
            a, b, c = P[faces[f][0]], P[faces[f][1]], P[faces[f][2]]
            nrm = np.cross(b - a, c - a)                            # outwards of the owner
            pts.append((a + b + c) / 3.0 + sgn * 1e-6 * h * nrm / np.linalg.norm(nrm))
        groups.append(np.array(pts))
    if centres is not None:
        groups.append(pick(np.asarray(centres, np.float64).reshape(-1, 3), 300))
    groups.append(np.full((1, 3), np.nan))
    groups.append((lo + 100.0 * (hi - lo))[None, :])
    n_uniform = max(1500, 6000 - sum(g.shape[0] for g in groups))           # (a small mesh has fewer vertices, faces and edges to offer)
    groups.append(lo - 0.05 * (hi - lo) + rs.random_sample((n_uniform, 3)) * 1.1 * (hi - lo))
    X = np.concatenate(groups)
    return X[rs.permutation(X.shape[0])], h


_CASES = {}


def case(oracle, name):
    """(mesh, warped, FindCellRef, X, h) of one mesh of MESHES, built once per process: the centres from the restatement, the points of case_points"""
    if name not in _CASES:
        make, warped = MESHES[name]
        mesh = make()
        npatch = len(mesh["patch_start"])
        o = oracle.LduSolver(mesh, 1e-3, 0.01, U_BC.get(name, [0] * npatch), [(0, 0, 0)] * npatch, [0] * npatch)
        C = np.array(o.geometry("C"), np.float64).reshape(-1, 3)
        o.close()
        X, h = case_points(mesh, C)
        _CASES[name] = (mesh, warped, FindCellRef(mesh, C), X, h)
    return _CASES[name]
