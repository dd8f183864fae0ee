"""A plain numpy statement of the general-mesh pressure multigrid (csrc/ldu_amg.hip): the agglomeration hierarchy, the Galerkin coarse operators, the
V-cycle, and OpenFOAM's PCG around it -- the reference that tests/test_amg_reference.py holds to itself and to closed forms and tests/test_amg_parity.py
holds the HIP solver to.  It depends on neither the product nor the oracle.

Input: the mesh dict (tests/poly_meshes.py), the internal-face areas, the level-0 face coefficients p_coef[:n_internal] and diagonal p_diag as the
solver's get() returns them after a step, the pressure reference cell (None where a fixed-value patch makes one unnecessary) and the number of pairwise
passes per level.  Everything below level 0 is rebuilt here.

  graph          per cell its internal faces in ascending face number; a cyclic pair's faces are internal faces, after the mesh's own, pair by pair
                 in patch order, owner = the lower of the two cells
  agglomeration  up to `passes` matching passes per level, composed.  One pass: in cell order a free cell pairs with its free neighbour across the
                 heaviest face -- among the faces within 0.8 of the heaviest the first in row order --; a cell left alone joins the cluster of its
                 heaviest clustered neighbour (same tie rule); clusters are numbered by their first cell; a coarse row lists its neighbours ascending,
                 each with the summed weight.  Passes stop once a level has COARSEST / 2 cells or fewer, or when a pass no longer shrinks the graph;
                 a level that is not under 0.9 of the one above is not added; levels are added until one has COARSEST cells or fewer.
                 Weights are doubles summed in the product's order: the comparisons must fall as they do there
  operators      row c: diag_c x_c - sum coef x_nbr.  scale = (n_fine / n_coarse)^(-1/3), a double.  Coarse off-diagonal = scale * the sum of the fine
                 entries between two aggregates; coarse diagonal = scale * (the children's diagonals - the entries inside the aggregate, from both
                 sides) + (1 - scale) * 0.5 diag_0[ref] on the aggregate that holds the reference cell (setReference doubled that diagonal: the point
                 term is half of it, and it is carried down unscaled)
  V-cycle        from zero x = wa b / d, x += wb (b - A x) / d; restrict the residual by summing over aggregates; recurse; prolong by injection;
                 x += wb (b - A x) / d, x += wa (b - A x) / d; the last level is solved exactly: x = A^-1 b with A^-1 from Gauss-Jordan elimination
                 without pivoting (what the device does in LDS: the same arithmetic in `dtype`)
  PCG            PCG.C with lduMatrix::solver::normFactor [OF-6]

Every class takes `dtype`: numpy.longdouble is the reference, numpy.float64 the same statement in the device's number format -- the distance between
the two is what double arithmetic alone costs, and the parity test's bounds are ten times that.

Dense is the second statement, in dense linear algebra: explicit P matrices, coarse operator scale P^T (A - D_point) P + D_point, the cycle as a
product of matrices that gives M^-1 outright.  CPU tests only."""
import numpy as np

LD = np.longdouble
WA, WB = 1.7318685872766142, 0.5695012757370842           # kWa, kWb: the doubles in ldu_amg.hip
COARSEST = 64                                              # kAmgCoarsest
PAIR_TIE = 0.8                                             # kPairTie
MAX_LEVELS = 24


def internal_faces(mesh):
    """(owner, neighbour) of the solver's internal faces: the mesh's own, then the folded cyclic pairs"""
    ni = len(mesh["neighbour"])
    own = [int(v) for v in mesh["owner"][:ni]]; nei = [int(v) for v in mesh["neighbour"]]
    pn = mesh.get("patch_neighbour")
    if pn is not None:
        for a, b in enumerate(pn):
            if b < 0 or b < a:
                continue
            for q in range(int(mesh["patch_size"][a])):
                ca, cb = int(mesh["owner"][mesh["patch_start"][a] + q]), int(mesh["owner"][mesh["patch_start"][b] + q])
                own.append(min(ca, cb)); nei.append(max(ca, cb))
    return np.asarray(own, np.int64), np.asarray(nei, np.int64)


class Graph:
    """rows as lists: off[c] .. off[c + 1] index nbr (the neighbour) and w (the weight, a Python float = a double)"""
    def __init__(self, n, off, nbr, w):
        self.n, self.off, self.nbr, self.w = n, off, nbr, w

    def widest(self):
        return max([1] + [self.off[c + 1] - self.off[c] for c in range(self.n)])


def mesh_graph(n_cells, own, nei, weight):
    """(graph, face_of): face_of[q] = the face of row entry q"""
    rows = [[] for _ in range(n_cells)]
    for f in range(len(own)):                    # ascending face number lands in every row in ascending order
        rows[own[f]].append((int(nei[f]), f)); rows[nei[f]].append((int(own[f]), f))
    off, nbr, w, face_of = [0], [], [], []
    for r in rows:
        for nb, f in r:
            nbr.append(nb); w.append(float(weight[f])); face_of.append(f)
        off.append(len(nbr))
    return Graph(n_cells, off, nbr, w), np.asarray(face_of, np.int64)


def _pick(G, cl, c, free, tie):
    """the neighbour of c to go with: among the free (or the clustered) ones, the first in row order whose face is within `tie` of the heaviest"""
    best = -1.0
    for q in range(G.off[c], G.off[c + 1]):
        nb = G.nbr[q]
        if nb != c and ((cl[nb] < 0) if free else (cl[nb] >= 0)) and G.w[q] > best:
            best = G.w[q]
    if best < 0.0:
        return -1
    for q in range(G.off[c], G.off[c + 1]):
        nb = G.nbr[q]
        if nb != c and ((cl[nb] < 0) if free else (cl[nb] >= 0)) and G.w[q] >= tie * best:
            return nb
    return -1


def pair_pass(G, tie=PAIR_TIE):
    """(cluster of every cell, number of clusters)"""
    ALONE = -2
    cl = [-1] * G.n
    nc = 0
    for c in range(G.n):
        if cl[c] >= 0:
            continue
        mate = _pick(G, cl, c, True, tie)
        if mate >= 0:
            cl[c] = cl[mate] = nc; nc += 1
        else:
            cl[c] = ALONE
    for c in range(G.n):
        if cl[c] != ALONE:
            continue
        host = _pick(G, cl, c, False, tie)
        if host >= 0:
            cl[c] = cl[host]
        else:
            cl[c] = nc; nc += 1
    number, out = {}, []
    for v in cl:                                   # by first cell
        if v not in number:
            number[v] = len(number)
        out.append(number[v])
    return out, nc


def coarse_graph(G, cl, nc):
    members = [[] for _ in range(nc)]
    for c in range(G.n):
        members[cl[c]].append(c)
    off, nbr, w = [0], [], []
    for I in range(nc):
        row = {}
        for c in members[I]:
            for q in range(G.off[c], G.off[c + 1]):
                J = cl[G.nbr[q]]
                if J != I:
                    row[J] = row.get(J, 0.0) + G.w[q]          # summed in the order met: children ascending, each child's row in order
        for J in sorted(row):
            nbr.append(J); w.append(row[J])
        off.append(len(nbr))
    return Graph(nc, off, nbr, w)


def agglomerate(G, passes=3, tie=PAIR_TIE):
    """[(graph, agg)] per level, finest first; agg: this level's cell -> the next level's (None on the last)"""
    out = []
    while G.n > COARSEST and len(out) + 1 < MAX_LEVELS:
        agg = list(range(G.n)); cur = G; nc = G.n
        for _ in range(passes):
            if not nc > COARSEST // 2:
                break
            cl, n2 = pair_pass(cur, tie)
            if n2 >= nc:
                break
            agg = [cl[a] for a in agg]
            cur = coarse_graph(cur, cl, n2); nc = n2
        if nc >= G.n or nc > 0.9 * G.n:
            break
        out.append((G, np.asarray(agg, np.int64)))
        G = cur
    out.append((G, None))
    if len(out) > 1 and G.n > COARSEST:
        raise ValueError("the agglomeration stalled at %d cells" % G.n)
    return out


class Level:
    """CSR rows (row, nbr, coef aligned), the diagonal, agg, the coarse cell that holds the reference cell (or None)"""
    def __init__(self, G, agg, dtype):
        self.n, self.W, self.agg = G.n, G.widest(), agg
        self.off = np.asarray(G.off, np.int64); self.nbr = np.asarray(G.nbr, np.int64).reshape(-1)
        self.row = np.repeat(np.arange(G.n), np.diff(self.off))
        self.dtype = dtype
        self.coef = self.diag = None
        self.ref = None

    def apply(self, x):
        y = self.diag * x
        np.subtract.at(y, self.row, self.coef * x[self.nbr])
        return y

    def ell(self):
        """(nbr, coef) slot-major [W, n]: a row's entries first, then the cell itself with coefficient 0"""
        nb = np.tile(np.arange(self.n), (self.W, 1)); cf = np.zeros((self.W, self.n), self.dtype)
        slot = np.arange(len(self.row)) - self.off[self.row]
        nb[slot, self.row] = self.nbr; cf[slot, self.row] = self.coef
        return nb, cf

    def dense(self):
        m = np.zeros((self.n, self.n), self.dtype)
        m[np.arange(self.n), np.arange(self.n)] = self.diag
        np.subtract.at(m, (self.row, self.nbr), self.coef)
        return m


def scale_of(n_fine, n_coarse):
    """the double the product forms: std::pow((double) n_fine / (double) n_coarse, -1.0 / 3.0)"""
    return (float(n_fine) / float(n_coarse)) ** (-1.0 / 3.0)


def invert_no_pivot(m):
    """Gauss-Jordan in place, no pivoting, in the precision of m (k_amg_coarsest_invert's arithmetic)"""
    a = m.copy(); n = a.shape[0]
    one = a.dtype.type(1)
    for k in range(n):
        p = one / a[k, k]
        col = a[:, k].copy()
        rowk = a[k, :] * p
        rowk[k] = p
        a -= col[:, None] * rowk[None, :]
        a[:, k] = -col * p
        a[k, :] = rowk
    return a


class Hierarchy:
    def __init__(self, mesh, areas, p_coef, p_diag, ref_cell=None, passes=3, dtype=LD, tie=PAIR_TIE):
        own, nei = internal_faces(mesh)
        ni = len(own)
        self.dtype = dtype
        G, face_of = mesh_graph(int(mesh["n_cells"]), own, nei, np.asarray(areas, np.float64)[:ni])
        chain = agglomerate(G, passes, tie)
        self.levels = [Level(g, a, dtype) for g, a in chain]
        self.ref_cell = ref_cell
        ref = ref_cell
        for L in self.levels:
            L.ref = ref
            ref = None if ref is None or L.agg is None else int(L.agg[ref])
        self.face_of = face_of
        self.set_matrix(p_coef, p_diag)

    def set_matrix(self, p_coef, p_diag):
        """level 0 from the face coefficients and the diagonal; every coarse level and the last level's inverse from them"""
        dt = self.dtype
        L0 = self.levels[0]
        L0.coef = np.asarray(p_coef, np.float64)[self.face_of].astype(dt)
        L0.diag = np.asarray(p_diag, np.float64).astype(dt)
        point = dt(0.5) * L0.diag[self.ref_cell] if self.ref_cell is not None else None
        self.scales = []
        for F, C in zip(self.levels[:-1], self.levels[1:]):
            s = dt(scale_of(F.n, C.n)); self.scales.append(s)
            I, J = F.agg[F.row], F.agg[F.nbr]
            inside = I == J
            # a coarse row ascends by neighbour and the rows follow one another: the keys row * n + nbr ascend
            slot = np.searchsorted(C.row * C.n + C.nbr, I[~inside] * C.n + J[~inside])
            tot = np.zeros(len(C.row), dt); np.add.at(tot, slot, F.coef[~inside])
            C.coef = s * tot
            d = np.zeros(C.n, dt); np.add.at(d, F.agg, F.diag)
            din = np.zeros(C.n, dt); np.add.at(din, I[inside], F.coef[inside])
            C.diag = s * (d - din)
            if point is not None:
                C.diag[C.ref] += (dt(1) - s) * point
        self.coarse_inv = invert_no_pivot(self.levels[-1].dense())

    def mg_levels(self):
        return [(L.n, L.W) for L in self.levels]

    def apply(self, x):
        return self.levels[0].apply(np.asarray(x, self.dtype))

    def _vcycle(self, l, b):
        dt = self.dtype
        L = self.levels[l]
        if l + 1 == len(self.levels):
            return self.coarse_inv.T @ b            # x_t = sum_j inv[j, t] b_j, as the tail kernel reads the (symmetric) inverse
        wa, wb = dt(WA), dt(WB)
        x = wa * b / L.diag
        x = x + wb * (b - L.apply(x)) / L.diag
        r = b - L.apply(x)
        bc = np.zeros(self.levels[l + 1].n, dt); np.add.at(bc, L.agg, r)
        x = x + self._vcycle(l + 1, bc)[L.agg]
        x = x + wb * (b - L.apply(x)) / L.diag
        x = x + wa * (b - L.apply(x)) / L.diag
        return x

    def precondition(self, r):
        """z = M^-1 r: one V-cycle from zero"""
        return self._vcycle(0, np.asarray(r, np.float64).astype(self.dtype))


class Dense:
    """the same hierarchy in dense linear algebra, from a Hierarchy's aggregates: A_0 dense, P_l [n_l, n_l+1] of zeros and ones,
    A_l+1 = scale P^T (A_l - D_l) P + P^T D_l P with D_0 = the reference cell's point term; Minv = the cycle's matrix"""
    def __init__(self, H, dtype=None):
        dt = self.dtype = dtype or H.dtype
        self.A = [H.levels[0].dense().astype(dt)]
        n0 = H.levels[0].n
        D = np.zeros((n0, n0), dt)
        if H.ref_cell is not None:
            D[H.ref_cell, H.ref_cell] = dt(0.5) * self.A[0][H.ref_cell, H.ref_cell]
        self.P = []
        for F, C in zip(H.levels[:-1], H.levels[1:]):
            P = np.zeros((F.n, C.n), dt); P[np.arange(F.n), F.agg] = 1
            s = dt(scale_of(F.n, C.n))
            Dc = P.T @ D @ P
            self.A.append(s * (P.T @ (self.A[-1] - D) @ P) + Dc)
            self.P.append(P); D = Dc
        self.Minv = self._minv(0)

    def _inverse(self, m):
        if self.dtype == np.float64:
            return np.linalg.inv(m)
        x = np.linalg.inv(m.astype(np.float64)).astype(self.dtype)           # two Newton steps lift the double inverse to the working precision
        for _ in range(2):
            x = x @ (2 * np.eye(m.shape[0], dtype=self.dtype) - m @ x)
        return x

    def _minv(self, l):
        dt = self.dtype
        A = self.A[l]
        if l + 1 == len(self.A):
            return self._inverse(A)
        n = A.shape[0]
        Dinv = np.diag(1 / np.diag(A)); E = np.eye(n, dtype=dt)
        X = dt(WA) * Dinv
        X = X + dt(WB) * Dinv @ (E - A @ X)
        P = self.P[l]
        X = X + P @ self._minv(l + 1) @ P.T @ (E - A @ X)
        X = X + dt(WB) * Dinv @ (E - A @ X)
        X = X + dt(WA) * Dinv @ (E - A @ X)
        return X


def pcg(A, M, b, x0, iters, dtype=LD):
    """OpenFOAM's PCG.C: A, M callables (matrix, preconditioner).  Returns ([x_1 .. x_iters], [res_0 .. res_iters]) with the residuals
    sum|r| / normFactor, normFactor = sum(|A x - A xbar| + |b - A xbar|) + 1e-20, xbar the mean of the initial x"""
    b = np.asarray(b, np.float64).astype(dtype); x = np.asarray(x0, np.float64).astype(dtype)
    wA = A(x)
    pA = A(np.full(x.shape, x.mean(), dtype))
    norm = (np.abs(wA - pA) + np.abs(b - pA)).sum() + dtype(1e-20)
    r = b - wA
    xs, res = [], [np.abs(r).sum() / norm]
    p, old = None, None
    for it in range(iters):
        z = M(r)
        zr = z @ r
        p = z.copy() if it == 0 else z + (zr / old) * p
        wA = A(p)
        alpha = zr / (wA @ p)
        x = x + alpha * p
        r = r - alpha * wA
        old = zr
        xs.append(x.copy()); res.append(np.abs(r).sum() / norm)
    return xs, res
