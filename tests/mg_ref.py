"""A plain numpy.longdouble statement of the block pressure solver's multigrid V-cycle and of OpenFOAM's PCG: the reference that
tests/test_mg_reference.py holds the CPU oracle to and tests/test_mg_parity.py the HIP solver.  It depends on neither of them.

Input: the level-0 coefficients diag, ux, uy, uz in cell order i + nx (j + ny k) -- ux[c], uy[c], uz[c] sit on the face of cell c towards +x, +y, +z --
the block's dimensions, and the pressure reference cell (None where a fixed-value pressure side makes one unnecessary).  Everything below level 0 is
rebuilt here from those four arrays.

  operator    y_c = diag_c x_c - sum over the six faces of u_face x_neighbour
  shapes      (n + 1) // 2 per axis and level; the last level is the first with N <= 128 and no edge over 8, or with every edge <= 2
  coarsening  aggregates (i >> 1, j >> 1, k >> 1); coarse diag = sum of 0.5 diag - the faces inside the aggregate; a coarse face = 0.5 sum of the fine
              faces between two aggregates; the aggregate of level l + 1 that holds the reference cell gets 0.25 diag_0[ref] added
  V-cycle     from zero x = wa b / diag, x += wb (b - A x) / diag; restrict the residual by summing over aggregates; recurse; prolong by injection;
              x += wb (b - A x) / diag, x += wa (b - A x) / diag; the last level is solved exactly (dense elimination)
  PCG         PCG.C with lduMatrix::solver::normFactor [OF-6]
"""
import numpy as np

LD = np.longdouble
WA, WB = LD(1.7318685872766142), LD(0.5695012757370842)      # the Chebyshev pair of Jacobi weights (kMgWa, kMgWb), as the doubles the solvers hold
COARSEST_CELLS, COARSEST_EDGE = 128, 8


def shapes(nx, ny, nz):
    """[(nx, ny, nz)] per level, finest first"""
    out = []
    while True:
        out.append((nx, ny, nz))
        if (nx * ny * nz <= COARSEST_CELLS and max(nx, ny, nz) <= COARSEST_EDGE) or max(nx, ny, nz) <= 2:
            return out
        nx, ny, nz = (nx + 1) // 2, (ny + 1) // 2, (nz + 1) // 2


class Level:
    def __init__(self, dims, diag, ux, uy, uz):
        nx, ny, nz = dims
        self.dims = dims
        sh = (nz, ny, nx)
        self.diag = np.asarray(diag, LD).reshape(sh).copy()
        # a coefficient on a face with no cell behind it takes no part in the operator: dropped here once
        self.ux = np.asarray(ux, LD).reshape(sh).copy(); self.ux[:, :, -1] = 0
        self.uy = np.asarray(uy, LD).reshape(sh).copy(); self.uy[:, -1, :] = 0
        self.uz = np.asarray(uz, LD).reshape(sh).copy(); self.uz[-1, :, :] = 0

    def apply(self, x):
        y = self.diag * x
        y[:, :, :-1] -= self.ux[:, :, :-1] * x[:, :, 1:]
        y[:, :, 1:] -= self.ux[:, :, :-1] * x[:, :, :-1]
        y[:, :-1, :] -= self.uy[:, :-1, :] * x[:, 1:, :]
        y[:, 1:, :] -= self.uy[:, :-1, :] * x[:, :-1, :]
        y[:-1, :, :] -= self.uz[:-1, :, :] * x[1:, :, :]
        y[1:, :, :] -= self.uz[:-1, :, :] * x[:-1, :, :]
        return y

    def dense(self):
        nx, ny, nz = self.dims
        n = nx * ny * nz
        m = np.zeros((n, n), LD)
        e = np.zeros((nz, ny, nx), LD)
        for c in range(n):
            e.flat[c] = 1
            m[:, c] = self.apply(e).ravel()
            e.flat[c] = 0
        return m


def _padded(a, dims_c):
    """a fine-level array on the even-sized box that the coarse level's aggregates span (zeros where there is no fine cell)"""
    out = np.zeros((2 * dims_c[2], 2 * dims_c[1], 2 * dims_c[0]), LD)
    out[:a.shape[0], :a.shape[1], :a.shape[2]] = a
    return out


def _children(a, dk, dj, di):
    return a[dk::2, dj::2, di::2]


def coarsen(fine, dims_c, ref_ijk, ref_term):
    """the level under `fine`; ref_ijk: the coarse aggregate that holds the reference cell, or None"""
    d, x, y, z = (_padded(a, dims_c) for a in (fine.diag, fine.ux, fine.uy, fine.uz))
    cd = np.zeros((dims_c[2], dims_c[1], dims_c[0]), LD)
    cx, cy, cz = cd.copy(), cd.copy(), cd.copy()
    for dk in (0, 1):
        for dj in (0, 1):
            for di in (0, 1):
                cd += LD(0.5) * _children(d, dk, dj, di)
                # the face towards +x of a child at di = 0 lies inside the aggregate, that of a child at di = 1 between two aggregates
                if di == 0: cd -= _children(x, dk, dj, di)
                else: cx += LD(0.5) * _children(x, dk, dj, di)
                if dj == 0: cd -= _children(y, dk, dj, di)
                else: cy += LD(0.5) * _children(y, dk, dj, di)
                if dk == 0: cd -= _children(z, dk, dj, di)
                else: cz += LD(0.5) * _children(z, dk, dj, di)
    if ref_ijk is not None:
        i, j, k = ref_ijk
        cd[k, j, i] += LD(0.25) * ref_term
    return Level(dims_c, cd, cx, cy, cz)


def solve_dense(m, b):
    """m x = b by Gaussian elimination with partial pivoting, in the precision of m"""
    m = m.copy(); x = np.array(b, LD).copy()
    n = m.shape[0]
    for p in range(n):
        q = p + int(np.argmax(np.abs(m[p:, p])))
        if q != p:
            m[[p, q]] = m[[q, p]]; x[[p, q]] = x[[q, p]]
        f = m[p + 1:, p] / m[p, p]
        m[p + 1:, p:] -= f[:, None] * m[p, p:][None, :]
        x[p + 1:] -= f * x[p]
    for p in range(n - 1, -1, -1):
        x[p] = (x[p] - m[p, p + 1:] @ x[p + 1:]) / m[p, p]
    return x


class Hierarchy:
    def __init__(self, diag, ux, uy, uz, dims, ref_cell=None, ref_aggregate=None):
        """ref_aggregate(l, (i, j, k)) -> the aggregate of level l that gets the reference term: only for tests that show a misplaced term is seen"""
        nx, ny, nz = dims
        self.dims = tuple(dims)
        self.shapes = shapes(nx, ny, nz)
        self.levels = [Level(self.shapes[0], diag, ux, uy, uz)]
        ref = None
        if ref_cell is not None:
            ref = (ref_cell % nx, (ref_cell // nx) % ny, ref_cell // (nx * ny))
            ref_term = LD(np.asarray(diag, np.float64).ravel()[ref_cell])
        for l in range(1, len(self.shapes)):
            at = None
            if ref is not None:
                at = tuple(q >> l for q in ref)
                if ref_aggregate is not None:
                    at = ref_aggregate(l, at)
            self.levels.append(coarsen(self.levels[-1], self.shapes[l], at, ref_term if ref is not None else None))
        self._dense = None

    def operators(self, l):
        """(diag, ux, uy, uz) of level l, flat, in cell order"""
        L = self.levels[l]
        return tuple(a.ravel() for a in (L.diag, L.ux, L.uy, L.uz))

    def apply(self, x):
        L = self.levels[0]
        return L.apply(np.asarray(x, LD).reshape(L.diag.shape)).ravel()

    def _coarsest(self, b):
        L = self.levels[-1]
        if self._dense is None:
            self._dense = L.dense()
        return solve_dense(self._dense, b.ravel()).reshape(b.shape)

    def _vcycle(self, l, b):
        L = self.levels[l]
        if l + 1 == len(self.levels):
            return self._coarsest(b)
        x = WA * b / L.diag
        x = x + WB * (b - L.apply(x)) / L.diag
        r = b - L.apply(x)
        dims_c = self.shapes[l + 1]
        rp = _padded(r, dims_c)
        bc = sum(_children(rp, dk, dj, di) for dk in (0, 1) for dj in (0, 1) for di in (0, 1))
        e = self._vcycle(l + 1, bc)
        nz, ny, nx = r.shape
        x = x + np.repeat(np.repeat(np.repeat(e, 2, axis=0), 2, axis=1), 2, axis=2)[:nz, :ny, :nx]
        x = x + WB * (b - L.apply(x)) / L.diag
        x = x + WA * (b - L.apply(x)) / L.diag
        return x

    def precondition(self, r):
        """z = M^-1 r: one V-cycle from zero"""
        L = self.levels[0]
        return self._vcycle(0, np.asarray(r, LD).reshape(L.diag.shape)).ravel()

    def jacobi(self, r):
        return np.asarray(r, LD) / self.levels[0].diag.ravel()

    def contraction(self, e):
        """what one cycle leaves of the error e in the energy norm: ||(I - M^-1 A) e||_A / ||e||_A"""
        e = np.asarray(e, LD)
        ae = self.apply(e)
        f = e - self.precondition(ae)
        return float(np.sqrt((f @ self.apply(f)) / (e @ ae)))


def pcg(A, M, b, x0, iters):
    """OpenFOAM's PCG.C: A, M callables (matrix, preconditioner).  Returns ([x_1 .. x_iters], [res_0 .. res_iters]) with the residuals
    sum|r| / normFactor, normFactor = sum(|A x - A xbar| + |b - A xbar|) + 1e-20, xbar the mean of the initial x"""
    b = np.asarray(b, LD); x = np.asarray(x0, LD).copy()
    wA = A(x)
    pA = A(np.full(x.shape, x.mean(), LD))
    norm = (np.abs(wA - pA) + np.abs(b - pA)).sum() + LD(1e-20)
    r = b - wA
    xs, res = [], [np.abs(r).sum() / norm]
    p = None
    wArA_old = LD(1)
    for it in range(iters):
        z = M(r)
        wArA = z @ r
        p = z.copy() if it == 0 else z + (wArA / wArA_old) * p
        wA = A(p)
        alpha = wArA / (wA @ p)
        x = x + alpha * p
        r = r - alpha * wA
        wArA_old = wArA
        xs.append(x.copy()); res.append(np.abs(r).sum() / norm)
    return xs, res
