"""tests/amg_ref.py -- the long-double statement of the general-mesh pressure multigrid that tests/test_amg_parity.py holds the HIP solver to -- held
to itself and to closed forms, on the CPU: the hierarchies of tests/amg_cases.py, the structure of the aggregates, the row-wise statement against the
dense one (explicit P matrices, M^-1 outright), and what a preconditioner must be.  The level-0 matrices are synthetic (amg_cases.synthetic_matrix)."""
import functools

import numpy as np
import pytest

import amg_cases as ac
import amg_ref as ar
import poly_meshes as pm

LD = np.longdouble
NAMES = [c.name for c in ac.CASES]
DENSE_MAX = 2000             # cells up to which M^-1 is formed outright
DENSE_LD_MAX = 400           # ... in long double (numpy multiplies long-double matrices without BLAS); above it in double


@functools.lru_cache(maxsize=None)
def hierarchy(name, dtype=LD):
    c = ac.BY_NAME[name]
    areas, coef, diag, _ = ac.synthetic_matrix(c)
    return ar.Hierarchy(c.mesh, areas, coef, diag, c.ref, c.passes, dtype)


@functools.lru_cache(maxsize=None)
def dense(name):
    n = ac.BY_NAME[name].mesh["n_cells"]
    dt = LD if n <= DENSE_LD_MAX else np.float64
    H = hierarchy(name, dt)
    return H, ar.Dense(H)


def statement_bound(dtype, family):
    """two statements in the same number format differ by what that format costs: ten times d64 in double, 2^-11 of that in long double (64 against 53 bits)"""
    return ac.BOUND_FACTOR * ac.D64[family] * (1.0 if dtype == np.float64 else 2.0 ** -11)


@pytest.mark.parametrize("name", NAMES)
def test_the_level_table(name):
    assert hierarchy(name).mg_levels() == ac.BY_NAME[name].levels


def test_reference_cells_off_aggregate_zero():
    """the cases that name a reference cell other than 0 do so to put the point term on another aggregate than the first"""
    moved = [c for c in ac.CASES if c.ref not in (None, 0)]
    assert len(moved) >= 4
    for c in moved:
        assert hierarchy(c.name).levels[1].ref != 0, c.name


def test_wavy_lattice_stacks_into_boxes():
    """16^3, mildly distorted: the face areas differ by a few per cent, count as ties, and three passes give 2 x 2 x 2 boxes on level 0; with the strict
    maximum in place of the tie rule they do not (what the rule is for, and that this test sees the rule)"""
    n = 16
    mesh = pm.hex_block(n, n, n, vertex_map=pm.wavy(0.03))
    G, _ = ar.mesh_graph(n ** 3, *ar.internal_faces(mesh), ac.face_areas(mesh))
    chain = ar.agglomerate(G)
    assert [(g.n, g.widest()) for g, _ in chain] == [(4096, 6), (512, 6), (64, 6)]
    i, j, k = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    box = np.zeros(n ** 3, np.int64)
    box[(i + n * (j + n * k)).ravel()] = ((i // 2) + (n // 2) * ((j // 2) + (n // 2) * (k // 2))).ravel()
    assert np.array_equal(chain[0][1], box)
    strict = ar.agglomerate(G, tie=1.0)
    assert not np.array_equal(strict[0][1], box)


@pytest.mark.parametrize("name", NAMES)
def test_aggregates_partition_the_cells_and_are_connected(name):
    H = hierarchy(name)
    for L, C in zip(H.levels[:-1], H.levels[1:]):
        agg = L.agg
        assert agg.shape == (L.n,) and agg.min() == 0 and agg.max() == C.n - 1 and len(np.unique(agg)) == C.n
        first = np.full(C.n, L.n); np.minimum.at(first, agg, np.arange(L.n))
        assert np.all(np.diff(first) > 0)                                   # numbered by first cell
        # connected: spread the lowest cell number through the faces inside each aggregate until nothing changes
        inside = agg[L.row] == agg[L.nbr]
        r, c = L.row[inside], L.nbr[inside]
        lab = np.arange(L.n)
        for _ in range(L.n):
            new = lab.copy(); np.minimum.at(new, r, lab[c])
            if np.array_equal(new, lab):
                break
            lab = new
        assert np.array_equal(lab, first[agg])
        # the coarse rows: ascending neighbours, no self entry, symmetric pattern
        assert np.all(C.nbr != C.row)
        same_row = C.row[1:] == C.row[:-1]
        assert np.all(np.diff(C.nbr)[same_row] > 0)
        pairs = set(zip(C.row.tolist(), C.nbr.tolist()))
        assert all((b, a) in pairs for a, b in pairs)


@pytest.mark.parametrize("name", NAMES)
def test_ell_padding_follows_the_entries(name):
    H = hierarchy(name)
    for L in H.levels:
        nb, cf = L.ell()
        assert nb.shape == cf.shape == (L.W, L.n)
        pad = nb == np.arange(L.n)[None, :]
        assert np.all(cf[pad] == 0) and np.all(cf[~pad] > 0)
        assert np.all(pad[1:] >= pad[:-1])                                   # once a row is padding it stays padding
        assert (~pad).sum() == len(L.row) and (~pad).sum(axis=0).max() == L.W


@pytest.mark.parametrize("name", [c.name for c in ac.CASES if c.mesh["n_cells"] <= DENSE_MAX])
def test_the_two_statements_agree(name):
    """coarse operators level by level, and M^-1 applied to unit vectors (the columns of the dense M^-1) and to the probe vectors"""
    H, D = dense(name)
    dt = H.dtype
    assert len(D.A) == len(H.levels)
    for l, L in enumerate(H.levels):
        a, b = L.dense(), D.A[l]
        assert ac.rel(np.diag(a), np.diag(b)) <= statement_bound(dt, "diag"), (l, ac.rel(np.diag(a), np.diag(b)))
        off = lambda m: m - np.diag(np.diag(m))
        if L.n > 1:
            assert np.abs(off(a) - off(b)).max() <= statement_bound(dt, "coef") * np.abs(off(b)).max(), l
    n = H.levels[0].n
    cells = sorted({0, n - 1, n // 2, H.ref_cell or 0, *np.random.RandomState(2).randint(0, n, 3).tolist()})
    for c in cells:
        z = H.precondition(np.eye(1, n, c).ravel())
        assert ac.rel(z, D.Minv[:, c]) <= statement_bound(dt, "cycle"), (c, ac.rel(z, D.Minv[:, c]))
    _, _, _, C = ac.synthetic_matrix(ac.BY_NAME[name])
    for nm, r in ac.probe_vectors(H, C, H.ref_cell).items():
        z, zd = H.precondition(r), D.Minv @ r.astype(dt)
        assert ac.rel(z, zd) <= statement_bound(dt, "cycle"), (nm, ac.rel(z, zd))


@pytest.mark.parametrize("name", NAMES)
def test_the_cycle_is_symmetric_and_positive_definite(name):
    c = ac.BY_NAME[name]
    if c.mesh["n_cells"] <= DENSE_MAX:
        H, D = dense(name)
        M = D.Minv.astype(np.float64)
        assert np.abs(M - M.T).max() <= statement_bound(np.float64, "cycle") * np.abs(M).max()
        np.linalg.cholesky(0.5 * (M + M.T))                                  # raises unless positive definite
    else:
        H = hierarchy(name)
        rs = np.random.RandomState(11)
        for _ in range(3):
            a, b = rs.standard_normal(H.levels[0].n), rs.standard_normal(H.levels[0].n)
            Ma, Mb = H.precondition(a), H.precondition(b)
            assert abs(Ma @ b - Mb @ a) <= 1e-15 * (np.abs(Ma) @ np.abs(b)) and Ma @ a > 0 and Mb @ b > 0


@pytest.mark.parametrize("name", NAMES)
def test_coarse_rows_sum_to_the_scaled_fine_row_sums(name):
    """without a reference term -- a fixed-value patch, or here a positive term on every diagonal in place of the doubled reference cell -- the Galerkin
    product keeps row sums: the row sum of a coarse cell = scale * the summed row sums of its children"""
    c = ac.BY_NAME[name]
    areas, coef, diag, _ = ac.synthetic_matrix(c)
    if c.ref is not None:
        diag = diag.copy(); diag[c.ref] *= 0.5
        diag += 0.01 * diag * np.random.RandomState(3).random_sample(len(diag))
    H = ar.Hierarchy(c.mesh, areas, coef, diag, None, c.passes, LD)
    for l, (F, C) in enumerate(zip(H.levels[:-1], H.levels[1:])):
        rsum = lambda L: L.apply(np.ones(L.n, LD))
        want = np.zeros(C.n, LD); np.add.at(want, F.agg, rsum(F))
        want *= H.scales[l]
        assert float(H.scales[l]) == (F.n / C.n) ** (-1.0 / 3.0)
        assert np.abs(rsum(C) - want).max() <= 1e-17 * np.abs(C.diag).max(), l


def test_clean_pairs_scale_by_the_cube_root_of_two():
    H = hierarchy("line_1pass")
    assert np.array_equal(H.levels[0].agg, np.arange(200) // 2) and float(H.scales[0]) == 2.0 ** (-1.0 / 3.0)
    F, C = H.levels[0], H.levels[1]
    # a chain: the coarse coefficient between two pairs is the one fine coefficient between them, scaled
    fine = {(int(r), int(c)): v for r, c, v in zip(F.row, F.nbr, F.coef)}
    for r, c, v in zip(C.row, C.nbr, C.coef):
        assert v == H.scales[0] * fine[(2 * int(r) + (1 if c > r else 0), 2 * int(c) + (0 if c > r else 1))]
    # the point term is carried whole: the reference aggregate's row sum is scale * 0 + the point term
    point = LD(0.5) * F.diag[0]
    assert abs(C.apply(np.ones(C.n, LD))[0] - point) <= 1e-17 * point


def test_single_level_cycle_is_the_inverse():
    H = hierarchy("single_level")
    assert len(H.levels) == 1
    A = H.levels[0].dense()
    cols = np.stack([H.precondition(np.asarray(A[:, c], np.float64)) for c in range(H.levels[0].n)], axis=1)
    # (the columns of A were rounded to double on the way in: 2^-53 of them comes back multiplied by the inverse)
    assert np.abs(cols - np.eye(H.levels[0].n)).max() <= 2.0 ** -52 * np.abs(H.coarse_inv).max() * np.abs(A).max()


def test_d64_is_what_amg_cases_records():
    """the parity test's bounds are ten times amg_cases.D64: the float64 statement against the long-double one, largest over the cases, re-measured here"""
    worst = {k: 0.0 for k in ac.D64}
    for c in ac.CASES:
        for k, v in ac.measure_d64(c).items():
            worst[k] = max(worst[k], v)
    for k in ac.D64:
        assert ac.D64[k] / 2 <= worst[k] <= ac.D64[k], (k, worst[k], ac.D64[k])
