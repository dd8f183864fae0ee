"""tests/find_cell_ref.py (mesh.findCell restated as OpenFOAM's face-fan tetrahedra, numpy, long double) held to properties, without a device: the tetrahedra tile
every mesh of tests/test_ldu_find_cell.py, and the point sets of that file carry the adversarial share its cases count on."""
import numpy as np
import pytest

import find_cell_ref as fr
import poly_meshes as pm


@pytest.mark.parametrize("name", list(fr.MESHES))
def test_the_tetrahedra_tile_the_mesh(oracle, name):
    """every uniform point inside is in exactly one cell; no interior vertex, face centre or edge midpoint is in none; a vertex is in every cell that has it; points
    outside the bounding box are in no cell"""
    mesh, warped, ref, _, h = fr.case(oracle, name)
    rs = np.random.RandomState(7)
    P = np.asarray(mesh["points"], np.float64)
    lo, hi = P.min(axis=0), P.max(axis=0)
    X = lo + rs.random_sample((3000, 3)) * (hi - lo)
    _, n_adm, _, _ = ref.classify(X)
    if name == "hex_sheared":                             # the mesh is not its bounding box: inside = the unsheared point lies in the unit box
        un = X.copy()
        un[:, 1] -= 0.25 * X[:, 2]
        un[:, 0] -= 0.3 * un[:, 1] + 0.2 * X[:, 2]
        inside = np.all((un > 1e-6) & (un < 1 - 1e-6), axis=1)
        outside = np.any((un < -1e-6) | (un > 1 + 1e-6), axis=1)
        assert inside.sum() > 500 and outside.sum() > 500
        assert np.all(n_adm[inside] >= 1) and np.all(n_adm[outside] == 0)
        X, n_adm = X[inside], n_adm[inside]
    elif name == "cyclic_wavy":                           # every vertex moves by up to 0.025 per component: no side of the box is a plane
        inside = np.all((X > lo + 0.06) & (X < hi - 0.06), axis=1)
        X, n_adm = X[inside], n_adm[inside]
    assert np.all(n_adm >= 1), "a point inside the mesh that no tetrahedron holds"
    assert np.all(n_adm == 1), "a uniform point in two cells: the tetrahedra overlap (or, one in a million, a seed put it within 1e-9 of a shared triangle: change the seed)"
    faces = fr.faces_of(mesh)
    ni = len(mesh["neighbour"])
    own, nei = np.asarray(mesh["owner"]), np.asarray(mesh["neighbour"])
    cells_with = [set() for _ in range(P.shape[0])]
    for f, q in enumerate(faces):
        for v in q:
            cells_with[v].add(int(own[f]))
            if f < ni:
                cells_with[v].add(int(nei[f]))
    got = ref.cells_of(P)
    assert all(cells_with[v] <= got[v] for v in range(P.shape[0])), "a vertex is not in a cell that has it"
    fc = np.array([P[q].mean(axis=0) for q in faces[:ni]])
    em = np.array([0.5 * (P[a] + P[b]) for q in faces[:ni] for a, b in zip(q, np.roll(q, -1))])
    for Y in (fc, em):
        assert np.all(ref.classify(Y)[1] >= 1)
    far = np.concatenate([hi + rs.random_sample((200, 3)) * 0.3 + 1e-6, lo - rs.random_sample((200, 3)) * 0.3 - 1e-6, np.full((1, 3), np.nan), (lo + 100 * (hi - lo))[None, :]])
    assert np.all(ref.classify(far)[3])


def test_a_lattice_answers_floor_x_over_dx(oracle):
    n = (5, 4, 6)
    L = (1.0, 0.8, 1.5)
    mesh = pm.hex_block(*n, L, renumber_seed=3)
    o = oracle.LduSolver(mesh, 1e-3, 0.01, [0] * 6, [(0, 0, 0)] * 6, [0] * 6)
    ref = fr.FindCellRef(mesh, o.geometry("C"))
    o.close()
    rs = np.random.RandomState(2)
    X = rs.random_sample((2000, 3)) * np.array(L)
    ijk = np.floor(X / (np.array(L) / np.array(n))).astype(int)
    want = mesh["perm"][ijk[:, 0] + n[0] * (ijk[:, 1] + n[1] * ijk[:, 2])]
    got = ref.cells_of(X)
    assert all(g == {int(w)} for w, g in zip(want, got))


@pytest.mark.parametrize("name", list(fr.MESHES))
def test_the_point_sets_carry_their_adversarial_share(oracle, name):
    """what tests/test_ldu_find_cell.py asserts of its inputs before it calls the device, here without one"""
    mesh, warped, ref, X, h = fr.case(oracle, name)
    assert mesh["n_cells"] <= 1000 and 6000 <= X.shape[0] <= 7000
    pairs, n_adm, d_in, d_out = ref.classify(X)
    free = ~d_in & ~d_out
    assert free.mean() <= 0.02, free.mean()
    assert (n_adm > 1).sum() >= 500 and d_out.sum() >= 200
    if warped:
        assert (d_in & ~ref.admissible(pairs, ref.nearest_centre(np.nan_to_num(X)), X.shape[0])).sum() >= 100
