"""tests/ldu_heat_ref.py, the numpy restatement of the T equation on a general mesh, held to what it must reduce to: heat_transfer_ref.assemble_T (the block's
restatement) on a lattice written as a polyhedral mesh, a non-orthogonal correction that sums to zero over the cells, and a uniform temperature as an exact solution.
The geometry arrays come from the CPU restatement of fy_ldu_solver (oracle.LduSolver.geometry), which tests/test_ldu_parity.py pins the device solver's to.  No GPU."""
import numpy as np
import pytest

import heat_transfer_ref as ht
import ldu_heat_ref as lh
import poly_meshes as pm

SHAPE = (5, 4, 3)
GRADING = (0.01 * 1.25 ** np.arange(5), 0.012 * np.ones(4), 0.015 * 0.85 ** np.arange(3))


def geometry(oracle, mesh):
    o = oracle.LduSolver(mesh, 1e-3, 0.01, [0] * len(mesh["patch_start"]), [(0, 0, 0)] * len(mesh["patch_start"]), [0] * len(mesh["patch_start"]))
    g = lh.geometry_of(o)
    orig = o.geometry("orig_face") if mesh.get("patch_neighbour") is not None else None
    o.close()
    return g, orig


def lattice(oracle, graded):
    nx, ny, nz = SHAPE
    if graded:
        h = [np.asarray(a, float) for a in GRADING]
        mesh = pm.hex_block(nx, ny, nz, vertex_map=lh.graded_map(SHAPE, h))
    else:
        h = ht.block_sizes(nx, ny, nz, 0.02)
        mesh = pm.hex_block(nx, ny, nz, (nx * 0.02, ny * 0.02, nz * 0.02))
    return mesh, h, lh.addressing(mesh), geometry(oracle, mesh)[0]


def random_fields(rs, nx, ny, nz):
    N = nx * ny * nz
    phi = (1e-5 * rs.standard_normal((nx + 1) * ny * nz), 1e-5 * rs.standard_normal(nx * (ny + 1) * nz), 1e-5 * rs.standard_normal(nx * ny * (nz + 1)))
    return phi, 0.6 + 0.4 * rs.random_sample(N), 1e-5 * rs.random_sample(N), 300.0 + 50.0 * rs.random_sample(N), 1e-3 * rs.random_sample(N), 0.3 * rs.random_sample(N)


@pytest.mark.parametrize("graded", [False, True], ids=["uniform", "graded"])
@pytest.mark.parametrize("scheme", [ht.LINEAR, ht.UPWIND], ids=["linear", "upwind"])
@pytest.mark.parametrize("fields", ["alpha", "nut"])
def test_lattice_equals_the_block_restatement(oracle, graded, scheme, fields):
    """both patch kinds (fixedValue on XMIN, YMAX, ZMIN), Sp and Su, random phi of both signs.  `alpha`: a random void fraction with the molecular diffusivity;
    `nut`: a random eddy viscosity (Prt 0.85, the boundary's nut the cell's) with alpha = 1.  With BOTH non-uniform the two restatements share every term but the face
    diffusivity alpha_f Deff_f, which each forms as the product of the two linear interpolates -- the same number, so that case is in test_product_of_interpolates"""
    nx, ny, nz = SHAPE
    mesh, h, ad, geo = lattice(oracle, graded)
    phi, alpha, nut, T, Sp, Su = random_fields(np.random.RandomState(3), nx, ny, nz)
    alpha, nut = (alpha, None) if fields == "alpha" else (None, nut)
    bc, val = [1, 0, 0, 1, 1, 0], [280.0, 0, 0, 330.0, 310.0, 0]
    D, Prt, dt, rho_cp = 2e-6, 0.85, 0.02, 4.18e6
    A0, b0 = ht.assemble_T(h, dt, phi, alpha, nut, T, D, Prt, bc, val, scheme, Sp=Sp, Su=Su, rho_cp=rho_cp)
    A1, b1, corr = lh.assemble_T(ad, geo, dt, lh.lattice_phi(mesh, ad, phi), T, D, Prt, bc, val, scheme, alpha=alpha, nut=nut, Sp=Sp, Su=Su, rho_cp=rho_cp)
    eA, eb = np.abs(A1 - A0).max() / np.abs(A0).max(), np.abs(b1 - b0).max() / np.abs(b0).max()
    print(f"graded={graded} scheme={scheme} {fields}: |dA| / max|A| = {eA:.2e}, |db| / max|b| = {eb:.2e}, max|corr| / max|b| = {np.abs(corr).max() / np.abs(b0).max():.2e}")
    assert eA <= 1e-13 and eb <= 1e-13
    assert np.abs(corr).max() <= 1e-13 * np.abs(b0).max()    # an orthogonal mesh: kvec = 0
    assert (np.abs(A0).sum(axis=1) > 0).all() and (np.diag(A0) != np.diag(ht.assemble_T(h, dt, phi, alpha, nut, T, D, Prt, bc, val, scheme)[0])).all()      # Sp reached A


def test_product_of_interpolates(oracle):
    """alpha AND nut non-uniform on the graded lattice: gam_f = alphaf_f (Deff)_f |Sf|, the product of the two linear interpolates as the block states it -- the
    interpolate of the product alpha Deff would differ from it by w (1 - w) (alpha_O - alpha_N)(Deff_O - Deff_N), far above the bar"""
    nx, ny, nz = SHAPE
    mesh, h, ad, geo = lattice(oracle, True)
    phi, alpha, nut, T, Sp, Su = random_fields(np.random.RandomState(5), nx, ny, nz)
    bc, val = [1, 0, 0, 1, 1, 0], [280.0, 0, 0, 330.0, 310.0, 0]
    A0, b0 = ht.assemble_T(h, 0.02, phi, alpha, nut, T, 2e-6, 0.85, bc, val, ht.LINEAR)
    A1, b1, _ = lh.assemble_T(ad, geo, 0.02, lh.lattice_phi(mesh, ad, phi), T, 2e-6, 0.85, bc, val, lh.LINEAR, alpha=alpha, nut=nut)
    assert np.abs(A1 - A0).max() <= 1e-13 * np.abs(A0).max() and np.abs(b1 - b0).max() <= 1e-13 * np.abs(b0).max()
    ni = ad["nei"].size
    o, n, w = ad["own"][:ni], ad["nei"], geo["w"]
    Deff = 2e-6 + nut / 0.85
    cross = (w * (1 - w) * (alpha[o] - alpha[n]) * (Deff[o] - Deff[n]) * geo["magSf"][:ni] * geo["dcNO"][:ni])
    assert np.abs(cross).max() > 1e-6 * np.abs(A0).max()


def wavy_mesh(oracle):
    mesh = pm.hex_block(5, 4, 6, (1.0, 0.8, 1.2), pm.wavy(0.04, (1.0, 0.8, 1.2)), renumber_seed=4)
    return mesh, lh.addressing(mesh), geometry(oracle, mesh)[0]


def test_explicit_correction_sums_to_zero(oracle):
    """a wavy mesh: the non-orthogonal flux is added to the owner and taken from the neighbour, so b's share of it sums to zero over the cells to round-off
    -- while the correction itself is a good part of the diffusive flux"""
    mesh, ad, geo = wavy_mesh(oracle)
    nc, nf = ad["n_cells"], ad["own"].size
    rs = np.random.RandomState(7)
    T = 300.0 + 50.0 * rs.random_sample(nc)
    args = (ad, geo, 0.05, np.zeros(nf), T, 1e-3, 1.0, [0] * 6, [0.0] * 6, lh.LINEAR)
    alpha = 0.6 + 0.4 * rs.random_sample(nc)
    A, b, corr = lh.assemble_T(*args, alpha=alpha)
    part = np.zeros(nc)
    np.add.at(part, ad["own"][:corr.size], corr); np.add.at(part, ad["nei"], -corr)
    assert np.abs(corr).max() > 0 and np.abs(geo["kvec"]).max() > 1e-3
    assert abs(part.sum()) <= 1e-13 * np.abs(corr).sum(), (part.sum(), np.abs(corr).sum())
    # zeroGradient everywhere, no flow, no sources: the columns of A sum to alpha V / dt (the implicit diffusion is symmetric), so the heat content sum alpha V T
    # changes by the sum of the explicit correction only -- by nothing
    Tn = np.linalg.solve(A, b)
    heat = alpha * geo["V"]
    assert np.abs(Tn - T).max() > 0.1
    assert abs((heat * (Tn - T)).sum()) <= 1e-14 * (heat * np.abs(T)).sum()      # (each T carries eps |T| of rounding: 1e-14 of the heat content is ~50 eps)


@pytest.mark.parametrize("scheme", [lh.LINEAR, lh.UPWIND], ids=["linear", "upwind"])
def test_uniform_temperature_solves_the_system(oracle, scheme):
    """T = T0 everywhere with fixedValue patches at T0 (two of them; the rest zeroGradient), a random flux that is NOT divergence free, random alpha and nut, and
    Sp, Su = Sp T0: every term cancels in its own row -- the bounded convection, the gradient (zero for a constant on a closed cell), the sources"""
    mesh, ad, geo = wavy_mesh(oracle)
    nc, nf = ad["n_cells"], ad["own"].size
    rs = np.random.RandomState(9)
    T0 = 312.5
    Sp = 1e-2 * rs.random_sample(nc)
    A, b, corr = lh.assemble_T(ad, geo, 0.05, 1e-3 * rs.standard_normal(nf), np.full(nc, T0), 1e-3, 0.9, [1, 0, 0, 1, 0, 0], [T0, 0, 0, T0, 0, 0], scheme,
                               alpha=0.6 + 0.4 * rs.random_sample(nc), nut=1e-3 * rs.random_sample(nc), Sp=Sp, Su=Sp * T0, rho_cp=50.0)
    res = np.abs(A @ np.full(nc, T0) - b).max()
    print(f"scheme {scheme}: max |A T0 - b| = {res:.3e} of max|b| = {np.abs(b).max():.3e}; max|corr| = {np.abs(corr).max():.3e}")
    assert res <= 1e-12 * np.abs(b).max()
    assert np.abs(corr).max() <= 1e-12 * np.abs(b).max()
    assert np.abs(np.linalg.solve(A, b) - T0).max() <= 1e-12 * T0


def test_cyclic_pairs_become_internal_faces(oracle):
    """addressing() folds a cyclic pair as the solver does: the CPU restatement's orig_face is the mesh face each of its faces was made from"""
    box = (1.0, 0.8, 1.2)
    mesh = pm.make_cyclic(pm.hex_block(5, 4, 3, box, pm.wavy_periodic(0.02, box)), [(0, 1)])
    ad = lh.addressing(mesh)
    geo, orig = geometry(oracle, mesh)
    assert ad["nei"].size == len(mesh["neighbour"]) + 4 * 3 and ad["own"].size == len(mesh["owner"]) - 4 * 3
    np.testing.assert_array_equal(ad["orig_face"], orig.astype(int))
    assert geo["w"].size == ad["nei"].size and geo["magSf"].size == ad["own"].size and sorted(set(ad["patch_of"])) == [2, 3, 4, 5]
