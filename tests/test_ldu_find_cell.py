"""mesh.findCell on general polyhedral meshes (k_ldu_find_cell, point-force mode of fy_ldu_solver) against tests/find_cell_ref.py: OpenFOAM's face-fan tetrahedra in
numpy long double, written from the mesh dictionary alone.  Per mesh about 6 000 records at once: uniform points (some outside), vertices, face centres and edge
midpoints exact and jittered by 1e-12 and 1e-9 of the cell size, points just off interior faces, points 1e-6 of the cell size inside and outside boundary faces
(cyclic halves among them), cell centres, a NaN, a record 100 box lengths away.

    decidedly inside  (a tetrahedron holds the point at tolerance 0):      found == 1 and the cell read back is in cells_of(x, 1e-9)
    decidedly outside (no tetrahedron holds it at tolerance 1e-9):         found == -1, cell -1, exact zero force
    in between (free; at most 2 % of a case, asserted from the reference): either, but a cell that is given must be in cells_of(x, 1e-9)

The cell is read back with LduSolver.particle_cells(); the Stokes drag of a found particle is 3 pi d nu rho (U[cell] - v) of THAT cell at 1e-10 (the bar of
test_ldu_parity.py::test_point_force_coupling_on_a_general_mesh).  Meshes of at most 1 000 cells; tests/test_find_cell_ref.py holds the reference and these inputs to
properties without a device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import find_cell_ref as fr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("name", list(fr.MESHES))
def test_find_cell_matches_the_tet_reference(product, oracle, name):
    mesh, warped, ref, X, h = fr.case(oracle, name)
    n = X.shape[0]
    # ---- what the reference says of the inputs, before any device call
    pairs, n_adm, d_in, d_out = ref.classify(X)
    free = ~d_in & ~d_out
    assert mesh["n_cells"] <= 1000 and free.mean() <= 0.02, free.mean()
    assert (n_adm > 1).sum() >= 500 and d_out.sum() >= 200
    if warped:
        assert (d_in & ~ref.admissible(pairs, ref.nearest_centre(np.nan_to_num(X)), n)).sum() >= 100
    # ---- the device
    npatch = len(mesh["patch_start"])
    nu, rho = 0.01, 1000.0
    u_val = [(0, 0, 0)] * npatch
    u_val[3] = (1.0, 0, 0)
    s = product.LduSolver(mesh, 1e-3, nu, fr.U_BC.get(name, [0] * npatch), u_val, [0] * npatch, rho_f=rho)
    U0 = np.random.RandomState(4).rand(mesh["n_cells"], 3) * 0.2
    s.set("U", U0)
    rs = np.random.RandomState(5)
    rec = np.zeros((n, 10))
    rec[:, 0:3] = X
    rec[:, 3:9] = rs.standard_normal((n, 6)) * 0.1
    rec[:, 9] = 0.05 * h
    s.set_particles(rec)
    s.step()                                              # (the forces are formed from the U the step starts with)
    cells, found, F = s.particle_cells(), s.found(), s.forces()
    s.set("U", U0)
    s.set_particles(rec)
    s.step()
    cells2, found2 = s.particle_cells(), s.found()
    s.close()
    ok_cell = ref.admissible(pairs, np.where(cells >= 0, cells, 0), n) & (cells >= 0)
    lost, wrong, ghosts = d_in & (found != 1), (cells >= 0) & ~ok_cell, d_out & (found != -1)
    print("find_cell %s: %d records, %d decidedly inside, %d outside, %d free; lost inside %d, in a cell that does not hold them %d, found outside %d"
          % (name, n, d_in.sum(), d_out.sum(), free.sum(), lost.sum(), wrong.sum(), ghosts.sum()))
    assert cells.dtype == np.int32 and np.all((found == 1) | (found == -1)) and np.array_equal(found == 1, cells >= 0) and cells.max() < mesh["n_cells"]
    assert not lost.any(), "particles inside the mesh that findCell lost: %r" % (X[lost][:5],)
    assert not wrong.any(), "particles in a cell none of whose tetrahedra holds them: %r" % (X[wrong][:5],)
    assert not ghosts.any(), "particles outside the mesh that were given a cell: %r" % (X[ghosts][:5],)
    hit = cells >= 0
    drag = 3 * np.pi * (2 * rec[hit, 9:10]) * nu * rho * (U0[cells[hit]] - rec[hit, 3:6])
    np.testing.assert_allclose(F[hit, 0:3], drag, rtol=1e-10, atol=1e-16)
    assert np.all(F[~hit] == 0.0)
    assert np.array_equal(cells, cells2) and np.array_equal(found, found2)


def test_particle_cells_needs_particles_and_a_step(product):
    """before the first step, and between set_particles and the step that locates those particles, the read-out is refused by name -- never a buffer nobody has written"""
    import poly_meshes as pm
    s = product.LduSolver(pm.hex_block(4, 4, 4), 1e-3, 0.01, [0] * 6, [(0, 0, 0)] * 6, [0] * 6)
    rec = np.zeros((5, 10))
    rec[:, 0:3] = np.linspace(0.1, 0.9, 5)[:, None]
    rec[:, 9] = 0.01

    def refused():
        with pytest.raises(product.FoamYadeError) as e:
            s.particle_cells()
        assert "fy_ldu_solver_get_particle_cells_host" in str(e.value)

    refused()
    s.step()
    assert s.particle_cells().shape == (0,)               # (a step has located the empty set)
    s.set_particles(rec)
    refused()
    s.step()
    first = s.particle_cells()
    assert first.shape == (5,) and np.all(first >= 0)
    s.set_particles(rec[:3])
    refused()
    s.step()
    assert np.array_equal(s.particle_cells(), first[:3])
    s.close()


def test_particle_cells_is_refused_by_name_in_gaussian_mode(product):
    import poly_meshes as pm
    s = product.LduSolver(pm.hex_block(4, 4, 4), 1e-3, 0.01, [0] * 6, [(0, 0, 0)] * 6, [2] * 6, solver=1, g=(0, 0, -9.81))
    rec = np.zeros((3, 10))
    rec[:, 0:3] = 0.5
    rec[:, 9] = 0.01
    s.set_particles(rec)
    s.step()
    with pytest.raises(product.FoamYadeError) as e:
        s.particle_cells()
    assert "fy_ldu_solver_get_particle_cells_host" in str(e.value) and "Gaussian" in str(e.value)
    s.close()


def test_find_cell_with_the_hint_from_a_short_stack():
    """the cases once more in a child interpreter under FOAMYADE_LOCATE_STACK=2 (the switch is read when the library is loaded).  The switch shortens the DFS stack of
    the Gaussian locate's explicit-tree walk (k_locate); the point-force hint is k_nearest_cell, whose private stack reads no option, so this run repeats the same
    device path in a fresh process: it holds the answers to be the same there, and would notice the day the hint moves to the walk the switch reaches"""
    env = dict(os.environ, FOAMYADE_LOCATE_STACK="2")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "-k", "matches_the_tet_reference"],
                       env=env, cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout
