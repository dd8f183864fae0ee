"""The selectable drag closures (fy_set_drag_law: Di Felice, Koch-Hill, Beetstra; Schiller-Naumann in point mode) and the Saffman-Mei lift
(FY_FORCE_SAFFMAN_MEI_LIFT) against their numpy restatement (tests/force_laws_ref.py, written from the formulas): the library's own stencils and void
fraction go in, forces and the momentum sources must come out.  Law 0 is the reference's, bit for bit."""
import numpy as np
import pytest

import force_laws_ref as ref
import golden_cases as gc
import golden_util as gu
import poly_meshes as pm

pytestmark = pytest.mark.gpu

MUTABLE = ("uSourceDrag", "alpha", "uSource", "uParticle")


def assert_close(a, b, rtol, what):
    scale = np.abs(b).max() + 1e-300
    np.testing.assert_allclose(a, b, rtol=rtol, atol=rtol * 1e-3 * scale, err_msg=what)


def fresh(Nc):
    return dict(uSourceDrag=np.zeros(Nc), alpha=np.zeros(Nc), uSource=np.zeros((Nc, 3)), uParticle=np.zeros((Nc, 3)))


def engine(product, c, fields, mut):
    """the coupling object of a golden case: a uniform block, or (graded cases) the general mesh of its centres and volumes"""
    if gc.is_graded(c):
        P = gc.mesh_points(c)
        mesh = product.GeneralMesh(gc.cell_centres(c), gc.cell_volumes(c), P.min(axis=0), P.max(axis=0))
    else:
        mesh = product.BlockMesh(c.nx, c.ny, c.nz, c.dx, c.origin)
    fy = product.FoamYade(mesh, fields["U"], fields["gradP"], fields["vGrad"], fields["divT"], fields["ddtU"], c.g,
                          mut["uSourceDrag"], mut["alpha"], mut["uSource"], mut["uParticle"], bool(c.gaussian))
    fy.setScalarProperties(c.rhoP, c.rhoF, c.nu)
    return fy


def batches_of(c, rec):
    off = gu.batch_offsets(c, rec.shape[0])
    return [rec[off[b]:off[b + 1]] for b in range(len(off) - 1)]


def run(fy, c, rec):
    """one setParticleAction on a clean slate; returns (forces, per-batch stencils)"""
    fy.setSourceZero()
    bs = batches_of(c, rec)
    fy.setParticles(bs)
    fy.setParticleAction(c.dt)
    return np.concatenate([fy.forces(b) for b in range(len(bs))]), [fy.stencils(b) for b in range(len(bs))]


def restate(c, rec, stencils, fields, mut, law, models):
    """forces, uSourceDrag and uSource of one call, batch after batch as FoamYade.C:612-628 walks them.  Each batch's force pass sees the void fraction its own
    deposit left: the last batch's is the mutated field itself, an earlier one's is rebuilt from the stencils (and must arrive at the mutated field in the end)"""
    V = gc.cell_volumes(c)
    alpha, uP = np.ones(c.ncells), np.zeros((c.ncells, 3))
    D, S, F, diag = np.zeros(c.ncells), np.zeros((c.ncells, 3)), [], []
    bs = batches_of(c, rec)
    for b, (r, (k, ids, w, chain)) in enumerate(zip(bs, stencils)):
        ref.deposit(r, ids, w, V, alpha, uP)
        if b == len(bs) - 1:
            assert_close(alpha, mut["alpha"], gu.RTOL_GPU, "replayed alpha"); assert_close(uP, mut["uParticle"], gu.RTOL_GPU, "replayed uParticle")
            alpha, uP = mut["alpha"].copy(), mut["uParticle"].copy()
        f, d, s, dg = ref.gaussian_batch(law, models, r, ids, w, fields, alpha, uP, V, c.rhoF, c.rhoP, c.nu, c.dt)
        F.append(f); D += d; S += s; diag.append(dg)
    return np.concatenate(F), D, S, dict(eps=np.concatenate([d["eps"] for d in diag]), Re=np.concatenate([d["Re"] for d in diag]))


def dense_cluster_case():
    """an 8^3 block with a packed cluster: void fractions down to the floor, next to dilute cells"""
    return gc.Case("g8_dense", 8, 8, 8, 0.1, np_=300, seed=91, cluster=400, fast=10)


GAUSSIAN_INPUTS = ["g8_serial", "g9x7x5_odd", "g16x12x10_graded", "g16_parallel3", "g8_dense"]


def inputs_of(name):
    if name == "g8_dense":
        c = dense_cluster_case()
        return c, gc.fluid_fields(c), gc.particle_records(c, 0)
    c = gc.CASES_BY_NAME[name]
    return c, gc.fluid_fields(c), gu.load(name)["records_s0"]


@pytest.mark.parametrize("name", GAUSSIAN_INPUTS)
def test_gaussian_laws_match_the_restatement(product, name):
    c, fields, rec = inputs_of(name)
    mut = fresh(c.ncells)
    fy = engine(product, c, fields, mut)
    seen_phi = []
    for law in (product.DRAG_DI_FELICE, product.DRAG_KOCH_HILL, product.DRAG_BEETSTRA, product.DRAG_REFERENCE):
        fy.setDragLaw(law)
        F, st = run(fy, c, rec)
        chain = np.concatenate([s[3] for s in st])
        Fr, D, S, dg = restate(c, rec, st, fields, mut, law, 0)
        ok = chain <= 12
        assert ok.mean() > 0.9 and np.isfinite(Fr[ok]).all()
        assert_close(F[ok], Fr[ok], gu.RTOL_GPU, f"force, law {law}")
        assert_close(mut["uSourceDrag"], D, gu.RTOL_GPU, f"uSourceDrag, law {law}")
        assert_close(mut["uSource"], S, gu.RTOL_GPU, f"uSource, law {law}")
        seen_phi.append(1.0 - dg["eps"])
    fy.close()
    if name == "g8_dense":                   # this input is built to put particles on both sides of Koch-Hill's switch at phi = 0.4, whatever the goldens do
        phi = seen_phi[1]
        assert (phi < 0.4).sum() >= 10 and (phi >= 0.4).sum() >= 10, ((phi < 0.4).sum(), (phi >= 0.4).sum())


def isolated_cloud():
    """27 particles 11 cells apart on a 32^3 block: a stencil reaches at most sqrt(1.25) * interpRange = 4.5 cells (meshTree.C:155), so no cell hears from two
    particles and every per-cell sum of the call has ONE term.  The scatters add through atomics, whose order changes from run to run -- with several terms per cell
    two runs of the SAME code differ in the last bits of the fields and, through alpha, of the forces; with one term they are reproducible and 'bit for bit' can be
    asked of them.  Radii and speeds put particles on both sides of the law's switches: alpha_f = 0.8 (Wen-Yu / Ergun) and Re = 1000"""
    c = gc.Case("isolated", 32, 32, 32, 0.1, seed=93)
    rs = np.random.RandomState(c.seed)
    cells = np.array([(i, j, k) for k in (4, 15, 26) for j in (4, 15, 26) for i in (4, 15, 26)], dtype=np.float64)
    rec = np.zeros((27, 10))
    rec[:, 0:3] = (cells + 0.05 + 0.9 * rs.random_sample((27, 3))) * c.dx
    rec[:, 3:6] = (rs.random_sample((27, 3)) * 2 - 1) * np.where(np.arange(27) % 3 == 0, 2.5, 0.1)[:, None]
    rec[:, 6:9] = (rs.random_sample((27, 3)) * 2 - 1) * 0.1
    rec[:, 9] = np.where(np.arange(27) % 2 == 0, 1.0, 0.2) * c.dx
    return c, gc.fluid_fields(c), rec


def assert_one_term_per_cell(st, ncells):
    ids = st[0][1]
    assert np.bincount(ids[ids >= 0], minlength=ncells).max() == 1


@pytest.mark.parametrize("gaussian", [1, 0])
def test_law_zero_is_the_default_bit_for_bit(product, gaussian):
    if gaussian:
        c, fields, rec = isolated_cloud()
    else:
        c = gc.CASES_BY_NAME["p32_serial_c1"]
        fields, rec = gc.fluid_fields(c), gu.load(c.name)["records_s0"]
    other = product.DRAG_KOCH_HILL if gaussian else product.DRAG_SCHILLER_NAUMANN
    out = []
    for calls in ((), (product.DRAG_REFERENCE,), (other,), (other, product.DRAG_REFERENCE)):
        mut = fresh(c.ncells)
        fy = engine(product, c, fields, mut)
        for law in calls:
            fy.setDragLaw(law)
        F, st = run(fy, c, rec)
        if len(calls) == 2:                                                   # one object: law 2 (4) for a call, then back
            fy.setDragLaw(calls[0]); run(fy, c, rec)
            fy.setDragLaw(calls[1]); F, st = run(fy, c, rec)
        out.append((F, {nm: mut[nm].copy() for nm in MUTABLE}))
        if gaussian:
            assert_one_term_per_cell(st, c.ncells)
            eps = np.array([(st[0][2][q] * mut["alpha"][np.maximum(st[0][1][q], 0)]).sum() for q in range(rec.shape[0])])
            Re = 1e-9 + np.linalg.norm(np.array([(st[0][2][q][:, None] * fields["U"][np.maximum(st[0][1][q], 0)]).sum(axis=0) for q in range(27)]) - rec[:, 3:6], axis=1) * 2 * rec[:, 9] / c.nu
            assert (eps > 0.8).sum() >= 3 and (eps <= 0.8).sum() >= 3 and (Re < 1000).sum() >= 3 and (Re > 1000).sum() >= 3
        fy.close()
    base = out[0]
    assert np.abs(base[0]).max() > 0
    for F, m in (out[1], out[3]):
        assert np.array_equal(F, base[0])
        for nm in MUTABLE:
            assert np.array_equal(m[nm], base[1][nm]), nm
    assert not np.array_equal(out[2][0], base[0])


def test_dilute_limit_is_stokes(product):
    """one particle, phi ~ 1e-6, Re ~ 1e-4, uniform stream, no pressure gradient: |F| / (3 pi rho nu d m) -> 1 for Koch-Hill and Beetstra (leading corrections
    3 sqrt(phi / 2) ~ 2e-3 and 1.5 sqrt(phi) ~ 1.5e-3) and -> (0.63 + 480)^2 / 240000 = 0.9625 for Di Felice (Re Cd / 24 at Re = 1e-4)"""
    c = gc.Case("dilute", 8, 8, 8, 0.1, nu=1e-3, rhoF=1000.0)
    d = 0.0215 * c.dx
    m = 1e-4 * c.nu / d
    fields = dict(U=np.tile([m, 0.0, 0.0], (c.ncells, 1)), gradP=np.zeros((c.ncells, 3)), divT=np.zeros((c.ncells, 3)), ddtU=np.zeros((c.ncells, 3)),
                  vGrad=np.zeros((c.ncells, 9)))
    rec = np.zeros((1, 10)); rec[0, 0:3] = 0.05 + 0.3 * c.dx; rec[0, 9] = 0.5 * d
    mut = fresh(c.ncells)
    fy = engine(product, c, fields, mut)
    stokes = 3 * np.pi * c.rhoF * c.nu * d * m
    for law, limit in ((product.DRAG_KOCH_HILL, 1.0), (product.DRAG_BEETSTRA, 1.0), (product.DRAG_DI_FELICE, 0.9625)):
        fy.setDragLaw(law)
        F, st = run(fy, c, rec)
        phi = 1.0 - (st[0][2][0] * mut["alpha"][np.maximum(st[0][1][0], 0)]).sum()
        assert 2e-7 < phi < 5e-6, phi
        ratio = np.linalg.norm(F[0, :3]) / stokes
        assert abs(ratio - limit) < 1e-2, (law, ratio)
        assert F[0, 1] == 0.0 and F[0, 2] == 0.0
    fy.close()


def find_cell(c, rec):
    """the uniform block's findCell stand-in: inside the closed bounding box, floor((p - min) / dx) clamped"""
    o = np.array(c.origin); n = np.array([c.nx, c.ny, c.nz])
    p = rec[:, 0:3]
    inside = np.all((p >= o) & (p <= o + n * c.dx), axis=1)
    ijk = np.minimum(((p - o) / c.dx).astype(np.int64), n - 1)
    return np.where(inside, ijk[:, 0] + c.nx * (ijk[:, 1] + c.ny * ijk[:, 2]), -1)


@pytest.mark.parametrize("name", ["p32_serial_c1", "p20x12x8_parallel4", "p8_fast"])
def test_schiller_naumann_in_point_mode(product, name):
    if name == "p8_fast":                    # the goldens stay below Re = 10: a seeded 8^3 case whose fast particles pass Re = 1000
        c = gc.Case("p8_fast", 8, 8, 8, 0.1, gaussian=0, np_=200, seed=92, fast=60, nu=1e-5)
        rec = gc.particle_records(c, 0)
    else:
        c = gc.CASES_BY_NAME[name]
        rec = gu.load(name)["records_s0"]
    fields = gc.fluid_fields(c)
    mut = fresh(c.ncells)
    fy = engine(product, c, fields, mut)
    F0, _ = run(fy, c, rec)
    fy.setDragLaw(product.DRAG_SCHILLER_NAUMANN)
    F, _ = run(fy, c, rec)
    found = np.concatenate([fy.found(b) for b in range(len(batches_of(c, rec)))])
    cell = find_cell(c, rec)
    assert np.array_equal(found == 1, cell >= 0)
    Fr, S, Re = ref.point_batch(ref.SCHILLER_NAUMANN, rec, cell, fields["U"], gc.cell_volumes(c), c.rhoF, c.nu)
    assert_close(F[:, :3], Fr, gu.RTOL_GPU, "Schiller-Naumann drag")
    assert_close(mut["uSource"], S, gu.RTOL_GPU, "uSource")
    assert np.array_equal(F[:, 3:], F0[:, 3:])                                # stokesDragTorque is not the drag law's business
    Fs, _, _ = ref.point_batch(ref.REFERENCE, rec, cell, fields["U"], gc.cell_volumes(c), c.rhoF, c.nu)
    assert_close(F0[:, :3], Fs, gu.RTOL_GPU, "Stokes drag")
    if name == "p8_fast":
        assert (Re < 1000).sum() >= 10 and (Re > 1000).sum() >= 10, ((Re < 1000).sum(), (Re > 1000).sum())
    fy.close()


def test_laws_of_the_other_mode_are_refused(product):
    for name, bad, good in (("p16_parallel2", (1, 2, 3, 99, -1), (0, 4)), ("g8_serial", (4, 99, -1), (0, 1, 2, 3))):
        c = gc.CASES_BY_NAME[name]
        fy = engine(product, c, gc.fluid_fields(c), fresh(c.ncells))
        for law in bad:
            with pytest.raises(product.FoamYadeError) as e:
                fy.setDragLaw(law)
            assert "error 1" in str(e.value) and "FY_DRAG_REFERENCE" in str(e.value)
            assert ("FY_DRAG_SCHILLER_NAUMANN" in str(e.value)) == (not c.gaussian) and ("FY_DRAG_BEETSTRA" in str(e.value)) == bool(c.gaussian)
        for law in good:
            fy.setDragLaw(law)
        fy.close()
    c = gc.CASES_BY_NAME["p16_parallel2"]
    fy = engine(product, c, gc.fluid_fields(c), fresh(c.ncells))
    with pytest.raises(product.FoamYadeError):
        fy.setForceModels(product.FORCE_SAFFMAN_MEI_LIFT)
    fy.close()


@pytest.mark.parametrize("name,law", [("g8_serial", 0), ("g16_parallel3", 3), ("g16x12x10_graded", 2)])
def test_lift_matches_the_restatement(product, name, law):
    c, fields, rec = inputs_of(name)
    mut = fresh(c.ncells)
    fy = engine(product, c, fields, mut)
    fy.setDragLaw(law)
    F_off, _ = run(fy, c, rec)
    for models in (product.FORCE_SAFFMAN_MEI_LIFT, product.FORCE_SAFFMAN_MEI_LIFT | product.FORCE_GAUSSIAN_TORQUE | product.FORCE_ADDED_MASS):
        fy.setForceModels(models)
        F, st = run(fy, c, rec)
        ok = np.concatenate([s[3] for s in st]) <= 12
        Fr, D, S, _ = restate(c, rec, st, fields, mut, law, models)
        assert_close(F[ok][:, :3], Fr[ok][:, :3], gu.RTOL_GPU, f"force, models {models}")
        assert_close(F[ok][:, 3:], Fr[ok][:, 3:], gu.RTOL_GPU, f"torque, models {models}")
        assert_close(mut["uSource"], S, gu.RTOL_GPU, f"uSource, models {models}")
        assert_close(mut["uSourceDrag"], D, gu.RTOL_GPU, f"uSourceDrag, models {models}")
    lift = np.abs(F[ok][:, :3] - F_off[ok][:, :3]).max()
    assert lift > 1e-6 * np.abs(F_off[ok]).max()                              # the golden vGrad is sheared: the lift is there
    fy.close()


def test_lift_without_shear_is_exactly_zero(product):
    """vGrad = 0: the forces (and uSource) of a run with the lift on equal the lift-off run's exactly, and nothing is NaN although Re_w = 0 and, for one particle
    at rest in its fluid, Re_p = 0 too.  On the cloud whose sums have one term per cell (isolated_cloud): there two runs are reproducible bit for bit"""
    c, fields, rec = isolated_cloud()
    fields = dict(fields, U=np.zeros_like(fields["U"]), vGrad=np.zeros_like(fields["vGrad"]))            # a fluid at rest ...
    rec[5, 3:6] = 0.0                                                                                   # ... and one particle at rest in it: u_r = 0 exactly
    out = []
    for models in (0, product.FORCE_SAFFMAN_MEI_LIFT):
        mut = fresh(c.ncells)
        fy = engine(product, c, fields, mut)
        fy.setForceModels(models)
        F, st = run(fy, c, rec)
        assert_one_term_per_cell(st, c.ncells)
        out.append((F, mut["uSource"].copy()))
        fy.close()
    assert np.isfinite(out[1][0]).all() and np.isfinite(out[1][1]).all() and np.abs(out[0][0]).max() > 0
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_lift_needs_vgrad_on_slabs_too(product):
    """pimpleFoamYade, 8 x 8 x 16, two steps with Beetstra + lift: two z-slabs against the single domain at tests/test_slabs.py's bar for its coupled runs
    (forces 1e-6, fields 1e-5 of the largest value).  The start velocity is sheared across the slab interface, so the lift there reads vGrad's ghost planes"""
    n, nz = 8, 16
    dx = 0.1 / n
    case = product.make_case(1, n, n, nz, dx, 2e-4, 1e-5, u_bc=[0] * 6, u_val=[(0, 0, 0)] * 6, g=(0, 0, -9.81), p_bc=[2] * 6)
    one = product.Solver(case); many = product.VirtualSlabs(case, 2)
    models = product.FORCE_SAFFMAN_MEI_LIFT
    for s in [one] + many.solvers:
        s.set_drag_law(product.DRAG_BEETSTRA); s.set_force_models(models)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(n), np.arange(n), indexing="ij")
    z, y = (k.ravel() + 0.5) * dx, (j.ravel() + 0.5) * dx
    U0 = np.stack([0.3 * np.sin(np.pi * z / (nz * dx)) ** 2 * np.sin(np.pi * y / (n * dx)), np.zeros_like(z), 0.05 * np.sin(2 * np.pi * y / (n * dx)) * np.sin(np.pi * z / (nz * dx))], axis=1)
    one.set("U", U0); many.set("U", U0)
    gcase = gc.Case("s", n, n, nz, 0.1, gaussian=1, np_=1900, seed=33, cluster=100, vel_scale=0.05)
    plain = None
    for step in range(2):
        rec = gc.particle_records(gcase, step)
        rec = rec[(rec[:, 2] > 0) & (rec[:, 2] < nz * dx)]
        one.set_particles(rec); many.set_particles(rec)
        one.step(); many.step()
        fo, fm = one.forces(), many.forces()
        sc = np.abs(fo[:, :3]).max()
        assert sc > 0 and np.abs(fm[:, :3] - fo[:, :3]).max() <= 1e-6 * sc, np.abs(fm[:, :3] - fo[:, :3]).max() / sc
        if step == 0:
            plain = fo.copy()
    for nm in ("U", "p", "alpha", "uSource"):
        x, y_ = many.get(nm), one.get(nm)
        sc = np.abs(y_).max() + 1e-300
        assert np.abs(x - y_).max() <= 1e-5 * sc, (nm, np.abs(x - y_).max() / sc)
    many.close(); one.close()
    # the lift is a visible share of the first step's forces (else the comparison above would not see a missing halo)
    ref_solver = product.Solver(case)
    ref_solver.set_drag_law(product.DRAG_BEETSTRA)
    ref_solver.set("U", U0)
    rec = gc.particle_records(gcase, 0)
    rec = rec[(rec[:, 2] > 0) & (rec[:, 2] < nz * dx)]
    ref_solver.set_particles(rec); ref_solver.step()
    near = np.abs(rec[:, 2] - 0.5 * nz * dx) < 2 * dx                        # particles whose stencils cross the interface
    assert np.abs(plain[near, :3] - ref_solver.forces()[near, :3]).max() > 1e-4 * np.abs(plain[:, :3]).max()
    ref_solver.close()


def ldu_stencils(product, s):
    n = s._batch_n[0]
    k = np.zeros(n, np.int32); ids = np.full((n, product.MAXK), -1, np.int32); w = np.zeros((n, product.MAXK)); chain = np.zeros(n, np.int32)
    product._check(product.lib().fy_get_stencils_host(s._cpl, 0, product._i(k), product._i(ids), product._d(w), product._i(chain)))
    return k, ids, w, chain


def test_koch_hill_on_a_general_mesh(product):
    """fy_ldu_solver (pimpleFoamYade) on the smallest lattice of tests/poly_meshes.py with Koch-Hill.
    (a) With a cloud of its own, the forces and uSourceDrag of its coupling object equal the restatement on the stencils that object reports: law and flags work on
    the general mesh's coupling unchanged.
    (b) Against fy_solver on the same block, in tests/test_ldu_parity.py's pairing and at its bar (1e-6 of the largest value, U and p): fy_solver runs the cloud
    with Koch-Hill, the general-mesh solver is fed the void fraction and the sources that produced.  The pairing feeds them because the two k-d trees break the
    ties of a lattice's centres differently, so one cloud takes other improvement chains in the two solvers; measured here with each solver running the cloud
    itself (one step, this cloud): U differs by 0.99 of its largest value (4e-3 m/s, all of it made by the cloud), p by 0.08 -- the tree, not the law"""
    n, box = 10, 0.1
    dx = box / n
    mesh = pm.hex_block(n, n, n, (box, box, box))
    kw = dict(p_tol=1e-11, p_rel_tol=0.0, p_final_tol=1e-11, u_tol=1e-11)
    case = product.make_case(1, n, n, n, dx, 2e-4, 1e-5, g=(0, 0, -9.81), p_bc=[2] * 6, p_solver=0, n_outer_correctors=1, n_correctors=2, p_max_iter=5000, **kw)
    mk = lambda: product.LduSolver(mesh, 2e-4, 1e-5, [0] * 6, [(0, 0, 0)] * 6, [2] * 6, solver=1, g=(0, 0, -9.81), n_outer_correctors=1, n_correctors=2, p_max_iter=5000, **kw)
    f, h, fed = product.Solver(case), mk(), mk()
    for s in (f, h, fed):
        s.set_drag_law(product.DRAG_KOCH_HILL); s.hold_sources(True)
    with pytest.raises(product.FoamYadeError):
        h.set_drag_law(product.DRAG_SCHILLER_NAUMANN)
    rs = np.random.RandomState(17)
    rec = np.zeros((2000, 10))
    rec[:, 0:3] = rs.random_sample((2000, 3)) * np.array([box, box, 0.6 * box]) + np.array([0.0, 0.0, 0.05 * box])
    rec[:, 3:6] = 0.05 * rs.standard_normal((2000, 3))
    rec[:, 9] = 0.2 * dx
    f.set_particles(rec); h.set_particles(rec)
    f.step(); h.step()
    # (a) U, p were zero before the step, so the force pass interpolated U = 0, gradP = 0, divT = 0
    k, ids, w, chain = ldu_stencils(product, h)
    V = np.full(n ** 3, dx ** 3)
    zero3 = np.zeros((n ** 3, 3))
    fields = dict(U=zero3, gradP=zero3, divT=zero3, ddtU=zero3, vGrad=np.zeros((n ** 3, 9)))
    Fr, D, S, dg = ref.gaussian_batch(ref.KOCH_HILL, 0, rec, ids, w, fields, h.get("alpha"), h.get("uParticle").reshape(-1, 3), V, 1000.0, 2650.0, 1e-5, 2e-4)
    ok = chain <= 12
    assert ok.mean() > 0.9 and np.abs(Fr[ok]).max() > 0
    assert_close(h.forces()[ok][:, :3], Fr[ok][:, :3], gu.RTOL_GPU, "Koch-Hill on the general mesh")
    assert_close(h.get("uSourceDrag"), D, gu.RTOL_GPU, "uSourceDrag on the general mesh")
    # (b)
    assert f.get("alpha").min() < 0.9
    fed.set("alpha", f.get("alpha")); fed.set("uSourceDrag", f.get("uSourceDrag")); fed.set("uSource", f.get("uSource"))
    fed.step()
    Uf, Uh = f.get("U").reshape(-1, 3), fed.get("U").reshape(-1, 3)
    assert np.abs(Uf).max() > 1e-4 and np.abs(Uh - Uf).max() <= 1e-6 * np.abs(Uf).max(), np.abs(Uh - Uf).max() / np.abs(Uf).max()
    pf, ph = f.get("p"), fed.get("p")
    pf, ph = pf - pf.mean(), ph - ph.mean()
    assert np.abs(ph - pf).max() <= 1e-6 * np.abs(pf).max(), np.abs(ph - pf).max() / np.abs(pf).max()
    f.close(); h.close(); fed.close()
