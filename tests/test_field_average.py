"""Device-side fieldAverage (fy_solver_set_field_average, fy_ldu_solver_set_field_average, controlDict functions): the running means and prime2Means a solver
keeps equal tests/field_average_ref.py fed the same per-step fields BIT FOR BIT -- the kernel performs the restatement's IEEE operations, uncontracted -- and
the closed forms at 1e-12 of the data's scale (n eps = 2e-15 apart; three decades of room).  The per-step fields are read with hold_sources(True), after the
step and before the next: what stood where runTime.write() stands, which is where the sample is taken."""
import os
import re
import subprocess

import numpy as np
import pytest

import field_average_ref as far
import poly_meshes as pm
from field_average_cases import KINDS, ON, add_functions, case_copy, field_average, open_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = {"U": 3, "uParticle": 3, "uSource": 3}            # components; every other field is a scalar


def shape_of(name, n):
    return (n, 3) if SHAPES.get(name) == 3 else (n,)


def read_fields(s, names, n, source="uSource"):
    """this step's fields as the sample saw them (LduSolver keeps the coupling's uSource under its own name)"""
    return {nm: s.get(source if nm == "uSource" else nm).reshape(shape_of(nm, n)) for nm in names}


def assert_averages(s, ref, history, dts, label=""):
    """the solver's means / prime2Means against the restatement (exactly) and, where the whole history is given, against the closed forms"""
    for q, (nm, item) in enumerate(ref.items()):
        m = s.get(nm + "Mean").reshape(item.m.shape)
        np.testing.assert_array_equal(m, item.m, err_msg=f"{label}{nm}Mean")
        assert s.average_state(q) == (item.N, item.T), (label, nm, s.average_state(q), item.N, item.T)
        if item.prime2:
            P = s.get(nm + "Prime2Mean").reshape(item.P.shape)
            np.testing.assert_array_equal(P, item.P, err_msg=f"{label}{nm}Prime2Mean")
        if history is not None:
            xs = [h[nm] for h in history]
            cm, cP = far.closed_form(xs, dts, item.base)
            scale = max(np.abs(x).max() for x in xs) + 1e-300
            assert np.abs(m - cm).max() <= 1e-12 * scale, (label, nm, np.abs(m - cm).max() / scale)
            if item.prime2:
                assert np.abs(P - cP).max() <= 1e-12 * scale ** 2, (label, nm, np.abs(P - cP).max() / scale ** 2)


def run_against_restatement(s, items, n, steps, particles=None, source="uSource", label=""):
    """items: (field, prime2[, base]) as handed to set_field_average.  Steps the solver, feeding the restatement what each step left; returns (ref, history, dts)"""
    ref = {it[0]: far.Item(shape_of(it[0], n), bool(it[1]), it[2] if len(it) > 2 else "time") for it in items}
    history, dts = [], []
    s.hold_sources(True)
    for step in range(steps):
        if particles is not None:
            s.set_particles(particles(step))
        s.step()
        dt = s.stats()["delta_t"]
        x = read_fields(s, ref, n, source)
        for nm, item in ref.items():
            item.add(x[nm], dt)
        history.append(x); dts.append(dt)
    assert_averages(s, ref, history, dts, label)
    return ref, history, dts


def bed_cloud(lo, hi, count, radius, seed):
    """a settling cloud in the box [lo, hi], moved a little each step"""
    rs = np.random.RandomState(seed)
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    base = np.zeros((count, 10))
    base[:, 0:3] = lo + (hi - lo) * rs.random_sample((count, 3))
    base[:, 3:6] = 0.05 * rs.standard_normal((count, 3))
    base[:, 9] = radius
    jitter = [0.02 * (hi - lo) * (rs.random_sample((count, 3)) - 0.5) for _ in range(16)]

    def at(step):
        rec = base.copy()
        rec[:, 0:3] = np.clip(base[:, 0:3] + jitter[step % 16], lo, hi)
        rec[:, 2] -= 2e-4 * step
        return rec
    return at


def test_block_pimple_bed(product):
    """6 x 6 x 10 bed box, 300 particles moved each step, 6 steps: U, p, alpha with both moments, uParticle's mean"""
    nx, ny, nz, dx = 6, 6, 10, 0.01
    n = nx * ny * nz
    s = product.Solver(product.make_case(1, nx, ny, nz, dx, 2e-4, 1e-5, g=(0, 0, -9.81), p_bc=[2] * 6))
    items = [("U", True), ("p", True), ("alpha", True), ("uParticle", False)]
    s.set_field_average(items)
    with pytest.raises(product.FoamYadeError):
        s.get("nutMean")                                   # laminar: no nut, so no nut average either
    cloud = bed_cloud((0.005, 0.005, 0.005), (0.055, 0.055, 0.05), 300, 0.2 * dx, 3)
    ref, history, dts = run_against_restatement(s, items, n, 6, cloud)
    assert ref["alpha"].m.min() < 1.0 and np.abs(ref["alpha"].P).max() > 0          # particles were there, and moved: the averages are not those of a constant
    assert np.abs(ref["U"].P).max() > 0 and np.abs(ref["uParticle"].m).max() > 0
    assert s.get("UPrime2Mean").size == 6 * n and s.get("pPrime2Mean").size == n
    with pytest.raises(product.FoamYadeError):
        s.get("uParticlePrime2Mean")                       # mean only
    s.close()


def test_bases_and_window_under_an_adjusted_time_step(product):
    """an iteration-base item beside a time-base item on a lid-driven box whose deltaT grows; start_after skips the first two of six steps, stop_after
    ends the sampling one step early"""
    n, dx = 8, 0.1 / 8
    u_val = [(0, 0, 0)] * 6
    u_val[3] = (1.0, 0, 0)
    mk = lambda: product.Solver(product.make_case(1, n, n, n, dx, 1e-3, 1e-3, u_val=u_val, p_bc=[0] * 6, adjust_time_step=1, max_co=0.5, max_delta_t=1.0))
    probe = mk()
    dts = []
    for _ in range(6):
        probe.step()
        dts.append(probe.stats()["delta_t"])
    probe.close()
    assert len(set(dts)) > 1, dts                           # the steps' deltaT take more than one value
    e = np.cumsum(dts)
    start_after, stop_after = e[2], e[4]                    # the ends of the third and fifth steps
    sampled = [far.in_window(e[k], dts[k], start_after, stop_after) for k in range(6)]
    assert sampled == [False, False, True, True, True, False]
    s = mk()
    items = [("U", True, "iteration"), ("p", True, "time")]
    s.set_field_average(items, start_after=start_after, stop_after=stop_after)
    ref = {it[0]: far.Item(shape_of(it[0], n ** 3), True, it[2]) for it in items}
    s.hold_sources(True)
    kept, kept_dt = [], []
    for k in range(6):
        s.step()
        assert s.stats()["delta_t"] == dts[k]
        if sampled[k]:
            x = read_fields(s, ref, n ** 3)
            for nm, item in ref.items():
                item.add(x[nm], dts[k])
            kept.append(x); kept_dt.append(dts[k])
        assert s.average_state(0)[0] == s.average_state(1)[0] == sum(sampled[:k + 1])
    assert s.average_state(0) == (3, ref["U"].T) and abs(ref["U"].T - (dts[2] + dts[3] + dts[4])) <= 1e-15
    assert_averages(s, ref, kept, kept_dt)
    # the two bases differ where the weights do
    tm, _ = far.closed_form([h["U"] for h in kept], kept_dt, "time")
    assert np.abs(tm - ref["U"].m).max() > 1e-9 * np.abs(tm).max()
    s.close()


def test_turbulence_fields(product):
    """kEpsilon on a 6^3 lid-driven box: the means of k, epsilon and nut"""
    n, dx = 6, 0.1 / 6
    u_val = [(0, 0, 0)] * 6
    u_val[3] = (0.5, 0, 0)
    kw = dict(turbulence_model=3, nut_bc=[0, 0, 1, 0, 0, 1], nut_value=[0, 0, 0.0, 0, 0, 1e-5], nut_initial=2e-5,
              k_bc=[0, 1, 1, 1, 0, 1], k_value=[0, 1e-4, 2e-4, 2e-4, 0, 1e-4], k_initial=5e-4, k_convection_scheme=1, k_tol=1e-9, k_relax=0.9,
              eps_bc=[0, 1, 0, 1, 0, 0], eps_value=[0, 2e-3, 0, 3e-3, 0, 0], eps_initial=2e-3, eps_convection_scheme=0, eps_tol=1e-9, eps_relax=0.8)
    s = product.Solver(product.make_case(1, n, n, n, dx, 2e-4, 1e-5, g=(0, 0, -9.81), u_val=u_val, p_bc=[2] * 6, **kw))
    items = [("k", False), ("epsilon", True), ("nut", False)]
    s.set_field_average(items)
    ref, history, _ = run_against_restatement(s, items, n ** 3, 4)
    assert np.abs(history[-1]["k"] - history[0]["k"]).max() > 0 and np.abs(ref["epsilon"].P).max() > 0
    s.close()


def test_general_mesh_ico(product):
    """icoFoamYade on 4 x 4 x 4 sheared hexahedra, lid-driven: U and p"""
    mesh = pm.hex_block(4, 4, 4, (0.1, 0.1, 0.1), pm.shear(0.2, 0.1, 0.1))
    u_val = [(0, 0, 0)] * 6
    u_val[3] = (1.0, 0, 0)
    s = product.LduSolver(mesh, 0.005, 0.01, [0] * 6, u_val, [0] * 6, n_non_orth=1)
    items = [("U", True), ("p", True, "iteration"), ("uSource", False)]
    s.set_field_average(items)
    ref, _, _ = run_against_restatement(s, items, 64, 5, source="uSourceCoupling", label="ico ")
    assert np.abs(ref["U"].P).max() > 0
    for nm in ("alpha", "uParticle", "nut"):                # icoFoamYade has none of them
        with pytest.raises(product.FoamYadeError) as e:
            s.set_field_average([nm])
        assert "error 1" in str(e.value) and nm in str(e.value)
    s.close()


def test_general_mesh_pimple_bed(product):
    """pimpleFoamYade on the 4 x 4 x 8 general bed with particles: U, alpha, uParticle"""
    mesh = pm.hex_block(4, 4, 8, (0.06, 0.06, 0.12))
    s = product.LduSolver(mesh, 2e-4, 1e-5, [0] * 6, [(0, 0, 0)] * 6, [2] * 6, solver=1, g=(0, 0, -9.81), n_outer_correctors=1, n_correctors=2, p_max_iter=5000)
    items = [("U", True), ("alpha", True), ("uParticle", True)]
    s.set_field_average(items)
    cloud = bed_cloud((0.005, 0.005, 0.005), (0.055, 0.055, 0.06), 300, 0.003, 11)
    ref, _, _ = run_against_restatement(s, items, 128, 6, cloud, source="uSourceCoupling", label="pimple ")
    assert ref["alpha"].m.min() < 1.0 and np.abs(ref["alpha"].P).max() > 0 and np.abs(ref["uParticle"].P).max() > 0
    s.close()


def test_averaging_does_not_perturb_the_run(product, tmp_path):
    """cavity_ico (no particles: deterministic), 10 steps with averaging on and off: identical U, p and fluxes"""
    fc = product.FoamCase(case_copy(tmp_path, "cavity_ico", "block"), 0)
    U0, p0 = fc.initial_fields()
    out = []
    for on in (True, False):
        s = product.Solver(fc.case)
        s.set("U", U0); s.set("p", p0)
        if on:
            s.set_field_average([("U", True), ("p", True), ("uSource", False)])
        for _ in range(10):
            s.step()
        out.append({nm: s.get(nm) for nm in ("U", "p", "phi_x", "phi_y", "phi_z")})
        if on:
            assert s.average_state(0) == (10, pytest.approx(10 * fc.delta_t, rel=1e-14)) and np.abs(s.get("UMean")).max() > 0
            s.set("UMean", np.ones(3 * s.n_cells))                      # writing an average is a plain copy: the flux of U stays
            assert np.array_equal(s.get("phi_x"), out[0]["phi_x"]) and np.array_equal(s.get("UMean"), np.ones(3 * s.n_cells))
            s.set_field_average(None)
            for nm in ("UMean", "UPrime2Mean", "pMean"):
                with pytest.raises(product.FoamYadeError):
                    s.get(nm)
            with pytest.raises(product.FoamYadeError):
                s.average_state(0)
        s.close()
    for nm in out[0]:
        assert np.array_equal(out[0][nm], out[1][nm]), nm
    assert np.abs(out[0]["U"]).max() > 0.1
    fc.close()


def test_refusals(product):
    lam = product.Solver(product.make_case(1, 6, 6, 6, 0.01, 2e-4, 1e-5, p_bc=[2] * 6))
    for items, word in (([("T", True)], "'T'"), (["k"], "'k'"), (["U", ("p", True), "U"], "twice"),
                        (["U", "p", "alpha", "uParticle", "uSource", "nut", "k", "epsilon", "U"], "9 items")):
        with pytest.raises(product.FoamYadeError) as e:
            lam.set_field_average(items)
        assert "error 1" in str(e.value) and word in str(e.value), str(e.value)             # FY_ERR_INVALID, naming the field
        with pytest.raises(product.FoamYadeError):
            lam.get("UMean")                                                                # a refused call leaves averaging off
    lam.set_field_average(["U"])
    assert lam.get("UMean").size == 3 * 216
    lam.close()
    case = product.make_case(0, 8, 8, 16, 0.1 / 8, 0.005, 0.01, p_bc=[0] * 6)
    slabs = product.VirtualSlabs(case, 2)
    for s in slabs.solvers:
        with pytest.raises(product.FoamYadeError) as e:
            s.set_field_average(["U"])
        assert "error 5" in str(e.value) and "slab" in str(e.value)                         # FY_ERR_UNSUPPORTED
    slabs.close()
    # the descriptor of a case applies at create: the same refusal there
    case.average = product.average_desc(["nut"])
    with pytest.raises(product.FoamYadeError) as e:
        product.Solver(case)
    assert "'nut'" in str(e.value)


def make_solver(product, fc, kind):
    if kind == "general":
        s = product.LduSolver.from_foam_case(fc)
    else:
        s = product.Solver(fc.case)
        U0, p0 = fc.initial_fields()
        s.set("U", U0); s.set("p", p0)
    s.hold_sources(True)
    return s


FILES = {"U": "U.water", "p": "p", "alpha": "alpha.water"}


@pytest.mark.parametrize("kind", KINDS)
def test_case_round_trip(product, tmp_path, kind):
    """bed_pimple with a fieldAverage object: the time directory holds the means, the prime2Means and the Properties file; a restart continues them exactly"""
    plain = case_copy(tmp_path / "plain", "bed_pimple", kind)
    dst = case_copy(tmp_path, "bed_pimple", kind)
    add_functions(dst, field_average([(FILES["U"], ON), ("p", ON), (FILES["alpha"], ON)], "restartOnRestart off;", name="avg"))
    cloud = bed_cloud((-0.025, -0.025, 0.005), (0.025, 0.025, 0.05), 300, 0.001 if kind == "block" else 0.003, 5)
    items = [("U", True), ("p", True), ("alpha", True)]

    fc = open_case(product, dst, 1, kind)
    assert fc.write_interval_steps == 5
    s = make_solver(product, fc, kind)
    n = s.n_cells
    ref, _, _ = run_against_restatement(s, items, n, fc.write_interval_steps, cloud, source="uSource" if kind == "block" else "uSourceCoupling")
    assert ref["alpha"].m.min() < 1.0
    tname = "%g" % (fc.start_time + fc.write_interval_steps * fc.delta_t)
    fc.write(s, tname)
    want = {"U.water", "p", "alpha.water"}
    averages = {f + suffix for f in FILES.values() for suffix in ("Mean", "Prime2Mean")}
    assert set(os.listdir(dst / tname)) == want | averages | {"uniform"}
    assert os.listdir(dst / tname / "uniform") == ["avgProperties"]
    text = (dst / tname / "U.waterPrime2Mean").read_text()
    assert "class       volSymmTensorField;" in text and f"nonuniform List<symmTensor> {n}" in text and "[0 2 -2 0 0 0 0]" in text and "calculated" in text
    first = text[text.index("(", text.index("List<symmTensor>")) + 1:].strip().splitlines()[0]
    assert re.fullmatch(r"\((\S+ ){5}\S+\)", first), first                        # six numbers per cell
    assert "class       volVectorField;" in (dst / tname / "U.waterMean").read_text() and "class       volScalarField;" in (dst / tname / "pPrime2Mean").read_text()
    props = (dst / tname / "uniform" / "avgProperties").read_text()
    for f in FILES.values():
        m = re.search(re.escape(f) + r"\s*\{\s*totalIter\s+6;\s*totalTime\s+(\S+);", props)                   # OpenFOAM's convention: N + 1, T + deltaT
        assert m and abs(float(m.group(1)) - 0.0012) < 1e-12, props

    # the same case without `functions` writes exactly what it wrote before
    fp = open_case(product, plain, 1, kind)
    sp = make_solver(product, fp, kind)
    sp.set_field_average(items)                                  # (averaging on the solver, but no function object in the case: nothing of it is written)
    sp.set_particles(cloud(0)); sp.step()
    fp.write(sp, tname)
    assert set(os.listdir(plain / tname)) == want
    sp.close(); fp.close()

    # restart from the written directory
    cd = dst / "system/controlDict"
    cd.write_text(cd.read_text().replace("startFrom       startTime;", "startFrom       latestTime;"))
    fc2 = open_case(product, dst, 1, kind)
    assert fc2.start_name == tname
    s2 = make_solver(product, fc2, kind)
    assert s2.average_state(0) == (0, 0.0)
    assert fc2.restore_averages(s2) == 3
    for q, nm in enumerate(ref):
        assert s2.average_state(q) == s.average_state(q) == (ref[nm].N, ref[nm].T)
        for suffix in ("Mean", "Prime2Mean"):
            np.testing.assert_array_equal(s2.get(nm + suffix), s.get(nm + suffix), err_msg=nm + suffix)       # 17 digits carry every double
    ref2 = {nm: far.Item(it.m.shape, True, "time", m=it.m, P=it.P, N=it.N, T=it.T) for nm, it in ref.items()}
    for step in range(2):                                         # two more steps equal the restatement seeded with what was restored
        s2.set_particles(cloud(5 + step)); s2.step()
        x = read_fields(s2, ref2, n)
        for nm, item in ref2.items():
            item.add(x[nm], s2.stats()["delta_t"])
    assert_averages(s2, ref2, None, None, "restart ")
    assert ref2["U"].N == 7
    s2.close(); fc2.close()

    # restartOnRestart on: from zero
    cd.write_text(cd.read_text().replace("restartOnRestart off;", "restartOnRestart on;"))
    fc3 = open_case(product, dst, 1, kind)
    s3 = make_solver(product, fc3, kind)
    assert fc3.restore_averages(s3) == 0 and s3.average_state(0) == (0, 0.0) and not s3.get("UMean").any()
    s3.close(); fc3.close()
    s.close(); fc.close()


def test_executable_writes_the_averages_and_names_what_it_ignores(product, tmp_path):
    exe = os.path.join(os.path.dirname(HERE), "yade-openfoam-coupling_amd", "bin", "foamYadeHip")
    if not os.path.exists(exe):
        pytest.fail("foamYadeHip has not been built: run __graft_entry__.build()")
    dst = case_copy(tmp_path, "bed_pimple", "block")
    body = field_average([("U.water", ON), ("p", ON), ("alpha.water", ON)], name="avg")
    add_functions(dst, body)
    out = subprocess.run([exe, "-solver", "pimple", "-case", str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "is not run" not in out.stdout and out.stdout.rstrip().endswith("End")
    times = sorted(d for d in os.listdir(dst) if d[0].isdigit())
    assert times == ["0", "0.001", "0.002"]
    for t in times[1:]:
        have = set(os.listdir(dst / t))
        assert {"U.waterMean", "U.waterPrime2Mean", "pMean", "pPrime2Mean", "alpha.waterMean", "alpha.waterPrime2Mean", "uniform"} <= have, (t, have)
        assert os.path.exists(dst / t / "uniform" / "avgProperties")
    assert re.search(r"totalIter\s+11;", (dst / "0.002" / "uniform" / "avgProperties").read_text())
    # one more function object, of a type that is not implemented: one line says so, and the run is the same
    other = case_copy(tmp_path / "other", "bed_pimple", "block")
    with open(other / "system/controlDict", "a") as f:
        f.write("\npurgeWrite 1;\n")
    add_functions(other, body + "    probes1 { type probes; libs (\"libsampling.so\"); fields (p); probeLocations ((0 0 0.01)); }\n")
    out2 = subprocess.run([exe, "-solver", "pimple", "-case", str(other)], capture_output=True, text=True, timeout=300)
    assert out2.returncode == 0, out2.stderr
    lines = [ln for ln in out2.stdout.splitlines() if "is not run" in ln]
    assert len(lines) == 1 and "probes1" in lines[0] and "probes" in lines[0]
    assert os.path.exists(other / "0.002" / "pMean")
    assert sorted(d for d in os.listdir(other) if d[0].isdigit()) == ["0", "0.002"]            # purgeWrite 1 took 0.001 with its uniform/ directory
